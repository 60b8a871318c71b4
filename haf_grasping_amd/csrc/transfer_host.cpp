// transfer_host.cpp -- the host side of haf_transfer_labels that needs neither a device nor an engine: haf_transfer_default,
// haf_invert_pose, the checks of the depth frame, the camera, the camera's label image, the parameters and the output (both entry points
// apply them), transfer_rules -- THE constants of a call, which both entry points form here -- and haf_transfer_labels_ref, the
// definition of record of transfer_rules.h's rules; the device kernels of transfer.hip are tested against it word for word.  Built with
// -ffp-contract=off like every unit (build.py: FLAGS).
#include "frame_stage.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using namespace haf_transfer_math;

namespace {

constexpr int32_t kMaxCameraSide = 32768;
constexpr float kMinFocal = 1.0f / 256.0f, kMaxFocal = 32768.0f, kMaxCentre = 32768.0f;
constexpr float kMinNear = 0.001f, kMaxNear = 16.0f;
constexpr int32_t kMaxSplat = 2;

bool in_range(float x, float lo, float hi) { return std::isfinite(x) && x >= lo && x <= hi; }

// round to nearest even of a double that fits int64 (the default rounding mode)
int64_t rne(double x) { return (int64_t)std::nearbyint(x); }

}  // namespace

int check_camera(const haf_camera &cam, std::string &err)
{
    if (cam.width < 1 || cam.width > kMaxCameraSide || cam.height < 1 || cam.height > kMaxCameraSide) {
        err = "haf_camera: width or height outside 1..32768";
        return HAF_E_ARG;
    }
    if (!in_range(cam.fx, kMinFocal, kMaxFocal) || !in_range(cam.fy, kMinFocal, kMaxFocal)) { err = "haf_camera: fx or fy outside 1/256..32768"; return HAF_E_ARG; }
    if (!in_range(cam.cx, -kMaxCentre, kMaxCentre) || !in_range(cam.cy, -kMaxCentre, kMaxCentre)) { err = "haf_camera: |cx| or |cy| above 32768"; return HAF_E_ARG; }
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(cam.base_to_camera[i])) { err = "haf_camera: base_to_camera has an entry that is not finite"; return HAF_E_ARG; }
    return HAF_OK;
}

int check_projection_params(const char *name, float near_m, float tol_abs, float tol_rel, std::string &err)
{
    const std::string n = name;
    if (!in_range(near_m, kMinNear, kMaxNear)) { err = n + ": near_m outside 0.001..16"; return HAF_E_ARG; }
    if (!std::isfinite(tol_abs) || !(tol_abs >= 0.0f)) { err = n + ": tol_abs must be finite and not negative"; return HAF_E_ARG; }
    if (!in_range(tol_rel, 0.0f, 1.0f)) { err = n + ": tol_rel outside 0..1"; return HAF_E_ARG; }
    return HAF_OK;
}

int check_transfer(const haf_frame *depth, const haf_camera *cam, const haf_label_image *l, int32_t n_labels, const haf_transfer_params *p,
                   const void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t out_on_device, std::string &err)
{
    if (!depth || !cam || !l || !p) { err = "null depth frame, camera, camera labels or parameters"; return HAF_E_ARG; }
    int rc = check_frame(*depth, err);
    if (rc != HAF_OK) return rc;
    if ((rc = check_label_output(*depth, labels, elem_bytes, row_stride_bytes, out_on_device, err)) != HAF_OK) return rc;
    if ((rc = check_camera(*cam, err)) != HAF_OK) return rc;
    if ((rc = check_projection_params("haf_transfer_params", p->near_m, p->tol_abs, p->tol_rel, err)) != HAF_OK) return rc;
    if (p->splat < 0 || p->splat > kMaxSplat) { err = "haf_transfer_params: splat outside 0..2"; return HAF_E_ARG; }
    if ((rc = check_label_image(l, cam->width, n_labels, err)) != HAF_OK) return rc;      // (the CAMERA's width: its image is the camera's)
    if (elem_bytes == 1 && n_labels > 255) { err = "n_labels above 255 with a uint8 output"; return HAF_E_ARG; }
    if (labels && l->on_device == out_on_device &&
        spans_overlap(image_span(labels, (size_t)depth->height, row_stride_bytes, (size_t)depth->width * (size_t)elem_bytes),
                      label_span(*l, cam->width, cam->height))) {
        err = "labels overlaps the camera's label image";
        return HAF_E_ARG;
    }
    return HAF_OK;
}

TransferRules transfer_rules(const haf_camera &cam, const haf_transfer_params &p)
{
    TransferRules r;
    memcpy(r.m, cam.base_to_camera, sizeof r.m);
    r.FX = (int32_t)rne((double)cam.fx * 256.0); r.FY = (int32_t)rne((double)cam.fy * 256.0);
    r.CX = (int32_t)rne((double)cam.cx * 256.0); r.CY = (int32_t)rne((double)cam.cy * 256.0);
    const int64_t near_w = rne((double)p.near_m * 65536.0);
    r.NEAR = (int32_t)(near_w < 1 ? 1 : near_w);
    const double ta = std::nearbyint((double)p.tol_abs * 65536.0);
    r.TA = ta >= (double)INT32_MAX ? INT32_MAX : (int32_t)ta;
    r.TR = (int32_t)rne((double)p.tol_rel * 65536.0);
    r.width = cam.width; r.height = cam.height;
    r.splat = p.splat;
    return r;
}

namespace {

int transfer_ref_impl(const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                      const haf_transfer_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t *zbuffer, int64_t *stats)
{
    std::string err;
    int rc = check_transfer(depth, cam, cam_labels, n_labels, p, labels, elem_bytes, row_stride_bytes, 0, err);
    if (rc != HAF_OK) return rc;
    if (depth->on_device != 0 || cam_labels->on_device != 0) return HAF_E_ARG;      // (host memory only: this function touches no device)
    const size_t W = (size_t)depth->width, H = (size_t)depth->height, n = W * H;
    const size_t Wc = (size_t)cam->width, Hc = (size_t)cam->height;
    std::vector<float> xyz(n * 3);
    if ((rc = haf_frame_points(depth, xyz.data())) != HAF_OK) return rc;
    const TransferRules r = transfer_rules(*cam, *p);
    std::vector<int32_t> Z(Wc * Hc, kTransferEmpty);
    int64_t front = 0, projects = 0, visible = 0, labelled = 0;
    for (size_t i = 0; i < n; i++) {
        int32_t Qz, uc, vc;
        const int stage = transfer_project(r, &xyz[3 * i], Qz, uc, vc);
        front += stage >= TRANSFER_FRONT;
        if (stage != TRANSFER_PROJECTS) continue;
        projects++;
        const int32_t u_lo = uc - r.splat < 0 ? 0 : uc - r.splat, u_hi = uc + r.splat >= r.width ? r.width - 1 : uc + r.splat;
        const int32_t v_lo = vc - r.splat < 0 ? 0 : vc - r.splat, v_hi = vc + r.splat >= r.height ? r.height - 1 : vc + r.splat;
        for (int32_t v = v_lo; v <= v_hi; v++)
            for (int32_t u = u_lo; u <= u_hi; u++) {
                int32_t &z = Z[(size_t)v * Wc + (size_t)u];
                z = Qz < z ? Qz : z;
            }
    }
    for (size_t v = 0; v < H; v++)
        for (size_t u = 0; u < W; u++) {
            int32_t Qz, uc, vc;
            uint32_t l = 0;
            if (transfer_project(r, &xyz[3 * (v * W + u)], Qz, uc, vc) == TRANSFER_PROJECTS &&
                transfer_visible(r, Qz, Z[(size_t)vc * Wc + (size_t)uc])) {
                visible++;
                l = transfer_label(load_label(*cam_labels, (size_t)uc, (size_t)vc), n_labels);
            }
            labelled += l != 0;
            store_label(labels, row_stride_bytes, elem_bytes, u, v, (uint32_t)l);
        }
    if (zbuffer) memcpy(zbuffer, Z.data(), Z.size() * sizeof(int32_t));
    if (stats) { stats[0] = (int64_t)n; stats[1] = front; stats[2] = projects; stats[3] = visible; stats[4] = labelled; }
    return HAF_OK;
}

int invert_pose_impl(const float *pose, float *inverse)
{
    if (!pose || !inverse) return HAF_E_ARG;
    double a[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++)
            if (!std::isfinite(pose[4 * r + c])) return HAF_E_ARG;
        for (int c = 0; c < 3; c++) a[r][c] = (double)pose[4 * r + c];
        t[r] = (double)pose[4 * r + 3];
    }
    // adj[r][c] = the cofactor of a[c][r]
    double adj[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            adj[r][c] = a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1];
        }
    const double det = a[0][0] * adj[0][0] + a[0][1] * adj[1][0] + a[0][2] * adj[2][0];
    if (!std::isfinite(det) || std::fabs(det) < 1e-12) return HAF_E_ARG;
    float out[12];
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
        for (int c = 0; c < 3; c++) {
            const double v = adj[r][c] / det;
            out[4 * r + c] = (float)v;
            s += v * t[c];
        }
        out[4 * r + 3] = (float)(-s);
    }
    memcpy(inverse, out, sizeof out);                     // (inverse may be pose itself)
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_transfer_default(haf_transfer_params *p)
{
    if (!p) return;
    p->near_m = 0.05f; p->tol_abs = 0.01f; p->tol_rel = 0.01f; p->splat = 1;
}

int haf_invert_pose(const float pose[12], float inverse[12]) { return haf::invert_pose_impl(pose, inverse); }

// (no C++ exception may cross the C-ABI: an image too large for the host comes back as a status)
int haf_transfer_labels_ref(const haf_frame *depth, const haf_camera *cam, const haf_label_image *cam_labels, int32_t n_labels,
                            const haf_transfer_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes, int32_t *zbuffer,
                            int64_t *stats)
{
    try {
        return haf::transfer_ref_impl(depth, cam, cam_labels, n_labels, p, labels, elem_bytes, row_stride_bytes, zbuffer, stats);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
