// clearance_host.cpp -- the host side of haf_check_grasps that needs neither a device nor an engine: haf_gripper_default, the checks of
// the frame, the mask, the gripper and the grasp list (both entry points apply them), gripper_rules -- the gripper's integer bounds and
// its reach --, grasp_axes and grasp_frame -- THE axes of a grasp in double and its twelve words, which both entry points call --, clearance_finish -- the derived
// fields, order and n_free from the integer rows, which both call too -- and haf_check_grasps_ref, the definition of record of
// clearance_rules.h's rules; the kernels of clearance.hip are tested against it word for word.  Built with -ffp-contract=off like every
// unit (build.py: FLAGS).
#include "frames.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace haf {

using namespace haf_clear_math;

namespace {
constexpr int64_t kClearMaxPixels = (int64_t)1 << 28;     // haf_fit_plane's bound: the counts stay below 2^31
constexpr double kBoundOne = (double)(1 << kClearBoundShift);

int32_t bound_word(double metres) { return (int32_t)llrint(metres * kBoundOne); }      // (|metres| <= 2: fits)
}  // namespace

bool gripper_rules(const haf_gripper &g, ClearBounds *b)
{
    const float dims[] = {g.opening, g.finger_thickness, g.finger_breadth, g.tip_depth, g.finger_length, g.palm_width, g.palm_breadth, g.palm_height};
    for (float x : dims)
        if (!std::isfinite(x) || x < 0.0f) return false;
    if (!(g.opening > 0.0f)) return false;
    const double half_open = (double)g.opening / 2, finger_out = half_open + (double)g.finger_thickness;
    const double u1 = (double)g.finger_length - (double)g.tip_depth, u2 = u1 + (double)g.palm_height;
    // the box that bounds all four regions, about the grasp point
    const double es = std::max(finger_out, (double)g.palm_width / 2), et = std::max((double)g.finger_breadth, (double)g.palm_breadth) / 2;
    const double eu = std::max(std::max((double)g.tip_depth, std::fabs(u1)), std::fabs(u2));
    const double reach = std::sqrt(es * es + et * et + eu * eu);
    if (!(reach <= 1.0)) return false;                    // (every dimension is then at most 2 m: its W fits an int32)
    b->half_open = bound_word(half_open);
    b->finger_out = bound_word(finger_out);
    b->half_breadth = bound_word((double)g.finger_breadth / 2);
    b->u0 = -bound_word((double)g.tip_depth);
    b->u1 = bound_word(u1);
    b->palm_half_w = bound_word((double)g.palm_width / 2);
    b->palm_half_b = bound_word((double)g.palm_breadth / 2);
    b->u2 = b->u1 + bound_word((double)g.palm_height);
    b->reach_q = (int32_t)std::ceil(reach * (double)kPlaneQuantum) + kClearReachMargin;
    return true;
}

int check_clearance(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, int32_t n_grasps, const void *grasps,
                    size_t grasp_stride_bytes, const haf_grasp_clearance *out, ClearBounds *bounds, std::string &err)
{
    if (!frame || !gripper || !grasps || !out) { err = "null frame, gripper, grasps or result"; return HAF_E_ARG; }
    const int rc = check_frame(*frame, err);
    if (rc != HAF_OK) return rc;
    if (mask && mask->mask) {
        if (mask->on_device != 0 && mask->on_device != 1) { err = "the mask's on_device must be 0 (host) or 1 (device)"; return HAF_E_ARG; }
        if (mask->row_stride_bytes < (size_t)frame->width) { err = "the mask's row stride is smaller than the width"; return HAF_E_ARG; }
    }
    if (check_grasp_list(gripper, n_grasps, grasp_stride_bytes, bounds, err) != HAF_OK) return HAF_E_ARG;
    if ((int64_t)frame->width * (int64_t)frame->height > kClearMaxPixels) { err = "a frame of more than 2^28 pixels"; return HAF_E_CAPACITY; }
    return HAF_OK;
}

int check_grasp_list(const haf_gripper *gripper, int32_t n_grasps, size_t grasp_stride_bytes, ClearBounds *bounds, std::string &err)
{
    if (!gripper_rules(*gripper, bounds)) {
        err = "haf_gripper: a dimension is negative or not finite, opening is not positive, or the reach exceeds 1 m";
        return HAF_E_ARG;
    }
    if (n_grasps < 1 || n_grasps > HAF_MAX_CHECK_GRASPS) { err = "n_grasps outside 1..HAF_MAX_CHECK_GRASPS"; return HAF_E_ARG; }
    if (grasp_stride_bytes < sizeof(haf_grasp_output) || grasp_stride_bytes % 8 != 0) {
        err = "the grasp stride is below sizeof(haf_grasp_output) or not a multiple of 8";
        return HAF_E_ARG;
    }
    return HAF_OK;
}

bool grasp_axes(const haf_grasp_output &g, double *a, double *b, double *c)
{
    const double *in[4] = {g.grasp_point1, g.grasp_point2, g.averaged_grasp_point, g.approach_vector};
    for (const double *v : in)
        for (int j = 0; j < 3; j++)
            if (!std::isfinite(v[j])) return false;
    double gv[3];
    const double an = std::sqrt(g.approach_vector[0] * g.approach_vector[0] + g.approach_vector[1] * g.approach_vector[1] +
                                g.approach_vector[2] * g.approach_vector[2]);
    if (!(an >= 1e-6)) return false;
    for (int j = 0; j < 3; j++) { a[j] = g.approach_vector[j] / an; gv[j] = g.grasp_point2[j] - g.grasp_point1[j]; }
    const double gn = std::sqrt(gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2]);
    if (!(gn >= 1e-6)) return false;
    const double ga = gv[0] * a[0] + gv[1] * a[1] + gv[2] * a[2];
    for (int j = 0; j < 3; j++) c[j] = gv[j] - ga * a[j];
    const double cn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (!(cn >= 1e-3 * gn)) return false;
    for (int j = 0; j < 3; j++) {
        c[j] /= cn;
        if (std::fabs(g.averaged_grasp_point[j]) > 16.0) return false;
    }
    b[0] = a[1] * c[2] - a[2] * c[1]; b[1] = a[2] * c[0] - a[0] * c[2]; b[2] = a[0] * c[1] - a[1] * c[0];
    return true;
}

void grasp_frame(const haf_grasp_output &g, int32_t reach_q, GraspWords *w)
{
    memset(w, 0, sizeof *w);
    w->reach_q = -1;                                      // void until every test has passed
    double a[3], b[3], c[3];
    if (!grasp_axes(g, a, b, c)) return;
    for (int j = 0; j < 3; j++) {
        w->a[j] = (int32_t)lrint((double)kClearAxisOne * a[j]);
        w->b[j] = (int32_t)lrint((double)kClearAxisOne * b[j]);
        w->c[j] = (int32_t)lrint((double)kClearAxisOne * c[j]);
        w->o[j] = (int32_t)lrint((double)kPlaneQuantum * g.averaged_grasp_point[j]);
    }
    w->reach_q = reach_q;
}

void grasp_frames(const void *grasps, size_t stride, int32_t n, int32_t reach_q, GraspWords *w)
{
    for (int32_t i = 0; i < n; i++) {
        haf_grasp_output g;
        memcpy(&g, static_cast<const char *>(grasps) + (size_t)i * stride, sizeof g);
        grasp_frame(g, reach_q, &w[i]);
    }
}

void clearance_row_decode(const uint32_t *dev_row, int32_t *row)
{
    for (int j = 0; j <= CLEAR_BETWEEN; j++) row[j] = (int32_t)dev_row[j];
    const bool any = row[CLEAR_BETWEEN] > 0;
    row[CLEAR_SMIN] = any ? ~haf_shape_math::shape_dec(dev_row[CLEAR_SMIN]) : 0;
    row[CLEAR_SMAX] = any ? haf_shape_math::shape_dec(dev_row[CLEAR_SMAX]) : 0;
    row[CLEAR_UMAX] = any ? haf_shape_math::shape_dec(dev_row[CLEAR_UMAX]) : 0;
}

void clearance_finish(const haf_gripper &g, const GraspWords *w, const int32_t *rows, int32_t n, haf_grasp_clearance *out, int32_t *order,
                      int32_t *n_free)
{
    const double unit = 1.0 / kBoundOne;
    int32_t nf = 0;
    for (int32_t i = 0; i < n; i++) {
        haf_grasp_clearance &c = out[i];
        memset(&c, 0, sizeof c);
        if (w[i].reach_q < 0) { c.free = -1; continue; }
        const int32_t *r = rows + (size_t)i * kClearRowWords;
        c.n_near = r[CLEAR_NEAR]; c.n_finger[0] = r[CLEAR_FINGER0]; c.n_finger[1] = r[CLEAR_FINGER1]; c.n_palm = r[CLEAR_PALM];
        c.n_between = r[CLEAR_BETWEEN];
        if (c.n_between > 0) {
            c.s_min = r[CLEAR_SMIN]; c.s_max = r[CLEAR_SMAX]; c.u_max = r[CLEAR_UMAX];
            c.width_m = (double)((int64_t)c.s_max - (int64_t)c.s_min) * unit;
            c.offset_m = (double)((int64_t)c.s_max + (int64_t)c.s_min) * unit / 2;
            c.top_m = (double)c.u_max * unit;
        }
        const int64_t hits = (int64_t)c.n_finger[0] + c.n_finger[1] + c.n_palm;
        c.free = (hits <= (int64_t)g.max_hits && c.n_between >= g.min_between) ? 1 : 0;
        if (c.free == 1) {
            if (order) order[nf] = i;
            nf++;
        }
    }
    if (n_free) *n_free = nf;
}

namespace {

int check_grasps_ref_impl(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, int32_t n_grasps, const void *grasps,
                          size_t stride, haf_grasp_clearance *out, int32_t *order, int32_t *n_free)
{
    std::string err;
    ClearBounds b;
    int rc = check_clearance(frame, mask, gripper, n_grasps, grasps, stride, out, &b, err);
    if (rc != HAF_OK) return rc;
    const bool masked = mask && mask->mask;
    if (frame->on_device != 0 || (masked && mask->on_device != 0)) return HAF_E_ARG;      // (host memory only: this function touches no device)
    const size_t W = (size_t)frame->width, H = (size_t)frame->height, n = W * H;
    std::vector<float> xyz(n * 3);
    if ((rc = haf_frame_points(frame, xyz.data())) != HAF_OK) return rc;
    std::vector<int32_t> qx(n), qy(n), qz(n);
    for (size_t i = 0; i < n; i++) {
        int32_t q[3];
        clear_point_words(&xyz[3 * i], !masked || mask->mask[(i / W) * mask->row_stride_bytes + i % W] != 0, q);
        qx[i] = q[0]; qy[i] = q[1]; qz[i] = q[2];
    }
    std::vector<GraspWords> w((size_t)n_grasps);
    grasp_frames(grasps, stride, n_grasps, b.reach_q, w.data());
    std::vector<int32_t> rows((size_t)n_grasps * kClearRowWords, 0);
    for (int32_t k = 0; k < n_grasps; k++) {
        const GraspWords &gw = w[(size_t)k];
        if (gw.reach_q < 0) continue;
        int32_t *r = &rows[(size_t)k * kClearRowWords];
        int32_t smin = INT32_MAX, smax = INT32_MIN, umax = INT32_MIN;
        for (size_t i = 0; i < n; i++) {
            const int32_t dx = qx[i] - gw.o[0], dy = qy[i] - gw.o[1], dz = qz[i] - gw.o[2];
            if (!clear_near(dx, dy, dz, gw.reach_q)) continue;
            r[CLEAR_NEAR]++;
            const int32_t s = clear_dot(gw.c, dx, dy, dz), t = clear_dot(gw.b, dx, dy, dz), u = clear_dot(gw.a, dx, dy, dz);
            switch (clear_region(b, s, t, u)) {
            case CLEAR_REGION_BETWEEN:
                r[CLEAR_BETWEEN]++;
                smin = s < smin ? s : smin; smax = s > smax ? s : smax; umax = u > umax ? u : umax;
                break;
            case CLEAR_REGION_FINGER0: r[CLEAR_FINGER0]++; break;
            case CLEAR_REGION_FINGER1: r[CLEAR_FINGER1]++; break;
            case CLEAR_REGION_PALM: r[CLEAR_PALM]++; break;
            default: break;
            }
        }
        if (r[CLEAR_BETWEEN] > 0) { r[CLEAR_SMIN] = smin; r[CLEAR_SMAX] = smax; r[CLEAR_UMAX] = umax; }
    }
    clearance_finish(*gripper, w.data(), rows.data(), n_grasps, out, order, n_free);
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_gripper_default(haf_gripper *g)
{
    if (!g) return;
    g->opening = 0.08f; g->finger_thickness = 0.01f; g->finger_breadth = 0.02f; g->tip_depth = 0.03f; g->finger_length = 0.06f;
    g->palm_width = 0.12f; g->palm_breadth = 0.04f; g->palm_height = 0.04f;
    g->max_hits = 0; g->min_between = 1;
}

// (no C++ exception may cross the C-ABI: a frame too large for the host comes back as a status)
int haf_check_grasps_ref(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, int32_t n_grasps, const void *grasps,
                         size_t grasp_stride_bytes, haf_grasp_clearance *out, int32_t *order, int32_t *n_free)
{
    try {
        return haf::check_grasps_ref_impl(frame, mask, gripper, n_grasps, grasps, grasp_stride_bytes, out, order, n_free);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
