// opening_host.cpp -- the host side of haf_fit_openings that needs neither a device nor an engine: haf_opening_default, the checks (both
// entry points apply them: check_clearance's, with the parameters' largest opening in the gripper's place, and the parameters' own),
// opening_rules -- the integers of opening_rules.h from the gripper's and the parameters' doubles, once per call --, opening_finish --
// the derived fields, order and n_found from the integer rows, which both call --, haf_apply_opening and haf_fit_openings_ref, the
// definition of record; the kernels of opening.hip are tested against it word for word.  A grasp's words are grasp_frames' and the
// points' words clear_point_words' (clearance_host.cpp, clearance_rules.h).  Built with -ffp-contract=off like every unit.
#include "frames.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace haf {

using namespace haf_open_math;

namespace {
constexpr double kBoundOne = (double)(1 << kClearBoundShift);

int32_t bound_word(double metres) { return (int32_t)llrint(metres * kBoundOne); }      // (|metres| <= 2: fits)
}  // namespace

bool opening_rules(const haf_gripper &g, const haf_opening_params &p, OpenRules *r, std::string &why)
{
    const float dims[] = {p.min_opening, p.max_opening, p.max_shift};
    for (float x : dims)
        if (!std::isfinite(x) || x < 0.0f) { why = "haf_opening_params: an opening or the shift is negative or not finite"; return false; }
    if (p.max_hits < 0 || p.min_between < 0) { why = "haf_opening_params: max_hits or min_between is negative"; return false; }
    if (p.min_opening > p.max_opening) { why = "haf_opening_params: min_opening exceeds max_opening"; return false; }
    const char *far = "haf_fit_openings: the reach of the gripper at max_opening and max_shift exceeds 1 m";
    const double u1 = (double)g.finger_length - (double)g.tip_depth, u2 = u1 + (double)g.palm_height;
    const double et = std::max((double)g.finger_breadth, (double)g.palm_breadth) / 2;
    const double eu = std::max(std::max((double)g.tip_depth, std::fabs(u1)), std::fabs(u2));
    // (in metres first: past this every W below is at most 2^26)
    const double e_m = std::max((double)p.max_opening / 2 + (double)g.finger_thickness, (double)g.palm_width / 2) + (double)p.max_shift;
    if (!(std::sqrt(e_m * e_m + et * et + eu * eu) <= 1.0)) { why = far; return false; }
    const int32_t w_open = bound_word((double)p.max_opening / 2), w_thick = bound_word((double)g.finger_thickness);
    const int32_t w_palm = bound_word((double)g.palm_width / 2), w_shift = bound_word((double)p.max_shift);
    const int32_t E = std::max(w_open + w_thick, w_palm) + w_shift;
    int32_t shift = 0;
    while ((E >> shift) + 2 > kOpenBins / 2) shift++;
    const int32_t B = (int32_t)1 << shift;
    r->shift = shift;
    r->half_bins = (E >> shift) + 2;
    r->tb = (w_thick >> shift) + 1;
    r->pb = (w_palm >> shift) + 1;
    r->c_max = w_shift >> shift;
    r->j_min = std::max((int32_t)1, (bound_word((double)p.min_opening / 2) + B - 1) >> shift);
    r->j_max = w_open >> shift;
    if (r->j_max < r->j_min) { why = "haf_opening_params: no half opening of a whole bin between min_opening and max_opening (j_max < j_min)"; return false; }
    const double es = (double)r->half_bins * (double)B / kBoundOne;
    const double reach = std::sqrt(es * es + et * et + eu * eu);
    if (!(reach <= 1.0)) { why = far; return false; }
    r->half_breadth = bound_word((double)g.finger_breadth / 2);
    r->u0 = -bound_word((double)g.tip_depth);
    r->u1 = bound_word(u1);
    r->palm_half_b = bound_word((double)g.palm_breadth / 2);
    r->u2 = r->u1 + bound_word((double)g.palm_height);
    r->reach_q = (int32_t)std::ceil(reach * (double)kPlaneQuantum) + kClearReachMargin;
    r->max_hits = p.max_hits;
    r->min_between = p.min_between;
    return true;
}

int check_openings(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, const haf_opening_params *params, int32_t n_grasps,
                   const void *grasps, size_t grasp_stride_bytes, const haf_grasp_opening *out, OpenRules *rules, std::string &err)
{
    if (!params) { err = "null params"; return HAF_E_ARG; }
    if (!gripper) { err = "null frame, gripper, grasps or result"; return HAF_E_ARG; }
    // check_clearance's refusals, for the gripper at the largest opening asked for (the gripper's own is not read); an opening that is
    // no positive number yet is the parameters' to refuse, below
    haf_gripper widest = *gripper;
    widest.opening = std::isfinite(params->max_opening) && params->max_opening > 0.0f ? params->max_opening : 1e-3f;
    ClearBounds unused;
    const int rc = check_clearance(frame, mask, &widest, n_grasps, grasps, grasp_stride_bytes, reinterpret_cast<const haf_grasp_clearance *>(out),
                                   &unused, err);
    if (rc != HAF_OK) return rc;
    return opening_rules(*gripper, *params, rules, err) ? HAF_OK : HAF_E_ARG;
}

void opening_info(const OpenRules &r, haf_opening_info *info)
{
    memset(info, 0, sizeof *info);
    info->shift = r.shift; info->half_bins = r.half_bins; info->tb = r.tb; info->pb = r.pb;
    info->j_min = r.j_min; info->j_max = r.j_max; info->c_max = r.c_max;
    info->bin_m = (double)((int64_t)1 << r.shift) / kBoundOne;
}

// the host's search: a grasp's two histograms (2 x kOpenBins words) -> its row of kOpenRowWords words (found is 1 or 0)
static void opening_search(const OpenRules &r, const uint32_t *hist, int32_t *row)
{
    uint32_t pf[kOpenBins + 1], pp[kOpenBins + 1];
    pf[0] = pp[0] = 0;
    for (int k = 0; k < kOpenBins; k++) { pf[k + 1] = pf[k] + hist[k]; pp[k + 1] = pp[k] + hist[kOpenBins + k]; }
    memset(row, 0, sizeof(int32_t) * kOpenRowWords);
    row[OPEN_FINGER_SLAB] = (int32_t)pf[kOpenBins]; row[OPEN_PALM_SLAB] = (int32_t)pp[kOpenBins];
    int32_t counts[kOpenRowWords];
    for (int32_t p = 0, n = open_placements(r); p < n; p++) {
        int32_t j, c;
        open_placement(r, p, &j, &c);
        if (!open_counts(r, pf, pp, j, c, counts)) continue;
        row[OPEN_FOUND] = 1; row[OPEN_J] = j; row[OPEN_C] = c;
        for (int k = OPEN_BETWEEN; k <= OPEN_PALM; k++) row[k] = counts[k];
        break;
    }
    for (int32_t j = r.j_min; j <= r.j_max; j++)
        if (open_counts(r, pf, pp, j, 0, counts)) { row[OPEN_SYM_J] = j; break; }
}

void opening_finish(const OpenRules &r, const GraspWords *w, const int32_t *rows, int32_t n, haf_grasp_opening *out, int32_t *order,
                    int32_t *n_found)
{
    const double bin = (double)((int64_t)1 << r.shift) / kBoundOne;
    int32_t nf = 0;
    for (int32_t i = 0; i < n; i++) {
        haf_grasp_opening &o = out[i];
        memset(&o, 0, sizeof o);
        if (w[i].reach_q < 0) { o.found = -1; continue; }
        const int32_t *row = rows + (size_t)i * kOpenRowWords;
        o.found = row[OPEN_FOUND]; o.j = row[OPEN_J]; o.c = row[OPEN_C]; o.sym_j = row[OPEN_SYM_J];
        o.n_between = row[OPEN_BETWEEN]; o.n_finger[0] = row[OPEN_FINGER0]; o.n_finger[1] = row[OPEN_FINGER1]; o.n_palm = row[OPEN_PALM];
        o.n_finger_slab = row[OPEN_FINGER_SLAB]; o.n_palm_slab = row[OPEN_PALM_SLAB];
        o.opening_m = 2.0 * (double)o.j * bin; o.shift_m = (double)o.c * bin; o.sym_opening_m = 2.0 * (double)o.sym_j * bin;
        if (o.found == 1) {
            if (order) order[nf] = i;
            nf++;
        }
    }
    if (n_found) *n_found = nf;
}

namespace {

int fit_openings_ref_impl(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, const haf_opening_params *params,
                          int32_t n_grasps, const void *grasps, size_t stride, haf_grasp_opening *out, int32_t *order, int32_t *n_found,
                          haf_opening_info *info, uint32_t *hist_out)
{
    std::string err;
    OpenRules r;
    int rc = check_openings(frame, mask, gripper, params, n_grasps, grasps, stride, out, &r, err);
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
    grasp_frames(grasps, stride, n_grasps, r.reach_q, w.data());
    std::vector<int32_t> rows((size_t)n_grasps * kOpenRowWords, 0);
    std::vector<uint32_t> own(hist_out ? 0 : 2 * kOpenBins);
    for (int32_t k = 0; k < n_grasps; k++) {
        uint32_t *hist = hist_out ? hist_out + (size_t)k * 2 * kOpenBins : own.data();
        memset(hist, 0, sizeof(uint32_t) * 2 * kOpenBins);
        const GraspWords &gw = w[(size_t)k];
        if (gw.reach_q < 0) continue;
        for (size_t i = 0; i < n; i++) {
            const int32_t dx = qx[i] - gw.o[0], dy = qy[i] - gw.o[1], dz = qz[i] - gw.o[2];
            if (!clear_near(dx, dy, dz, gw.reach_q)) continue;
            const int32_t s = clear_dot(gw.c, dx, dy, dz), t = clear_dot(gw.b, dx, dy, dz), u = clear_dot(gw.a, dx, dy, dz);
            const int slab = open_slab(r, t, u);
            const int32_t bin = open_bin(s, r.shift);
            if (slab == OPEN_SLAB_NONE || !open_bin_counted(r, bin)) continue;
            hist[(slab == OPEN_SLAB_PALM ? kOpenBins : 0) + kOpenZero + bin]++;
        }
        opening_search(r, hist, &rows[(size_t)k * kOpenRowWords]);
    }
    opening_finish(r, w.data(), rows.data(), n_grasps, out, order, n_found);
    if (info) opening_info(r, info);
    return HAF_OK;
}

int apply_opening_impl(const haf_grasp_output *in, const haf_grasp_opening *opening, haf_grasp_output *out)
{
    if (!in || !opening || !out || opening->found != 1) return HAF_E_ARG;
    double a[3], b[3], c[3];
    if (!grasp_axes(*in, a, b, c)) return HAF_E_ARG;      // (a void grasp has no closing axis)
    haf_grasp_output o = *in;
    for (int j = 0; j < 3; j++) {
        const double centre = in->averaged_grasp_point[j] + opening->shift_m * c[j];
        o.averaged_grasp_point[j] = centre;
        o.grasp_point1[j] = centre - opening->opening_m / 2 * c[j];
        o.grasp_point2[j] = centre + opening->opening_m / 2 * c[j];
    }
    *out = o;
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_opening_default(haf_opening_params *p)
{
    if (!p) return;
    p->min_opening = 0.01f; p->max_opening = 0.08f; p->max_shift = 0.0f; p->max_hits = 0; p->min_between = 1;
}

// (no C++ exception may cross the C-ABI: a frame too large for the host comes back as a status)
int haf_fit_openings_ref(const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, const haf_opening_params *params,
                         int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes, haf_grasp_opening *out, int32_t *order,
                         int32_t *n_found, haf_opening_info *info, uint32_t *hist)
{
    try {
        return haf::fit_openings_ref_impl(frame, mask, gripper, params, n_grasps, grasps, grasp_stride_bytes, out, order, n_found, info, hist);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

int haf_apply_opening(const haf_grasp_output *in, const haf_grasp_opening *opening, haf_grasp_output *out)
{
    return haf::apply_opening_impl(in, opening, out);
}

}  // extern "C"
