// space_host.cpp -- the host side of haf_check_space that needs neither a device nor an engine: haf_space_default, check_space -- every
// refusal of the views, the gripper, the grasp list and the parameters (both entry points apply it), which also forms THE constants of a
// call: the gripper's bounds (gripper_rules of clearance_host.cpp), the lattice (space_lattice) and every view's rules (transfer_rules
// of transfer_host.cpp for the camera the view is, frame_math of frames_host.cpp) --, space_finish -- clear, order and n_clear from the
// integer rows, which both call too -- and haf_check_space_ref, the definition of record of space_rules.h's rules; the kernel of
// space.hip is tested against it word for word.  Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "frames.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace haf {

using namespace haf_space_math;

namespace {

constexpr float kMinStep = 0.0005f, kMaxStep = 1.0f;
constexpr int64_t kSpaceMaxStates = (int64_t)1 << 22;     // bytes of `states` the call offers

// the haf_camera a view is read as; false when its pose cannot be inverted
bool view_camera(const haf_frame &f, haf_camera *cam)
{
    cam->width = f.width; cam->height = f.height;
    cam->fx = f.fx; cam->fy = f.fy; cam->cx = f.cx; cam->cy = f.cy;
    return haf_invert_pose(f.sensor_to_base, cam->base_to_camera) == HAF_OK;
}

// one 2- or 4-byte depth sample of a host view
uint32_t host_pixel(const haf_frame &f, int32_t u, int32_t v)
{
    const char *at = static_cast<const char *>(f.data) + (size_t)v * f.row_stride_bytes;
    if (f.kind == HAF_FRAME_DEPTH_U16) { uint16_t w; memcpy(&w, at + (size_t)u * 2, 2); return w; }
    uint32_t w;
    memcpy(&w, at + (size_t)u * 4, 4);
    return w;
}

}  // namespace

void space_lattice(const ClearBounds &b, int32_t S, SpaceLattice *l)
{
    memset(l, 0, sizeof *l);
    l->S = S;
    const int32_t box[SPACE_REGIONS][3][2] = {
        {{-b.half_open, b.half_open}, {-b.half_breadth, b.half_breadth}, {b.u0, b.u1}},
        {{-b.finger_out, -b.half_open}, {-b.half_breadth, b.half_breadth}, {b.u0, b.u1}},
        {{b.half_open, b.finger_out}, {-b.half_breadth, b.half_breadth}, {b.u0, b.u1}},
        {{-b.palm_half_w, b.palm_half_w}, {-b.palm_half_b, b.palm_half_b}, {b.u1, b.u2}},
    };
    int64_t total = 0;
    for (int r = 0; r < SPACE_REGIONS; r++) {
        bool flat = false;
        for (int a = 0; a < 3; a++) flat = flat || (int64_t)box[r][a][1] - (int64_t)box[r][a][0] <= 0;
        int64_t count = flat ? 0 : 1;
        for (int a = 0; a < 3; a++) {
            l->lo[r][a] = box[r][a][0]; l->hi[r][a] = box[r][a][1];
            const int64_t n = ((int64_t)box[r][a][1] - (int64_t)box[r][a][0]) / (int64_t)S;
            l->n[r][a] = flat ? 0 : (int32_t)(n < 1 ? 1 : n);
            count *= l->n[r][a];                          // (S >= W(0.0005) and hi - lo < 2^28: every n is below 2^13, a product below 2^39)
        }
        l->first[r] = (int32_t)(total < INT32_MAX ? total : INT32_MAX);
        total += count;
    }
    l->first[SPACE_REGIONS] = (int32_t)(total < INT32_MAX ? total : INT32_MAX);      // (above the cap: check_space refuses the call)
}

void space_info(const SpaceLattice &l, haf_space_info *info)
{
    memset(info, 0, sizeof *info);
    info->step = l.S;
    for (int r = 0; r < SPACE_REGIONS; r++)
        for (int a = 0; a < 3; a++) info->n[r][a] = l.n[r][a];
    info->n_samples = l.first[SPACE_REGIONS];
}

int check_space(const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params, int32_t n_grasps,
                const void *grasps, size_t grasp_stride_bytes, const haf_grasp_space *out, const uint8_t *states, SpaceCall *call, std::string &err)
{
    if (!views || !gripper || !params || !grasps || !out) { err = "null views, gripper, parameters, grasps or result"; return HAF_E_ARG; }
    if (check_grasp_list(gripper, n_grasps, grasp_stride_bytes, &call->b, err) != HAF_OK) return HAF_E_ARG;
    const haf_space_params &p = *params;
    if (!std::isfinite(p.sample_step) || !(p.sample_step >= kMinStep) || !(p.sample_step <= kMaxStep)) {
        err = "haf_space_params: sample_step outside 0.0005..1";
        return HAF_E_ARG;
    }
    if (check_projection_params("haf_space_params", p.near_m, p.tol_abs, p.tol_rel, err) != HAF_OK) return HAF_E_ARG;
    if (n_views < 1 || n_views > HAF_MAX_SPACE_VIEWS) { err = "n_views outside 1..HAF_MAX_SPACE_VIEWS"; return HAF_E_ARG; }
    const haf_transfer_params tp = {p.near_m, p.tol_abs, p.tol_rel, 0};
    for (int32_t k = 0; k < n_views; k++) {
        const haf_frame &f = views[k];
        const std::string which = "view " + std::to_string(k) + ": ";
        std::string why;
        const int rc = check_frame(f, why);
        if (rc != HAF_OK) { err = which + why; return rc; }
        if (f.kind != HAF_FRAME_DEPTH_U16 && f.kind != HAF_FRAME_DEPTH_F32) { err = which + "not a depth frame (an XYZ frame has no rays)"; return HAF_E_ARG; }
        haf_camera cam;
        if (!view_camera(f, &cam)) { err = which + "sensor_to_base cannot be inverted"; return HAF_E_ARG; }
        if (check_camera(cam, why) != HAF_OK) { err = which + why; return HAF_E_ARG; }
        SpaceViewRules &v = call->v[k];
        memset(&v, 0, sizeof v);
        v.r = transfer_rules(cam, tp);
        v.m = frame_math(f);
        v.kind = f.kind;
    }
    space_lattice(call->b, (int32_t)llrint((double)p.sample_step * (double)((int64_t)1 << kClearBoundShift)), &call->l);
    const int64_t N = call->l.first[SPACE_REGIONS];
    if (N > HAF_MAX_SPACE_SAMPLES) { err = "more than HAF_MAX_SPACE_SAMPLES lattice points: a larger sample_step is needed"; return HAF_E_ARG; }
    if (states && (int64_t)n_grasps * N > kSpaceMaxStates) { err = "states are offered for n_grasps * N <= 2^22 only"; return HAF_E_CAPACITY; }
    return HAF_OK;
}

void space_finish(const haf_space_params &p, const GraspWords *w, const int32_t *rows, int32_t n, haf_grasp_space *out, int32_t *order,
                  int32_t *n_clear)
{
    int32_t nc = 0;
    for (int32_t i = 0; i < n; i++) {
        haf_grasp_space &g = out[i];
        memset(&g, 0, sizeof g);
        if (w[i].reach_q < 0) { g.clear = -1; continue; }
        const int32_t *r = rows + (size_t)i * kSpaceRowWords;
        int64_t hit = 0, unknown = 0;
        for (int reg = 0; reg < SPACE_REGIONS; reg++) {
            for (int st = 0; st < SPACE_STATES; st++) g.n[reg][st] = r[reg * SPACE_STATES + st];
            if (reg == SPACE_BETWEEN) continue;
            hit += g.n[reg][SPACE_HIT];
            unknown += (int64_t)g.n[reg][SPACE_HIDDEN] + g.n[reg][SPACE_UNSEEN];
        }
        g.clear = (hit <= (int64_t)p.max_hit && unknown <= (int64_t)p.max_unknown && g.n[SPACE_BETWEEN][SPACE_HIT] >= p.min_between_hit) ? 1 : 0;
        if (g.clear == 1) {
            if (order) order[nc] = i;
            nc++;
        }
    }
    if (n_clear) *n_clear = nc;
}

namespace {

int check_space_ref_impl(const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params, int32_t n_grasps,
                         const void *grasps, size_t stride, haf_grasp_space *out, int32_t *order, int32_t *n_clear, haf_space_info *info,
                         uint8_t *states)
{
    std::string err;
    std::vector<SpaceCall> holder(1);
    SpaceCall &c = holder[0];
    int rc = check_space(views, n_views, gripper, params, n_grasps, grasps, stride, out, states, &c, err);
    if (rc != HAF_OK) return rc;
    for (int32_t k = 0; k < n_views; k++)
        if (views[k].on_device != 0) return HAF_E_ARG;    // (host memory only: this function touches no device)
    const int32_t N = c.l.first[SPACE_REGIONS];
    std::vector<GraspWords> w((size_t)n_grasps);
    grasp_frames(grasps, stride, n_grasps, c.b.reach_q, w.data());
    std::vector<int32_t> rows((size_t)n_grasps * kSpaceRowWords, 0);
    std::vector<int32_t> stu((size_t)N * 3);
    std::vector<uint8_t> region((size_t)N);
    for (int32_t j = 0; j < N; j++) region[(size_t)j] = (uint8_t)space_sample(c.l, j, &stu[(size_t)j * 3]);
    for (int32_t g = 0; g < n_grasps; g++) {
        uint8_t *st_row = states ? states + (size_t)g * (size_t)N : nullptr;
        if (st_row && N) memset(st_row, 0, (size_t)N);
        if (w[(size_t)g].reach_q < 0) continue;
        int32_t *row = &rows[(size_t)g * kSpaceRowWords];
        for (int32_t j = 0; j < N; j++) {
            int32_t Pq[3];
            float p[3];
            space_point(w[(size_t)g], &stu[(size_t)j * 3], Pq, p);
            int state = SPACE_UNSEEN;
            for (int32_t k = 0; k < n_views; k++) {
                int32_t Qz, uc, vc, Zobs;
                if (transfer_project(c.v[k].r, p, Qz, uc, vc) != TRANSFER_PROJECTS) continue;
                if (!space_observed(c.v[k], host_pixel(views[k], uc, vc), Zobs)) continue;
                const int s = space_state(c.v[k].r, Qz, Zobs);
                state = s > state ? s : state;
            }
            row[region[(size_t)j] * SPACE_STATES + state]++;
            if (st_row) st_row[j] = (uint8_t)state;
        }
    }
    space_finish(*params, w.data(), rows.data(), n_grasps, out, order, n_clear);
    if (info) space_info(c.l, info);
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_space_default(haf_space_params *p)
{
    if (!p) return;
    p->sample_step = 0.004f; p->near_m = 0.05f; p->tol_abs = 0.004f; p->tol_rel = 0.002f;
    p->max_hit = 0; p->max_unknown = 0; p->min_between_hit = 1;
}

// (no C++ exception may cross the C-ABI: a lattice too large for the host comes back as a status)
int haf_check_space_ref(const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params, int32_t n_grasps,
                        const void *grasps, size_t grasp_stride_bytes, haf_grasp_space *out, int32_t *order, int32_t *n_clear,
                        haf_space_info *info, uint8_t *states)
{
    try {
        return haf::check_space_ref_impl(views, n_views, gripper, params, n_grasps, grasps, grasp_stride_bytes, out, order, n_clear, info, states);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
