// engine_space.cpp -- haf_check_space (include/hafgrasp.h): the sample points of the gripper's lattice at n grasp poses against 1..8
// depth views, on the device.  Every refusal comes before any device work (check_space of space_host.cpp, then the capacities); the
// grasps become their twelve words by grasp_frames (clearance_host.cpp), on the host, in the pinned half of the call's block; then the
// host views go up (upload_frame of engine_stage.cpp) into the raw area of haf_score_frames, each at a multiple of 16 bytes, as
// haf_filter_depth stages its stack -- a device-resident view is read where it lies --, the grasps' words go up in one copy, ONE memset
// zeroes the rows, ONE launch of k_space_samples (space.hip) runs on the engine's stream, ONE copy brings back the rows and ONE
// synchronisation ends the call; `states`, when asked for, lie in the scratch and take a copy of their own to the caller's memory.
// clear, order and n_clear are space_finish's (space_host.cpp) -- the code haf_check_space_ref ends with, on the same integers.
// Nothing of the last scored batch is read or written: the raw area is only read inside the call that filled it, the stage timings are
// not touched; the block and the scratch are the ones every such call shares (call_io, call_scratch).
#include "engine_state.h"

namespace haf_host {

using namespace haf_space_math;

namespace {

// the call's block, device and pinned: [n_grasps rows] -- so far it comes back -- [as many grasps' words]
constexpr size_t kSpaceRowBytes = (size_t)kSpaceRowWords * 4, kSpaceGraspBytes = (size_t)kClearGraspWords * 4;

int check_space_impl(haf_engine *e, const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params,
                     int32_t n_grasps, const void *grasps, size_t stride, haf_grasp_space *out, int32_t *order, int32_t *n_clear,
                     haf_space_info *info, uint8_t *states)
{
    const std::string who = "haf_check_space: ";
    std::string why;
    int rc;
    std::vector<SpaceCall> holder(1);
    SpaceCall &c = holder[0];
    if ((rc = check_space(views, n_views, gripper, params, n_grasps, grasps, stride, out, states, &c, why)) != HAF_OK) return fail(e, rc, who + why);
    const int64_t mp = (int64_t)e->cfg.max_points;
    // the raw area: [host views, each at a multiple of 16 bytes]
    size_t off[HAF_MAX_SPACE_VIEWS] = {}, at = 0;
    int64_t host_px = 0;
    for (int k = 0; k < n_views; k++) {
        const int64_t px = (int64_t)views[k].width * (int64_t)views[k].height;
        if (px > mp) return fail(e, HAF_E_CAPACITY, who + "view " + std::to_string(k) + ": more pixels than max_points");
        if (views[k].on_device == 1) continue;
        off[k] = at;
        at += staged_bytes(views[k]);
        if ((host_px += px) > mp) return fail(e, HAF_E_CAPACITY, who + "view " + std::to_string(k) + ": the host views hold more pixels than max_points");
    }
    if (at > e->raw.dev.n) return fail(e, HAF_E_CAPACITY, who + "the raw staging area is too small");
    const size_t K = (size_t)n_grasps, N = (size_t)c.l.first[SPACE_REGIONS];
    const size_t grasps_at = K * kSpaceRowBytes;
    CallBuffers cb;
    if ((rc = call_buffers(e, who, grasps_at + K * kSpaceGraspBytes, "the copy-back block", states ? K * N : 0, "the samples' states", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host;

    GraspWords *const gw = reinterpret_cast<GraspWords *>(host + grasps_at);
    grasp_frames(grasps, stride, n_grasps, c.b.reach_q, gw);
    std::vector<SpaceDev> dholder(1);
    SpaceDev &d = dholder[0];
    memset(&d, 0, sizeof d);
    d.l = c.l;
    for (int k = 0; k < n_views; k++) {
        const haf_frame &f = views[k];
        const FrameDev fd = describe_frame(f, e->raw.dev.p + off[k]);
        d.v[k] = c.v[k];
        d.src[k] = fd.src;
        d.row_stride[k] = fd.row_stride;
        if (f.on_device != 1 && (rc = upload_frame(e, f, e->raw.host + off[k], e->raw.dev.p + off[k], s)) != HAF_OK) return rc;
    }
    d.n_views = n_views; d.n_grasps = n_grasps;
    d.grasps = reinterpret_cast<const int *>(dev + grasps_at);
    d.rows = reinterpret_cast<unsigned *>(dev);
    d.states = states ? reinterpret_cast<unsigned char *>(cb.scratch) : nullptr;
    HIPCHK(e, hipMemcpyAsync(dev + grasps_at, gw, K * kSpaceGraspBytes, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemsetAsync(dev, 0, K * kSpaceRowBytes, s));        // the rows are accumulated into: the block carries some earlier call's bytes
    launch_space(d, s);
    HIPCHK(e, hipGetLastError());
    if (states && K * N) HIPCHK(e, hipMemcpyAsync(states, d.states, K * N, hipMemcpyDeviceToHost, s));
    if ((rc = call_finish(e, cb, K * kSpaceRowBytes)) != HAF_OK) return rc;
    space_finish(*params, gw, reinterpret_cast<const int32_t *>(host), n_grasps, out, order, n_clear);
    if (info) space_info(c.l, info);
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_check_space(haf_engine *e, const haf_frame *views, int32_t n_views, const haf_gripper *gripper, const haf_space_params *params,
                    int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes, haf_grasp_space *out, int32_t *order, int32_t *n_clear,
                    haf_space_info *info, uint8_t *states)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] {
        return check_space_impl(e, views, n_views, gripper, params, n_grasps, grasps, grasp_stride_bytes, out, order, n_clear, info, states);
    });
}

}  // extern "C"
