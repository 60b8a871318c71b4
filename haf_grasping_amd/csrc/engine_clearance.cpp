// engine_clearance.cpp -- haf_check_grasps (include/hafgrasp.h): the scene's points inside the gripper's boxes at n grasp poses, on the
// device.  Every refusal comes before any device work (check_clearance of clearance_host.cpp, then the capacity); the grasps become
// their twelve words by grasp_frame (clearance_host.cpp), on the host, in the pinned half of the call's block; then the frame goes
// through the single-frame input of engine_stage.cpp and a host mask through its upload_image, the grasps' words go up in one copy, the
// rows are zeroed, the two launches of clearance.hip run on the engine's stream, ONE copy brings back the rows and ONE synchronisation
// ends the call.  The derived fields, order and n_free are clearance_finish's (clearance_host.cpp) -- the code haf_check_grasps_ref
// ends with, on the same integers.  Nothing of the last scored batch is read or written: the stage timings are not touched; the
// block and the scratch are the ones every such call shares (call_io, call_scratch).
#include "engine_state.h"

#include <vector>

namespace haf_host {

using namespace haf_clear_math;

namespace {

// the call's block, device and pinned: [HAF_MAX_CHECK_GRASPS rows] -- so far it comes back -- [as many grasps' words]; behind them, the
// packed bytes of a host mask
constexpr size_t kClearRowBytes = (size_t)kClearRowWords * 4, kClearGraspBytes = (size_t)kClearGraspWords * 4;
constexpr size_t kClearGraspsAt = (size_t)HAF_MAX_CHECK_GRASPS * kClearRowBytes;
constexpr size_t kClearMaskAt = up16(kClearGraspsAt + (size_t)HAF_MAX_CHECK_GRASPS * kClearGraspBytes);

int check_grasps_impl(haf_engine *e, const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, int32_t n_grasps,
                      const void *grasps, size_t stride, haf_grasp_clearance *out, int32_t *order, int32_t *n_free)
{
    const std::string who = "haf_check_grasps: ";
    std::string why;
    int rc;
    ClearDev d;
    memset(&d, 0, sizeof d);
    if ((rc = check_clearance(frame, mask, gripper, n_grasps, grasps, stride, out, &d.b, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *frame;
    const size_t K = (size_t)n_grasps;
    const haf_roi m = mask ? *mask : haf_roi{};            // (no haf_roi, or one without a mask: the whole frame)
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    const size_t mp = (size_t)e->cfg.max_points, words = up16(mp * 4);
    // the scratch: [qx][qy][qz], max_points words each, every array at a multiple of 16 bytes (k_clear_points stores 16-byte pieces)
    CallBuffers cb;
    if ((rc = call_buffers(e, who, kClearMaskAt + mp, "the copy-back block", 3 * words, "the points' coordinate words", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host, *const scratch = cb.scratch;

    GraspWords *const gw = reinterpret_cast<GraspWords *>(host + kClearGraspsAt);
    grasp_frames(grasps, stride, n_grasps, d.b.reach_q, gw);
    if ((rc = frame_input_upload(e, f, *in, s, &d.f)) != HAF_OK) return rc;
    ImageDev md;
    if ((rc = upload_image(e, f, m.mask, m.on_device, m.row_stride_bytes, 1, cb, kClearMaskAt, &md)) != HAF_OK) return rc;
    d.mask = static_cast<const unsigned char *>(md.src); d.mask_stride = md.row_stride;
    d.n_grasps = n_grasps;
    d.qx = reinterpret_cast<int *>(scratch);
    d.qy = reinterpret_cast<int *>(scratch + words);
    d.qz = reinterpret_cast<int *>(scratch + 2 * words);
    d.grasps = reinterpret_cast<const int *>(dev + kClearGraspsAt);
    d.rows = reinterpret_cast<unsigned *>(dev);
    HIPCHK(e, hipMemcpyAsync(dev + kClearGraspsAt, gw, K * kClearGraspBytes, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemsetAsync(dev, 0, K * kClearRowBytes, s));        // the rows are accumulated into: the block carries some earlier call's bytes
    launch_clearance(d, s);
    if ((rc = call_finish(e, cb, K * kClearRowBytes)) != HAF_OK) return rc;
    std::vector<int32_t> rows(K * kClearRowWords);
    for (size_t k = 0; k < K; k++) clearance_row_decode(reinterpret_cast<const uint32_t *>(host + k * kClearRowBytes), &rows[k * kClearRowWords]);
    clearance_finish(*gripper, gw, rows.data(), n_grasps, out, order, n_free);
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_check_grasps(haf_engine *e, const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, int32_t n_grasps,
                     const void *grasps, size_t grasp_stride_bytes, haf_grasp_clearance *out, int32_t *order, int32_t *n_free)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return check_grasps_impl(e, frame, mask, gripper, n_grasps, grasps, grasp_stride_bytes, out, order, n_free); });
}

}  // extern "C"
