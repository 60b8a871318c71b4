// engine_opening.cpp -- haf_fit_openings (include/hafgrasp.h): the smallest free opening of the gripper at n grasp poses, on the device.
// Every refusal comes before any device work (check_openings of opening_host.cpp, then the capacity); the grasps become their twelve
// words by grasp_frames (clearance_host.cpp), on the host, in the pinned half of the call's block; then the frame goes through the
// single-frame input of engine_stage.cpp and a host mask through its upload_image, the grasps' words go up in one copy, the histograms
// of n_grasps grasps are zeroed, the three launches of opening.hip run on the engine's stream, ONE copy brings back the rows -- and,
// only when the caller asked for them, the histograms behind them -- and ONE synchronisation ends the call.  The derived fields, order
// and n_found are opening_finish's (opening_host.cpp) -- the code haf_fit_openings_ref ends with, on the same integers.  Nothing of the
// last scored batch is read or written: the stage timings are not touched; the block and the scratch are the ones every such call
// shares (call_io, call_scratch).
#include "engine_state.h"

namespace haf_host {

using namespace haf_open_math;

namespace {

// the call's block, device and pinned: [HAF_MAX_CHECK_GRASPS grasps' words] [the packed bytes of a host mask, max_points] [n_grasps rows]
// [n_grasps grasps' histograms, when they are asked for] -- the last two come back in one copy.  The scratch: [qx][qy][qz] and, when
// nobody asked for them, the histograms
constexpr size_t kOpenRowBytes = (size_t)kOpenRowWords * 4, kOpenGraspBytes = (size_t)kClearGraspWords * 4;
constexpr size_t kOpenHistBytes = (size_t)2 * kOpenBins * 4;
constexpr size_t kOpenMaskAt = up16((size_t)HAF_MAX_CHECK_GRASPS * kOpenGraspBytes);

int fit_openings_impl(haf_engine *e, const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, const haf_opening_params *params,
                      int32_t n_grasps, const void *grasps, size_t stride, haf_grasp_opening *out, int32_t *order, int32_t *n_found,
                      haf_opening_info *info, uint32_t *hist)
{
    const std::string who = "haf_fit_openings: ";
    std::string why;
    int rc;
    OpenDev d;
    memset(&d, 0, sizeof d);
    if ((rc = check_openings(frame, mask, gripper, params, n_grasps, grasps, stride, out, &d.r, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *frame;
    const size_t K = (size_t)n_grasps;
    const haf_roi m = mask ? *mask : haf_roi{};            // (no haf_roi, or one without a mask: the whole frame)
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    const size_t mp = (size_t)e->cfg.max_points, words = up16(mp * 4), rows_at = up16(kOpenMaskAt + mp);
    const size_t back = K * (kOpenRowBytes + (hist ? kOpenHistBytes : 0));      // what comes back: the rows, the histograms when asked for
    CallBuffers cb;
    if ((rc = call_buffers(e, who, rows_at + back, "the copy-back block", 3 * words + (hist ? 0 : K * kOpenHistBytes),
                           "the points' coordinate words and the histograms", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host, *const scratch = cb.scratch;

    GraspWords *const gw = reinterpret_cast<GraspWords *>(host);
    grasp_frames(grasps, stride, n_grasps, d.r.reach_q, gw);
    if ((rc = frame_input_upload(e, f, *in, s, &d.c.f)) != HAF_OK) return rc;
    ImageDev md;
    if ((rc = upload_image(e, f, m.mask, m.on_device, m.row_stride_bytes, 1, cb, kOpenMaskAt, &md)) != HAF_OK) return rc;
    d.c.mask = static_cast<const unsigned char *>(md.src); d.c.mask_stride = md.row_stride;
    d.c.n_grasps = n_grasps;
    d.c.qx = reinterpret_cast<int *>(scratch);
    d.c.qy = reinterpret_cast<int *>(scratch + words);
    d.c.qz = reinterpret_cast<int *>(scratch + 2 * words);
    d.c.grasps = reinterpret_cast<const int *>(dev);
    d.rows = reinterpret_cast<int *>(dev + rows_at);
    const size_t hist_at = rows_at + K * kOpenRowBytes;    // (behind the rows of THIS call: one copy brings both)
    d.hist = reinterpret_cast<unsigned *>(hist ? dev + hist_at : scratch + 3 * words);
    HIPCHK(e, hipMemcpyAsync(dev, gw, K * kOpenGraspBytes, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemsetAsync(d.hist, 0, K * kOpenHistBytes, s));      // accumulated into: the memory carries some earlier call's bytes
    launch_openings(d, s);
    if ((rc = call_finish(e, cb, back, rows_at)) != HAF_OK) return rc;
    opening_finish(d.r, gw, reinterpret_cast<const int32_t *>(host + rows_at), n_grasps, out, order, n_found);
    if (info) opening_info(d.r, info);
    if (hist) memcpy(hist, host + hist_at, K * kOpenHistBytes);
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_fit_openings(haf_engine *e, const haf_frame *frame, const haf_roi *mask, const haf_gripper *gripper, const haf_opening_params *params,
                     int32_t n_grasps, const void *grasps, size_t grasp_stride_bytes, haf_grasp_opening *out, int32_t *order,
                     int32_t *n_found, haf_opening_info *info, uint32_t *hist)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] {
        return fit_openings_impl(e, frame, mask, gripper, params, n_grasps, grasps, grasp_stride_bytes, out, order, n_found, info, hist);
    });
}

}  // extern "C"
