// engine_plane.cpp -- haf_fit_plane (include/hafgrasp.h): the dominant plane of one sensor frame, on the device.  Every refusal comes
// before any device work (check_plane of plane_host.cpp, then the capacity); then the frame goes through the single-frame input of
// engine_stage.cpp and a host mask through its upload_image, the five launches of plane.hip run on the engine's stream, ONE copy brings
// back the counters, the moments, the counts and the hypothesis words, and ONE synchronisation ends the call.  The plane itself is
// plane_finish's (plane_host.cpp) -- the code haf_fit_plane_ref runs on the same integers.  Nothing of the last scored batch is read or
// written: the stage timings are not touched; the block and the scratch are the ones every such call shares (call_io, call_scratch).
#include "engine_state.h"

namespace haf_host {

using namespace haf_plane_math;

namespace {

// the call's block, device and pinned: [counters: 16 bytes][ten moments][n_hyp counts][n_hyp x 4 hypothesis words] -- so far it comes
// back -- [n_hyp thresholds]; behind the largest such block, the packed bytes of a host mask
constexpr size_t kPlaneCounterBytes = 16, kPlaneMomentBytes = kPlaneMoments * sizeof(int64_t);
constexpr size_t kPlaneCountsAt = kPlaneCounterBytes + kPlaneMomentBytes;                      // 96
constexpr size_t plane_hyps_at(size_t n_hyp) { return up16(kPlaneCountsAt + n_hyp * 4); }
constexpr size_t plane_thr_at(size_t n_hyp) { return plane_hyps_at(n_hyp) + n_hyp * 16; }
constexpr size_t kPlaneMaskAt = up16(plane_thr_at(HAF_MAX_PLANE_HYP) + (size_t)HAF_MAX_PLANE_HYP * 4);

int fit_plane_impl(haf_engine *e, const haf_frame *frame, const haf_roi *mask, const haf_plane_params *p, haf_plane_result *out,
                   int32_t *counts, float *hyps)
{
    const std::string who = "haf_fit_plane: ";
    std::string why;
    int rc;
    if ((rc = check_plane(frame, mask, p, out, why)) != HAF_OK) return fail(e, rc, who + why);
    const haf_frame &f = *frame;
    const size_t px = (size_t)f.width * (size_t)f.height, K = (size_t)p->n_hyp;
    const haf_roi m = mask ? *mask : haf_roi{};            // (no haf_roi, or one without a mask: the whole frame)
    StageBuf *in = nullptr;
    if ((rc = frame_input_prepare(e, f, who, &in)) != HAF_OK) return rc;
    const size_t hyps_at = plane_hyps_at(K), thr_at = plane_thr_at(K), mp = (size_t)e->cfg.max_points, blocks = plane_blocks(mp);
    // the scratch: [x][y][z: max_points words each][a usable bit per pixel, 64-bit words][a count per block of 1024 pixels]
    CallBuffers cb;
    if ((rc = call_buffers(e, who, kPlaneMaskAt + mp, "the copy-back block", up16(mp * 12) + blocks * (kPlaneBlockPixels / 64) * 8 + blocks * 4,
                           "the points, the usable bits and the block counts", &cb)) != HAF_OK) return rc;
    const hipStream_t s = cb.stream;
    char *const dev = cb.dev, *const host = cb.host, *const scratch = cb.scratch;

    PlaneDev d;
    memset(&d, 0, sizeof d);
    if ((rc = frame_input_upload(e, f, *in, s, &d.f)) != HAF_OK) return rc;
    ImageDev md;
    if ((rc = upload_image(e, f, m.mask, m.on_device, m.row_stride_bytes, 1, cb, kPlaneMaskAt, &md)) != HAF_OK) return rc;
    d.height = f.height;
    d.mask = static_cast<const unsigned char *>(md.src); d.mask_stride = md.row_stride;
    d.r = plane_rules(*p);
    d.x = reinterpret_cast<float *>(scratch);
    d.y = d.x + mp;
    d.z = d.y + mp;
    d.bits = reinterpret_cast<unsigned long long *>(scratch + up16(mp * 12));
    d.prefix = reinterpret_cast<int *>(d.bits + blocks * (kPlaneBlockPixels / 64));
    d.counters = reinterpret_cast<unsigned *>(dev);
    d.moments = reinterpret_cast<unsigned long long *>(dev + kPlaneCounterBytes);
    d.counts = reinterpret_cast<int *>(dev + kPlaneCountsAt);
    d.hyps = reinterpret_cast<float *>(dev + hyps_at);
    d.thr = reinterpret_cast<float *>(dev + thr_at);
    HIPCHK(e, hipMemsetAsync(dev, 0, hyps_at, s));         // counters, moments, counts: the block carries some earlier call's bytes
    launch_plane(d, s);
    if ((rc = call_finish(e, cb, thr_at)) != HAF_OK) return rc;
    unsigned cnt[4];
    memcpy(cnt, host, sizeof cnt);
    const int32_t *h_counts = reinterpret_cast<const int32_t *>(host + kPlaneCountsAt);
    const float *h_hyps = reinterpret_cast<const float *>(host + hyps_at);
    memcpy(out->moments, host + kPlaneCounterBytes, kPlaneMomentBytes);
    out->stats[0] = (int64_t)px; out->stats[1] = (int64_t)cnt[0]; out->stats[2] = (int64_t)cnt[1];
    plane_finish(f, *p, h_counts, h_hyps, out);
    if (counts) memcpy(counts, h_counts, K * sizeof(int32_t));
    if (hyps) memcpy(hyps, h_hyps, K * 4 * sizeof(float));
    return HAF_OK;
}

}  // namespace

}  // namespace haf_host

extern "C" {

int haf_fit_plane(haf_engine *e, const haf_frame *frame, const haf_roi *mask, const haf_plane_params *p, haf_plane_result *out,
                  int32_t *counts, float *hyps)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return fit_plane_impl(e, frame, mask, p, out, counts, hyps); });
}

}  // extern "C"
