// engine_roi.cpp -- haf_score_frames_roi (include/hafgrasp.h): haf_score_frames under an image-space mask per request.  The cloud, the
// binning and the integral images are the whole frame's; what the mask restricts is the evaluation list.  This unit holds the call's
// checks (all of them before any device work), the ROI buffers, the packing and upload of host masks and the launch of k_roi_mark; the
// request path itself is engine_request.cpp's, which takes three turns for a RoiCall:
//   * run_prestages: no fused k_small_pre; behind the integral image the ROI cell sets are marked and k_mask_count_roi writes
//     m = cell_in_box && any(S at c + T) -- k_scan, k_compact and every decision tier then run unchanged on the shorter list;
//   * vote_and_wait: the gated vote (v = 0 outside S);
//   * the adaptive choice of the screening form neither reads nor changes anything (roi_screen_overflow).
#include "engine_state.h"

namespace haf_host {

namespace {

// the ROI cell sets and the masks' area, on the first call (the precedent: the raw area of host XYZ views, score_views_impl)
int ensure_roi_buffers(haf_engine *e)
{
    if (e->d_roi_cells.p) return HAF_OK;
    const haf_config &c = e->cfg;
    HIPCHK(e, hipSetDevice(c.device));
    const size_t words = (size_t)c.max_clouds * (size_t)e->max_rolls * (size_t)c.grid_h * (size_t)roi_row_words(c.grid_w);
    const size_t mask_bytes = (size_t)c.max_points + (size_t)c.max_clouds * 16;
    hipError_t rc = e->roi_mask.ensure(mask_bytes);
    if (e->roi_mask.pinned_failed) return fail(e, HAF_E_DEVICE, "haf_score_frames_roi: no pinned memory for the masks");
    if (rc == hipSuccess && (rc = e->d_roi_cells.alloc(words)) != hipSuccess) e->roi_mask.release();      // all or nothing: the next call tries again
    if (rc != hipSuccess) return fail(e, HAF_E_DEVICE, std::string("haf_score_frames_roi: no device memory for the ROI buffers: ") + hipGetErrorString(rc));
    return HAF_OK;
}

}  // namespace

int roi_upload_masks(haf_engine *e, const RoiCall &roi, const haf_frame *frames, int B, hipStream_t s)
{
    for (int b = 0; b < B; b++) {
        if (roi.rois[b].on_device == 1) continue;
        const size_t n = (size_t)frames[b].width * (size_t)frames[b].height, at = roi.off[(size_t)b];
        HIPCHK(e, hipMemcpyAsync(e->roi_mask.dev.p + at, e->roi_mask.host + at, n, hipMemcpyHostToDevice, s));
    }
    return HAF_OK;
}

int roi_mark_cells(haf_engine *e, const RoiCall &roi, const haf_frame *frames, const CloudDev *h_clouds, const RollGeo *d_geo, const Dims &d,
                   float r_row, float r_col, hipStream_t s)
{
    const size_t grid_words = (size_t)d.H * (size_t)roi_row_words(d.W);
    HIPCHK(e, hipMemsetAsync(e->d_roi_cells.p, 0, (size_t)d.B * d.R * grid_words * sizeof(unsigned long long), s));
    for (int b = 0; b < d.B; b++) {
        const haf_roi &r = roi.rois[b];
        const bool dev = r.on_device == 1;
        const unsigned char *staged = reinterpret_cast<const unsigned char *>(e->roi_mask.dev.p) + roi.off[(size_t)b];
        launch_roi_mark(dev ? r.mask : staged, dev ? r.row_stride_bytes : (size_t)frames[b].width, frames[b].width,
                        frames[b].width * frames[b].height, h_clouds[b].xyz, d_geo + (size_t)b * d.R, d.R,
                        e->d_roi_cells.p + (size_t)b * d.R * grid_words, d.H, d.W, r_row, r_col, s);
    }
    HIPCHK(e, hipGetLastError());
    return HAF_OK;
}

// every refusal before any device work (haf_score_frames' own among them), then the batch path with frame b as the source of cloud b's
// points and rois[b] as the restriction of its evaluation list
int score_frames_roi_impl(haf_engine *e, int32_t n, const haf_frame *frames, const haf_roi *rois, const haf_grasp_input *in, haf_grasp_output *out)
{
    if (!e) return HAF_E_ARG;
    const std::string who = "haf_score_frames_roi: ";
    if (!frames || !rois || !in || !out || n < 1) return fail(e, HAF_E_ARG, who + "null or empty argument");
    if (e->prob_mode) return fail(e, HAF_E_ARG, who + "not available with HAF_FLAG_PROBABILITY");
    if (n > e->cfg.max_clouds) return fail(e, HAF_E_CAPACITY, who + "more frames than max_clouds");
    if (e->cfg.n_rolls > e->max_rolls) return fail(e, HAF_E_CAPACITY, who + "more rolls in one call than max_rolls_per_call");
    // request after request, its frame's refusals before its mask's: the masks of the requests in front of a refused frame come first
    const FrameBatch chk = check_frame_batch(frames, n, nullptr, e->cfg.max_points);
    const auto req = [&](int b) { return who + "request " + std::to_string(b) + ": "; };
    for (int b = 0; b < (chk.code != HAF_OK ? chk.request : n); b++) {
        if (!rois[b].mask) return fail(e, HAF_E_ARG, req(b) + "null mask");
        if (rois[b].on_device != 0 && rois[b].on_device != 1) return fail(e, HAF_E_ARG, req(b) + "haf_roi: on_device must be 0 (host) or 1 (device-resident)");
        if (rois[b].row_stride_bytes < (size_t)frames[b].width) return fail(e, HAF_E_ARG, req(b) + "haf_roi: row_stride_bytes smaller than a row");
    }
    if (chk.code != HAF_OK) return fail(e, chk.code, req(chk.request) + (chk.text.empty() ? "more pixels than max_points" : chk.text));
    int rc = ensure_roi_buffers(e);
    if (rc != HAF_OK) return rc;
    // host masks: their rows without the padding into the pinned area, counted on the way (classify_request)
    RoiCall call;
    call.rois = rois;
    call.masked.assign((size_t)n, -1);
    call.off.assign((size_t)n, 0);
    size_t at = 0;
    for (int b = 0; b < n; b++) {
        if (rois[b].on_device == 1) continue;
        const size_t w = (size_t)frames[b].width, px = w * (size_t)frames[b].height;
        call.off[(size_t)b] = at;
        char *const dst = e->roi_mask.host + at;
        pack_rows(dst, reinterpret_cast<const char *>(rois[b].mask), (size_t)frames[b].height, w, 1, 1, rois[b].row_stride_bytes);
        long cnt = 0;
        for (size_t i = 0; i < px; i++) cnt += dst[i] != 0;
        call.masked[(size_t)b] = cnt;
        at += up16(px);
    }
    const FrameSource from{frames, nullptr, &call};
    return score_batch_impl(e, n, chk.clouds.data(), in, out, &from);
}

}  // namespace haf_host
