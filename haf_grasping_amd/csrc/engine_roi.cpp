// engine_roi.cpp -- haf_score_frames_roi (include/hafgrasp.h): haf_score_frames under an image-space mask per request.  The cloud, the
// binning and the integral images are the whole frame's; what the mask restricts is the evaluation list.  This unit holds the call's
// checks (all of them before any device work), the ROI buffers, the upload of host masks and the launch of k_roi_mark (roi.hip); the
// request path itself is engine_request.cpp's, which takes three turns for a RoiCall:
//   * run_prestages: no fused k_small_pre; behind the integral image the ROI cell sets are marked and k_mask_count_roi writes
//     m = cell_in_box && any(S at c + T) -- k_scan, k_compact and every decision tier then run unchanged on the shorter list;
//   * vote_and_wait: the gated vote (v = 0 outside S);
//   * the adaptive choice of the screening form neither reads nor changes anything (roi_screen_overflow).
#include "engine_state.h"

namespace haf_host {

namespace {

size_t up16(size_t x) { return (x + 15) / 16 * 16; }

// the ROI cell sets and the masks' area, on the first call (the precedent: the raw area of host XYZ views, score_views_impl)
int ensure_roi_buffers(haf_engine *e)
{
    if (e->d_roi_cells.p) return HAF_OK;
    const haf_config &c = e->cfg;
    HIPCHK(e, hipSetDevice(c.device));
    const size_t words = (size_t)c.max_clouds * (size_t)e->max_rolls * (size_t)c.grid_h * (size_t)roi_row_words(c.grid_w);
    const size_t mask_bytes = (size_t)c.max_points + (size_t)c.max_clouds * 16;
    HIPCHK(e, e->d_roi_mask.alloc(mask_bytes));
    if (hipHostMalloc((void **)&e->h_roi_mask, mask_bytes) != hipSuccess) {
        e->d_roi_mask.release();
        e->h_roi_mask = nullptr;
        return fail(e, HAF_E_DEVICE, "haf_score_frames_roi: no pinned memory for the masks");
    }
    const hipError_t rc = e->d_roi_cells.alloc(words);
    if (rc != hipSuccess) {
        e->d_roi_mask.release();
        (void)hipHostFree(e->h_roi_mask);
        e->h_roi_mask = nullptr;
        HIPCHK(e, rc);
    }
    return HAF_OK;
}

}  // namespace

int roi_upload_masks(haf_engine *e, const RoiCall &roi, const haf_frame *frames, int B, hipStream_t s)
{
    for (int b = 0; b < B; b++) {
        if (roi.rois[b].on_device == 1) continue;
        const size_t n = (size_t)frames[b].width * (size_t)frames[b].height, at = roi.off[(size_t)b];
        HIPCHK(e, hipMemcpyAsync(e->d_roi_mask.p + at, e->h_roi_mask + at, n, hipMemcpyHostToDevice, s));
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
        launch_roi_mark(dev ? r.mask : e->d_roi_mask.p + roi.off[(size_t)b], dev ? r.row_stride_bytes : (size_t)frames[b].width, frames[b].width,
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
    int64_t total = 0;
    std::vector<haf_cloud> clouds((size_t)n);
    for (int b = 0; b < n; b++) {
        const std::string req = who + "request " + std::to_string(b) + ": ";
        std::string msg;
        const int rc = check_frame(frames[b], msg);
        if (rc != HAF_OK) return fail(e, rc, req + msg);
        const size_t px = (size_t)frames[b].width * (size_t)frames[b].height;
        total += (int64_t)px;
        if (total > e->cfg.max_points) return fail(e, HAF_E_CAPACITY, req + "more pixels than max_points");
        if (!rois[b].mask) return fail(e, HAF_E_ARG, req + "null mask");
        if (rois[b].on_device != 0 && rois[b].on_device != 1) return fail(e, HAF_E_ARG, req + "haf_roi: on_device must be 0 (host) or 1 (device-resident)");
        if (rois[b].row_stride_bytes < (size_t)frames[b].width) return fail(e, HAF_E_ARG, req + "haf_roi: row_stride_bytes smaller than a row");
        // (xyz is never read on this path, as in score_frames_impl)
        clouds[(size_t)b] = haf_cloud{static_cast<const float *>(frames[b].data), px, 3, 0};
    }
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
        const size_t w = (size_t)frames[b].width;
        call.off[(size_t)b] = at;
        long cnt = 0;
        for (int v = 0; v < frames[b].height; v++) {
            const uint8_t *src = rois[b].mask + (size_t)v * rois[b].row_stride_bytes;
            unsigned char *dst = e->h_roi_mask + at + (size_t)v * w;
            memcpy(dst, src, w);
            for (size_t u = 0; u < w; u++) cnt += src[u] != 0;
        }
        call.masked[(size_t)b] = cnt;
        at += up16(w * (size_t)frames[b].height);
    }
    return score_batch_impl(e, n, clouds.data(), in, out, frames, nullptr, &call);
}

}  // namespace haf_host
