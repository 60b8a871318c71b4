// engine_roi.cpp -- haf_score_frames_roi and haf_score_views_roi (include/hafgrasp.h): haf_score_frames / haf_score_views under
// image-space masks.  The cloud, the binning and the integral images are the whole scene's; what the masks restrict is the evaluation
// list.  This unit holds the calls' checks (all of them before any device work), the ROI buffers, the packing and upload of host masks
// and the launches of k_roi_mark (a frame per request: the points k_frame_points wrote, by pixel index) and k_roi_mark_view (views: the
// masked pixels deprojected again, the compacted points have no pixel index); the request path itself is engine_request.cpp's, which takes
// three turns for a RoiCall, with or without views:
//   * run_prestages: no fused k_small_pre; behind the integral image the ROI cell sets are marked and k_mask_count_roi writes
//     m = cell_in_box && any(S at c + T) -- k_scan, k_compact and every decision tier then run unchanged on the shorter list;
//   * vote_and_wait: the gated vote (v = 0 outside S);
//   * the adaptive choice of the screening form neither reads nor changes anything (roi_screen_overflow).
#include "engine_state.h"

namespace haf_host {

// the ROI cell sets and the masks' area, on the first call (the precedent: the raw area of host XYZ views, score_views_impl)
int ensure_roi_buffers(haf_engine *e, const std::string &who)
{
    if (e->d_roi_cells.p) return HAF_OK;
    const haf_config &c = e->cfg;
    HIPCHK(e, hipSetDevice(c.device));
    const size_t words = (size_t)c.max_clouds * (size_t)e->max_rolls * (size_t)c.grid_h * (size_t)roi_row_words(c.grid_w);
    const size_t mask_bytes = (size_t)c.max_points + (size_t)c.max_clouds * HAF_MAX_VIEWS * 16;      // (every view's mask at a multiple of 16 bytes)
    int rc = ensure_stage(e, e->roi_mask, mask_bytes, who, "the masks");
    if (rc == HAF_OK && (rc = ensure_dev(e, e->d_roi_cells, words, who, "the ROI buffers")) != HAF_OK) e->roi_mask.release();      // all or nothing: the next call tries again
    return rc;
}

// host masks of the call's views: their rows without the padding into the pinned area, counted on the way (classify_request).
// first[b]: the flat index of request b's first view, first[n] the number of views
static RoiCall stage_masks(haf_engine *e, const haf_frame *frames, const haf_roi *rois, int n, const std::vector<int> &first)
{
    RoiCall call;
    call.rois = rois;
    call.masked.assign((size_t)n, 0);
    call.off.assign((size_t)first[(size_t)n], 0);
    size_t at = 0;
    for (int b = 0; b < n; b++)
        for (int k = first[(size_t)b]; k < first[(size_t)b + 1]; k++) {
            if (!rois[k].mask) continue;
            if (rois[k].on_device == 1) { call.masked[(size_t)b] = -1; continue; }
            const size_t w = (size_t)frames[k].width, px = w * (size_t)frames[k].height;
            call.off[(size_t)k] = at;
            char *const dst = e->roi_mask.host + at;
            pack_rows(dst, reinterpret_cast<const char *>(rois[k].mask), (size_t)frames[k].height, w, 1, 1, rois[k].row_stride_bytes);
            long cnt = 0;
            for (size_t i = 0; i < px; i++) cnt += dst[i] != 0;
            if (call.masked[(size_t)b] >= 0) call.masked[(size_t)b] += cnt;
            at += up16(px);
        }
    return call;
}

int roi_upload_masks(haf_engine *e, const RoiCall &roi, const haf_frame *frames, int n_views, hipStream_t s)
{
    for (int k = 0; k < n_views; k++) {
        if (!RoiCall::staged(roi.rois[k])) continue;
        const size_t n = (size_t)frames[k].width * (size_t)frames[k].height, at = roi.off[(size_t)k];
        HIPCHK(e, hipMemcpyAsync(e->roi_mask.dev.p + at, e->roi_mask.host + at, n, hipMemcpyHostToDevice, s));
    }
    return HAF_OK;
}

void roi_describe_views(const haf_engine *e, const RoiCall &roi, const haf_frame *frames, const int32_t *views, int B, int R, int H, int W,
                        const RollGeo *d_geo, RoiViewDev *out)
{
    const size_t grid_words = (size_t)H * (size_t)roi_row_words(W);
    for (int b = 0, k = 0; b < B; b++)
        for (int v = 0; v < views[b]; v++, k++) {
            const haf_roi &r = roi.rois[k];
            const ImageDev m = describe_image(r.mask, r.on_device, r.row_stride_bytes, (size_t)frames[k].width, 1, e->roi_mask.dev.p + roi.off[(size_t)k]);
            out[k].mask = static_cast<const unsigned char *>(m.src); out[k].stride = m.row_stride;
            out[k].S = e->d_roi_cells.p + (size_t)b * R * grid_words;
            out[k].geo = d_geo + (size_t)b * R;
        }
}

int roi_mark_cells(haf_engine *e, const RoiCall &roi, const haf_frame *frames, const CloudDev *h_clouds, const RollGeo *d_geo, const Dims &d,
                   float r_row, float r_col, hipStream_t s, const RoiViews *views)
{
    const size_t grid_words = (size_t)d.H * (size_t)roi_row_words(d.W);
    HIPCHK(e, hipMemsetAsync(e->d_roi_cells.p, 0, (size_t)d.B * d.R * grid_words * sizeof(unsigned long long), s));
    if (views) {
        launch_roi_mark_views(views->d_frames, views->h_frames, views->d_roi, views->h_roi, views->n_views, d.R, d.H, d.W, r_row, r_col, s);
        HIPCHK(e, hipGetLastError());
        return HAF_OK;
    }
    for (int b = 0; b < d.B; b++) {
        const haf_roi &r = roi.rois[b];
        const ImageDev m = describe_image(r.mask, r.on_device, r.row_stride_bytes, (size_t)frames[b].width, 1, e->roi_mask.dev.p + roi.off[(size_t)b]);
        launch_roi_mark(static_cast<const unsigned char *>(m.src), (size_t)m.row_stride, frames[b].width,
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
    if (e->mdl.prob_mode) return fail(e, HAF_E_ARG, who + "not available with HAF_FLAG_PROBABILITY");
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
    int rc = ensure_roi_buffers(e, who);
    if (rc != HAF_OK) return rc;
    std::vector<int> first((size_t)n + 1);
    for (int b = 0; b <= n; b++) first[(size_t)b] = b;
    const RoiCall call = stage_masks(e, frames, rois, n, first);
    const FrameSource from{frames, nullptr, &call};
    return score_batch_impl(e, n, chk.clouds.data(), in, out, &from);
}

// haf_score_views with a mask per view: every refusal before any device work -- haf_score_views' own, then the call's; view after view,
// a view's frame before its mask, so the masks of the views in front of a refused frame come first -- then the batch path with the views
// of request b as the source of cloud b's points and their masks as the restriction of its evaluation list
int score_views_roi_impl(haf_engine *e, int32_t n, const int32_t *views_per_request, const haf_frame *frames, const haf_roi *rois,
                         const haf_grasp_input *in, haf_grasp_output *out, int64_t *n_points)
{
    if (!e) return HAF_E_ARG;
    const std::string who = "haf_score_views_roi: ";
    if (!views_per_request || !frames || !rois || !in || !out || n < 1) return fail(e, HAF_E_ARG, who + "null or empty argument");
    if (e->mdl.prob_mode) return fail(e, HAF_E_ARG, who + "not available with HAF_FLAG_PROBABILITY");
    if (n > e->cfg.max_clouds) return fail(e, HAF_E_CAPACITY, who + "more requests than max_clouds");
    if (e->cfg.n_rolls > e->max_rolls) return fail(e, HAF_E_CAPACITY, who + "more rolls in one call than max_rolls_per_call");
    std::vector<int> first((size_t)n + 1, 0);
    for (int b = 0; b < n; b++) {
        if (views_per_request[b] < 1 || views_per_request[b] > HAF_MAX_VIEWS)
            return fail(e, HAF_E_ARG, who + "request " + std::to_string(b) + ": view count outside [1, HAF_MAX_VIEWS]");
        first[(size_t)b + 1] = first[(size_t)b] + views_per_request[b];
    }
    const FrameBatch chk = check_frame_batch(frames, n, views_per_request, e->cfg.max_points);
    const auto at = [&](int b, int v) { return who + "request " + std::to_string(b) + " view " + std::to_string(v) + ": "; };
    const int checked = chk.code != HAF_OK ? first[(size_t)chk.request] + chk.view : first[(size_t)n];
    for (int b = 0; b < n; b++)
        for (int v = 0, k = first[(size_t)b]; v < views_per_request[b] && k < checked; v++, k++) {
            if (!rois[k].mask) continue;                  // (a camera without a segmenter: on_device and the stride are ignored)
            if (rois[k].on_device != 0 && rois[k].on_device != 1) return fail(e, HAF_E_ARG, at(b, v) + "haf_roi: on_device must be 0 (host) or 1 (device-resident)");
            if (rois[k].row_stride_bytes < (size_t)frames[k].width) return fail(e, HAF_E_ARG, at(b, v) + "haf_roi: row_stride_bytes smaller than a row");
        }
    if (chk.code != HAF_OK) return fail(e, chk.code, at(chk.request, chk.view) + (chk.text.empty() ? "more pixels than max_points" : chk.text));
    int rc = HAF_OK;
    if (chk.host_xyz && (rc = ensure_raw_xyz(e, who)) != HAF_OK) return rc;
    if ((rc = ensure_roi_buffers(e, who)) != HAF_OK) return rc;
    const RoiCall call = stage_masks(e, frames, rois, n, first);
    const FrameSource from{frames, views_per_request, &call};
    if ((rc = score_batch_impl(e, n, chk.clouds.data(), in, out, &from)) != HAF_OK) return rc;
    // (a batch whose every budget is negative runs nothing, on the device either: no count exists)
    for (int b = 0; n_points && b < n; b++) n_points[b] = (size_t)b < e->last.clouds.size() ? (int64_t)e->last.clouds[(size_t)b].n : -1;
    return HAF_OK;
}

}  // namespace haf_host
