// roi_host.cpp -- haf_roi_cells and haf_roi_cells_views, the host definitions of record of the cell sets of haf_score_frames_roi and
// haf_score_views_roi (include/hafgrasp.h): the ROI cells S_r of one roll -- of one frame, or the union over a request's masked views --
// and their dilation by the vote's footprint.  No device, no engine: the pixel's point is haf_frame_points', the roll
// transform fill_roll_geo's (engine_geometry.cpp) and the cell arithmetic grasp_cells.h's -- the two headers the device kernel
// (roi.hip: k_roi_mark, on the points of frames.hip) is compiled from.  Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "engine_state.h"
#include "grasp_cells.h"

namespace haf_host {

// eval = the T-dilation of S: the 29 taps of the vote (server.cpp:873-878), |dr| <= 2 and |dc| <= 2, plus dr = 0 and |dc| = 3, 4 (symmetric)
static void dilate_cells(const std::vector<uint8_t> &S, int H, int W, uint8_t *eval)
{
    memset(eval, 0, (size_t)H * W);
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            if (!S[(size_t)i * W + j]) continue;
            for (int dr = -2; dr <= 2; dr++) {
                const int reach = dr == 0 ? 4 : 2, rr = i + dr;
                if (rr < 0 || rr >= H) continue;
                for (int dc = -reach; dc <= reach; dc++)
                    if (j + dc >= 0 && j + dc < W) eval[(size_t)rr * W + j + dc] = 1;
            }
        }
}

static int roi_cells_impl(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const haf_frame *f, const uint8_t *mask,
                          size_t mask_row_stride, uint8_t *roi, uint8_t *eval)
{
    if (!cfg || !in || !f || !mask) return HAF_E_ARG;
    if (cfg->grid_h < 1 || cfg->grid_w < 1 || cfg->n_rolls < 1 || (int64_t)cfg->grid_h * cfg->grid_w > (int64_t)INT32_MAX) return HAF_E_ARG;
    if (roll < 0 || roll >= cfg->n_rolls) return HAF_E_ARG;
    std::string err;
    const int rc = check_frame(*f, err);
    if (rc != HAF_OK) return rc;
    if (f->on_device != 0) return HAF_E_ARG;               // (host memory only: this function touches no device)
    if (mask_row_stride < (size_t)f->width) return HAF_E_ARG;
    const int H = cfg->grid_h, W = cfg->grid_w;
    const size_t HW = (size_t)H * W, n = (size_t)f->width * (size_t)f->height;
    std::vector<float> xyz(n * 3);
    const int rp = haf_frame_points(f, xyz.data());
    if (rp != HAF_OK) return rp;
    haf_cell_math::CellGeo g;
    fill_cell_geo(*cfg, *in, roll, 1, &g);
    float r_row, r_col;
    haf_pick_math::cell_reach(H, W, &r_row, &r_col);
    std::vector<uint8_t> S(HW, 0);
    for (size_t v = 0; v < (size_t)f->height; v++)
        for (size_t u = 0; u < (size_t)f->width; u++) {
            if (mask[v * mask_row_stride + u] == 0) continue;
            const float *p = xyz.data() + (v * (size_t)f->width + u) * 3;
            if (!haf_cell_math::point_usable(p)) continue;
            const int32_t c = haf_cell_math::point_cell(g.m, p[0], p[1], p[2], r_row, r_col, H, W);
            if (c >= 0) S[(size_t)c] = 1;
        }
    if (roi) memcpy(roi, S.data(), HW);
    if (eval) dilate_cells(S, H, W, eval);
    return HAF_OK;
}

// the OR of roi_cells_impl over the views that have a mask; every view is checked before anything is written
static int roi_cells_views_impl(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const haf_frame *frames, const haf_roi *rois,
                                int32_t n_views, uint8_t *roi, uint8_t *eval)
{
    if (!cfg || !in || !frames || !rois || n_views < 1 || n_views > HAF_MAX_VIEWS) return HAF_E_ARG;
    if (cfg->grid_h < 1 || cfg->grid_w < 1 || cfg->n_rolls < 1 || (int64_t)cfg->grid_h * cfg->grid_w > (int64_t)INT32_MAX) return HAF_E_ARG;
    if (roll < 0 || roll >= cfg->n_rolls) return HAF_E_ARG;
    for (int k = 0; k < n_views; k++) {
        std::string err;
        const int rc = check_frame(frames[k], err);
        if (rc != HAF_OK) return rc;
        if (frames[k].on_device != 0) return HAF_E_ARG;
        if (!rois[k].mask) continue;
        if (rois[k].on_device != 0 || rois[k].row_stride_bytes < (size_t)frames[k].width) return HAF_E_ARG;      // (host masks only)
    }
    const size_t HW = (size_t)cfg->grid_h * cfg->grid_w;
    std::vector<uint8_t> S(HW, 0), one(HW);
    for (int k = 0; k < n_views; k++) {
        if (!rois[k].mask) continue;
        const int rc = roi_cells_impl(cfg, in, roll, &frames[k], rois[k].mask, rois[k].row_stride_bytes, one.data(), nullptr);
        if (rc != HAF_OK) return rc;
        for (size_t i = 0; i < HW; i++) S[i] |= one[i];
    }
    if (roi) memcpy(roi, S.data(), HW);
    if (eval) dilate_cells(S, cfg->grid_h, cfg->grid_w, eval);
    return HAF_OK;
}

}  // namespace haf_host

extern "C" {

int haf_roi_cells_views(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const haf_frame *frames, const haf_roi *rois,
                        int32_t n_views, uint8_t *roi, uint8_t *eval)
{
    return guarded(nullptr, [&] { return roi_cells_views_impl(cfg, in, roll, frames, rois, n_views, roi, eval); });
}

// (no C++ exception may cross the C-ABI)
int haf_roi_cells(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const haf_frame *frame, const uint8_t *mask,
                  size_t mask_row_stride, uint8_t *roi, uint8_t *eval)
{
    return guarded(nullptr, [&] { return roi_cells_impl(cfg, in, roll, frame, mask, mask_row_stride, roi, eval); });
}

}  // extern "C"
