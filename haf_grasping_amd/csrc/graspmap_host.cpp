// graspmap_host.cpp -- the host definitions of record of the per-pixel grasp maps (include/hafgrasp.h): haf_point_cells and
// haf_grasp_map_ref.  Neither touches a device or an engine: the roll transform is fill_roll_geo's (engine_geometry.cpp), the cell
// arithmetic grasp_cells.h's and the pixel's point frame_points.h's, the sources the device kernel (graspmap.hip) is compiled from.
// Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "engine_state.h"
#include "grasp_cells.h"

namespace haf_host {

using haf_cell_math::CellGeo;

static float half_extent(int cells) { return (float)((0.5 * (float)cells) / 100.0); }      // server.cpp:410-411 (engine_request.cpp: r_row)

void fill_cell_geo(const haf_config &cfg, const haf_grasp_input &in, int roll_first, int roll_count, CellGeo *geo)
{
    const NormalisedInput n = normalise(in);
    for (int r = 0; r < roll_count; r++) {
        RollGeo g;
        fill_roll_geo(cfg, in, n, roll_first + r, g);
        memcpy(geo[r].m, g.m, sizeof g.m);
        memset(geo[r].pad, 0, sizeof geo[r].pad);
    }
}

static int check_grid(const haf_config *cfg)
{
    return cfg && cfg->grid_h >= 1 && cfg->grid_w >= 1 && cfg->n_rolls >= 1 && (int64_t)cfg->grid_h * cfg->grid_w <= (int64_t)INT32_MAX;
}

static int point_cells_impl(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const float *xyz, size_t n, size_t stride_floats,
                            int32_t *cell)
{
    if (!check_grid(cfg) || !in || !cell || (n && !xyz)) return HAF_E_ARG;
    if (roll < 0 || roll >= cfg->n_rolls || stride_floats < 3) return HAF_E_ARG;
    if (n > (size_t)INT32_MAX) return HAF_E_CAPACITY;
    CellGeo g;
    fill_cell_geo(*cfg, *in, roll, 1, &g);
    const float r_row = half_extent(cfg->grid_h), r_col = half_extent(cfg->grid_w);
    for (size_t i = 0; i < n; i++) {
        const float *p = xyz + i * stride_floats;
        cell[i] = haf_cell_math::point_cell(g.m, p[0], p[1], p[2], r_row, r_col, cfg->grid_h, cfg->grid_w);
    }
    return HAF_OK;
}

static int grasp_map_ref_impl(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                              const haf_frame *f, int16_t *vote, int16_t *roll, int32_t *cell)
{
    if (!check_grid(cfg) || !in || !f) return HAF_E_ARG;
    if (roll_first < 0 || roll_count < 0 || (int64_t)roll_first + roll_count > cfg->n_rolls || (roll_count > 0 && !eval_grids)) return HAF_E_ARG;
    std::string err;
    const int rc = check_frame(*f, err);
    if (rc != HAF_OK) return rc;
    if (f->on_device != 0) return HAF_E_ARG;               // (host memory only: this function touches no device)
    std::vector<CellGeo> geo((size_t)std::max(1, roll_count));
    fill_cell_geo(*cfg, *in, roll_first, roll_count, geo.data());
    const int H = cfg->grid_h, W = cfg->grid_w;
    const size_t HW = (size_t)H * W;
    const float r_row = half_extent(H), r_col = half_extent(W);
    const haf_frame_math::FrameMath m = frame_math(*f);
    const char *base = static_cast<const char *>(f->data);
    for (uint32_t v = 0; v < (uint32_t)f->height; v++) {
        const char *row = base + (size_t)v * f->row_stride_bytes;
        for (uint32_t u = 0; u < (uint32_t)f->width; u++) {
            float p[3];
            if (f->kind == HAF_FRAME_DEPTH_U16) {
                uint16_t d;
                memcpy(&d, row + (size_t)u * 2, 2);
                haf_frame_math::point_u16(m, u, v, d, p);
            } else if (f->kind == HAF_FRAME_DEPTH_F32) {
                float d;
                memcpy(&d, row + (size_t)u * 4, 4);
                haf_frame_math::point_f32(m, u, v, d, p);
            } else {
                float s[3];
                memcpy(s, row + (size_t)u * f->point_stride_bytes, 12);
                haf_frame_math::point_xyz(m, s[0], s[1], s[2], p);
            }
            int best = haf_cell_math::kNoCellVote, best_roll = -1, best_cell = -1;
            if (haf_cell_math::point_usable(p)) {
                for (int r = 0; r < roll_count; r++) {
                    const int32_t ci = haf_cell_math::point_cell(geo[(size_t)r].m, p[0], p[1], p[2], r_row, r_col, H, W);
                    if (ci < 0) continue;
                    const int val = (int)eval_grids[(size_t)r * HW + (size_t)ci];
                    if (best_roll < 0 || val > best) { best = val; best_roll = roll_first + r; best_cell = ci; }
                }
            }
            const size_t i = (size_t)v * (size_t)f->width + u;
            if (vote) vote[i] = (int16_t)best;
            if (roll) roll[i] = (int16_t)best_roll;
            if (cell) cell[i] = best_cell;
        }
    }
    return HAF_OK;
}

}  // namespace haf_host

extern "C" {

// (no C++ exception may cross the C-ABI)
int haf_point_cells(const haf_config *cfg, const haf_grasp_input *in, int32_t roll, const float *xyz, size_t n, size_t stride_floats,
                    int32_t *cell)
{
    return guarded(nullptr, [&] { return point_cells_impl(cfg, in, roll, xyz, n, stride_floats, cell); });
}

int haf_grasp_map_ref(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                      const haf_frame *frame, int16_t *vote, int16_t *roll, int32_t *cell)
{
    return guarded(nullptr, [&] { return grasp_map_ref_impl(cfg, in, roll_first, roll_count, eval_grids, frame, vote, roll, cell); });
}

}  // extern "C"
