// graspmap_host.cpp -- the host definitions of record of the per-pixel grasp maps (include/hafgrasp.h): haf_point_cells,
// haf_grasp_map_ref and haf_label_best_ref.  None touches a device or an engine: the roll transform is fill_roll_geo's (engine_geometry.cpp), the cell
// arithmetic grasp_cells.h's and the pixel's point frame_points.h's, the sources the device kernel (graspmap.hip) is compiled from.
// Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "engine_state.h"
#include "grasp_cells.h"

namespace haf_host {

using haf_cell_math::CellGeo;

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
    float r_row, r_col;
    haf_pick_math::cell_reach(cfg->grid_h, cfg->grid_w, &r_row, &r_col);
    for (size_t i = 0; i < n; i++) {
        const float *p = xyz + i * stride_floats;
        cell[i] = haf_cell_math::point_cell(g.m, p[0], p[1], p[2], r_row, r_col, cfg->grid_h, cfg->grid_w);
    }
    return HAF_OK;
}

// haf_grasp_map_ref's per-pixel rule, written once: px(i, vote, roll, cell) for every pixel i = v * width + u of the host frame, in that order
template <class Px>
static int map_pixels(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                      const haf_frame *f, const Px &px)
{
    std::vector<CellGeo> geo((size_t)std::max(1, roll_count));
    fill_cell_geo(*cfg, *in, roll_first, roll_count, geo.data());
    const int H = cfg->grid_h, W = cfg->grid_w;
    const size_t HW = (size_t)H * W;
    float r_row, r_col;
    haf_pick_math::cell_reach(H, W, &r_row, &r_col);
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
            px((size_t)v * (size_t)f->width + u, (int16_t)best, (int16_t)best_roll, (int32_t)best_cell);
        }
    }
    return HAF_OK;
}

// what haf_grasp_map_ref and haf_label_best_ref refuse of their common arguments
static int check_map_ref_args(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                              const haf_frame *f)
{
    if (!check_grid(cfg) || !in || !f) return HAF_E_ARG;
    if (roll_first < 0 || roll_count < 0 || (int64_t)roll_first + roll_count > cfg->n_rolls || (roll_count > 0 && !eval_grids)) return HAF_E_ARG;
    std::string err;
    const int rc = check_frame(*f, err);
    if (rc != HAF_OK) return rc;
    if (f->on_device != 0) return HAF_E_ARG;               // (host memory only: this function touches no device)
    return HAF_OK;
}

static int grasp_map_ref_impl(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                              const haf_frame *f, int16_t *vote, int16_t *roll, int32_t *cell)
{
    const int rc = check_map_ref_args(cfg, in, roll_first, roll_count, eval_grids, f);
    if (rc != HAF_OK) return rc;
    return map_pixels(cfg, in, roll_first, roll_count, eval_grids, f, [&](size_t i, int16_t bv, int16_t br, int32_t bc) {
        if (vote) vote[i] = bv;
        if (roll) roll[i] = br;
        if (cell) cell[i] = bc;
    });
}

void label_pick_none(haf_label_pick *p)
{
    p->found = 0; p->u = p->v = p->roll = p->cell = -1; p->vote = HAF_MAP_NO_CELL; p->n_pixels = 0;
}

unsigned long long label_pick_key(const haf_label_pick &p, int32_t width)
{
    return haf_pick_math::pick_key(p.vote, p.roll, (unsigned)((size_t)p.v * (size_t)width + (size_t)p.u));
}

void label_order(const haf_label_pick *picks, int32_t n, const std::function<int32_t(int32_t)> &id_of, int32_t width, int32_t *order,
                 int32_t *n_found)
{
    std::vector<std::pair<unsigned long long, int32_t>> keys;
    for (int32_t k = 0; k < n; k++)
        if (picks[k].found) keys.emplace_back(label_pick_key(picks[k], width), id_of(k));
    std::sort(keys.begin(), keys.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    if (order)
        for (size_t k = 0; k < keys.size(); k++) order[k] = keys[k].second;
    if (n_found) *n_found = (int32_t)keys.size();
}

static int label_best_ref_impl(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                               const haf_frame *f, const haf_label_image *labels, int32_t n_labels, int32_t min_vote, haf_label_pick *picks,
                               int32_t *order, int32_t *n_found)
{
    int rc = check_map_ref_args(cfg, in, roll_first, roll_count, eval_grids, f);
    if (rc != HAF_OK) return rc;
    std::string err;
    if (!picks || check_label_image(labels, f->width, n_labels, err) != HAF_OK) return HAF_E_ARG;
    if (labels->on_device != 0) return HAF_E_ARG;           // (host memory only)
    for (int32_t l = 0; l < n_labels; l++) label_pick_none(&picks[l]);
    std::vector<unsigned long long> best((size_t)n_labels, 0ull);
    const size_t width = (size_t)f->width;
    rc = map_pixels(cfg, in, roll_first, roll_count, eval_grids, f, [&](size_t i, int16_t bv, int16_t br, int32_t bc) {
        const size_t v = i / width, u = i - v * width;
        const uint32_t lab = load_label(*labels, u, v);
        if (lab < 1u || lab > (unsigned)n_labels || !haf_pick_math::pick_qualifies(bv, br, min_vote)) return;
        haf_label_pick cand;
        cand.found = 1; cand.u = (int32_t)u; cand.v = (int32_t)v; cand.vote = bv; cand.roll = br; cand.cell = bc;
        haf_label_pick &p = picks[lab - 1];
        cand.n_pixels = p.n_pixels + 1;
        const unsigned long long key = label_pick_key(cand, f->width);
        if (key > best[lab - 1]) { best[lab - 1] = key; p = cand; }
        else p.n_pixels = cand.n_pixels;
    });
    if (rc != HAF_OK) return rc;
    label_order(picks, n_labels, [](int32_t l) { return l + 1; }, f->width, order, n_found);
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

int haf_label_best_ref(const haf_config *cfg, const haf_grasp_input *in, int32_t roll_first, int32_t roll_count, const float *eval_grids,
                       const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, int32_t min_vote, haf_label_pick *picks,
                       int32_t *order, int32_t *n_found)
{
    return guarded(nullptr, [&] {
        return label_best_ref_impl(cfg, in, roll_first, roll_count, eval_grids, frame, labels, n_labels, min_vote, picks, order, n_found);
    });
}

}  // extern "C"
