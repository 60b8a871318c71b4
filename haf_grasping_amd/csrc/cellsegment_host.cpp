// cellsegment_host.cpp -- the host side of haf_segment_cells that needs neither a device nor an engine: haf_cell_segment_default, the
// checks of the frame, the parameters and the label image (both entry points apply them), and haf_segment_cells_ref, the definition of
// record of cell_segment_rules.h's rules and of the integer rules behind them (counts, components, anchors, numbering); the device
// kernels of cellsegment.hip are tested against it word for word.  Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "frame_stage.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using namespace haf_cell_math;

int check_cell_segment(const haf_frame *frame, const haf_cell_segment_params *p, const void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                       int32_t out_on_device, const int32_t *n_labels, std::string &err)
{
    if (!frame || !p || !n_labels) { err = "null frame, parameters or n_labels"; return HAF_E_ARG; }
    int rc = check_frame(*frame, err);
    if (rc != HAF_OK) return rc;
    if ((rc = check_label_output(*frame, labels, elem_bytes, row_stride_bytes, out_on_device, err)) != HAF_OK) return rc;
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(p->plane[i])) { err = "haf_cell_segment_params: plane has an entry that is not finite"; return HAF_E_ARG; }
    if (!std::isfinite(p->min_height) || !std::isfinite(p->max_height)) { err = "haf_cell_segment_params: min_height and max_height must be finite"; return HAF_E_ARG; }
    if (p->min_points < 1) { err = "haf_cell_segment_params: min_points < 1"; return HAF_E_ARG; }
    if (p->max_labels < 1 || p->max_labels > (elem_bytes == 1 ? 255 : HAF_MAX_LABELS)) {
        err = "haf_cell_segment_params: max_labels outside 1..HAF_MAX_LABELS (1..255 for a uint8 image)";
        return HAF_E_ARG;
    }
    if (!std::isfinite(p->cell) || p->cell < 0.001f || p->cell > 1.0f) { err = "haf_cell_segment_params: cell outside 0.001 .. 1"; return HAF_E_ARG; }
    if (!(std::fabs(p->x0) <= 64.0f) || !(std::fabs(p->y0) <= 64.0f)) { err = "haf_cell_segment_params: x0 or y0 not finite or beyond 64 m"; return HAF_E_ARG; }
    if (p->nx < 1 || p->nx > 4096 || p->ny < 1 || p->ny > 4096) { err = "haf_cell_segment_params: nx or ny outside 1 .. 4096"; return HAF_E_ARG; }
    if ((int64_t)p->nx * p->ny > (int64_t)HAF_MAX_CELLS) { err = "haf_cell_segment_params: nx * ny > HAF_MAX_CELLS"; return HAF_E_ARG; }
    if (p->connectivity != 4 && p->connectivity != 8) { err = "haf_cell_segment_params: connectivity must be 4 or 8"; return HAF_E_ARG; }
    if (!std::isfinite(p->max_step)) { err = "haf_cell_segment_params: max_step must be finite"; return HAF_E_ARG; }
    return HAF_OK;
}

CellRules cell_rules(const haf_cell_segment_params &p)
{
    CellRules r;
    memcpy(r.band.plane, p.plane, sizeof r.band.plane);
    r.band.min_height = p.min_height; r.band.max_height = p.max_height; r.band.gap2 = 0.0f;
    r.x0 = p.x0; r.y0 = p.y0;
    r.inv_cell = 1.0f / p.cell;
    r.max_step = p.max_step;
    r.nx = p.nx; r.ny = p.ny; r.connectivity = p.connectivity;
    return r;
}

namespace {

// the root of a: parents only point at lower indices, so the walk ends; the path is shortened behind it
int32_t find_root(std::vector<int32_t> &parent, int32_t a)
{
    int32_t r = a;
    while (parent[(size_t)r] != r) r = parent[(size_t)r];
    while (parent[(size_t)a] != r) { const int32_t next = parent[(size_t)a]; parent[(size_t)a] = r; a = next; }
    return r;
}

void unite(std::vector<int32_t> &parent, int32_t a, int32_t b)
{
    a = find_root(parent, a); b = find_root(parent, b);
    if (a == b) return;
    if (a < b) parent[(size_t)b] = a; else parent[(size_t)a] = b;      // towards the lower index: a root is its component's anchor
}

int segment_cells_ref_impl(const haf_frame *frame, const haf_cell_segment_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                           uint16_t *cell_labels, haf_cell_segment_info *info, int32_t *n_labels, int64_t *stats)
{
    std::string err;
    int rc = check_cell_segment(frame, p, labels, elem_bytes, row_stride_bytes, 0, n_labels, err);
    if (rc != HAF_OK) return rc;
    if (frame->on_device != 0) return HAF_E_ARG;           // (host memory only: this function touches no device)
    const size_t W = (size_t)frame->width, H = (size_t)frame->height, n = W * H;
    std::vector<float> xyz(n * 3);
    if ((rc = haf_frame_points(frame, xyz.data())) != HAF_OK) return rc;
    const CellRules r = cell_rules(*p);
    const size_t nx = (size_t)r.nx, ny = (size_t)r.ny, nc = nx * ny;
    std::vector<int32_t> cell(n), count(nc, 0), parent(nc);
    std::vector<uint32_t> top(nc, 0u);
    int64_t fg = 0, outside = 0, occupied = 0;
    for (size_t i = 0; i < n; i++) {
        const float *q = &xyz[3 * i];
        cell[i] = -1;
        if (!cell_foreground(q, r)) continue;
        fg++;
        const int c = cell_of(q, r);
        if (c < 0) { outside++; continue; }
        cell[i] = c;
        count[(size_t)c]++;
        const uint32_t t = shape_enc(cell_height_key(q, r));
        if (t > top[(size_t)c]) top[(size_t)c] = t;
    }
    for (size_t c = 0; c < nc; c++) {
        parent[c] = count[c] > 0 ? (int32_t)c : -1;
        occupied += count[c] > 0;
    }
    const auto link = [&](size_t a, size_t b) {
        if (parent[b] >= 0 && cells_linked(top[a], top[b], r.max_step)) unite(parent, (int32_t)a, (int32_t)b);
    };
    const bool corners = r.connectivity == 8;
    for (size_t iy = 0; iy < ny; iy++)
        for (size_t ix = 0; ix < nx; ix++) {
            const size_t c = iy * nx + ix;
            if (parent[c] < 0) continue;
            if (ix + 1 < nx) link(c, c + 1);
            if (iy + 1 >= ny) continue;
            link(c, c + nx);
            if (corners && ix + 1 < nx) link(c, c + nx + 1);
            if (corners && ix > 0) link(c, c + nx - 1);
        }
    // point counts at the roots; then the roots in ascending order are the anchors in ascending order
    std::vector<int32_t> size(nc, 0), number(nc, 0);
    for (size_t c = 0; c < nc; c++)
        if (parent[c] >= 0) size[(size_t)find_root(parent, (int32_t)c)] += count[c];
    int64_t comps = 0, kept = 0;
    std::vector<uint32_t> label_top;
    for (size_t c = 0; c < nc; c++) {
        if (parent[c] != (int32_t)c) continue;
        comps++;
        if (size[c] < p->min_points) continue;
        kept++;
        if (kept > (int64_t)p->max_labels) continue;
        number[c] = (int32_t)kept;
        label_top.push_back(0u);
        if (info) {
            haf_cell_segment_info &s = info[kept - 1];
            s.n_points = size[c]; s.n_cells = 0;
            s.anchor_ix = s.ix_min = s.ix_max = (int32_t)(c % nx);
            s.anchor_iy = s.iy_min = s.iy_max = (int32_t)(c / nx);
            s.top = 0.0f;
        }
    }
    for (size_t iy = 0; iy < ny; iy++)
        for (size_t ix = 0; ix < nx; ix++) {
            const size_t c = iy * nx + ix;
            const int32_t l = parent[c] >= 0 ? number[(size_t)parent[c]] : 0;      // (every path was shortened to its root above)
            if (cell_labels) cell_labels[c] = (uint16_t)l;
            if (l == 0) continue;
            if (top[c] > label_top[(size_t)l - 1]) label_top[(size_t)l - 1] = top[c];
            if (!info) continue;
            haf_cell_segment_info &s = info[l - 1];
            s.n_cells++;
            if ((int32_t)ix < s.ix_min) s.ix_min = (int32_t)ix;
            if ((int32_t)ix > s.ix_max) s.ix_max = (int32_t)ix;
            if ((int32_t)iy < s.iy_min) s.iy_min = (int32_t)iy;
            if ((int32_t)iy > s.iy_max) s.iy_max = (int32_t)iy;
        }
    if (info)
        for (size_t l = 0; l < label_top.size(); l++) info[l].top = key_height(shape_dec(label_top[l]));
    for (size_t v = 0; v < H; v++)
        for (size_t u = 0; u < W; u++) {
            const int32_t c = cell[v * W + u];
            const int32_t l = c >= 0 ? number[(size_t)parent[(size_t)c]] : 0;
            store_label(labels, row_stride_bytes, elem_bytes, u, v, (uint32_t)l);
        }
    *n_labels = (int32_t)(kept < (int64_t)p->max_labels ? kept : (int64_t)p->max_labels);
    if (stats) { stats[0] = (int64_t)n; stats[1] = fg; stats[2] = outside; stats[3] = occupied; stats[4] = comps; stats[5] = kept; }
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_cell_segment_default(haf_cell_segment_params *p)
{
    if (!p) return;
    p->plane[0] = 0.0f; p->plane[1] = 0.0f; p->plane[2] = 1.0f; p->plane[3] = 0.0f;
    p->min_height = 0.01f; p->max_height = 0.0f; p->cell = 0.01f; p->x0 = -5.12f; p->y0 = -5.12f; p->nx = 1024; p->ny = 1024;
    p->connectivity = 8; p->max_step = 0.0f; p->min_points = 50; p->max_labels = 255;
}

// (no C++ exception may cross the C-ABI: a grid too large for the host comes back as a status)
int haf_segment_cells_ref(const haf_frame *frame, const haf_cell_segment_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                          uint16_t *cell_labels, haf_cell_segment_info *info, int32_t *n_labels, int64_t *stats)
{
    try {
        return haf::segment_cells_ref_impl(frame, p, labels, elem_bytes, row_stride_bytes, cell_labels, info, n_labels, stats);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
