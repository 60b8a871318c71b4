// segment_host.cpp -- the host side of haf_segment_frame that needs neither a device nor an engine: haf_segment_default, the checks of
// the frame, the parameters and the label image (both entry points apply them), and haf_segment_ref, the definition of record of
// segment_rules.h's predicates and of the integer rules behind them (components, anchors, numbering); the device kernels of
// segment.hip are tested against it word for word.  Built with -ffp-contract=off like every unit (build.py: FLAGS).
#include "frame_stage.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using namespace haf_segment_math;

// every refusal of the parameters; elem_bytes: the label image's, which bounds max_labels
static int check_segment_params(const haf_segment_params &p, int32_t elem_bytes, std::string &err)
{
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(p.plane[i])) { err = "haf_segment_params: plane has an entry that is not finite"; return HAF_E_ARG; }
    if (!std::isfinite(p.min_height) || !std::isfinite(p.max_height)) { err = "haf_segment_params: min_height and max_height must be finite"; return HAF_E_ARG; }
    if (!std::isfinite(p.max_gap) || !(p.max_gap > 0.0f)) { err = "haf_segment_params: max_gap must be finite and positive"; return HAF_E_ARG; }
    if (p.min_pixels < 1) { err = "haf_segment_params: min_pixels < 1"; return HAF_E_ARG; }
    if (p.max_labels < 1 || p.max_labels > (elem_bytes == 1 ? 255 : HAF_MAX_LABELS)) {
        err = "haf_segment_params: max_labels outside 1..HAF_MAX_LABELS (1..255 for a uint8 image)";
        return HAF_E_ARG;
    }
    return HAF_OK;
}

int check_segment(const haf_frame *frame, const haf_segment_params *p, const void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                  int32_t out_on_device, const int32_t *n_labels, std::string &err)
{
    if (!frame || !p || !n_labels) { err = "null frame, parameters or n_labels"; return HAF_E_ARG; }
    int rc = check_frame(*frame, err);
    if (rc != HAF_OK) return rc;
    if ((rc = check_segment_params(*p, elem_bytes, err)) != HAF_OK) return rc;
    return check_label_output(*frame, labels, elem_bytes, row_stride_bytes, out_on_device, err);
}

SegmentRules segment_rules(const haf_segment_params &p)
{
    SegmentRules r;
    memcpy(r.plane, p.plane, sizeof r.plane);
    r.min_height = p.min_height; r.max_height = p.max_height;
    r.gap2 = f_mul(p.max_gap, p.max_gap);
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

int segment_ref_impl(const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                     haf_segment_info *info, int32_t *n_labels, int64_t *stats)
{
    std::string err;
    int rc = check_segment(frame, p, labels, elem_bytes, row_stride_bytes, 0, n_labels, err);
    if (rc != HAF_OK) return rc;
    if (frame->on_device != 0) return HAF_E_ARG;           // (host memory only: this function touches no device)
    const size_t W = (size_t)frame->width, H = (size_t)frame->height, n = W * H;
    std::vector<float> xyz(n * 3);
    if ((rc = haf_frame_points(frame, xyz.data())) != HAF_OK) return rc;
    const SegmentRules r = segment_rules(*p);
    std::vector<int32_t> parent(n);
    int64_t fg = 0;
    for (size_t i = 0; i < n; i++) {
        const bool f = foreground(&xyz[3 * i], r);
        parent[i] = f ? (int32_t)i : -1;
        fg += f;
    }
    for (size_t v = 0; v < H; v++)
        for (size_t u = 0; u < W; u++) {
            const size_t i = v * W + u;
            if (parent[i] < 0) continue;
            if (u + 1 < W && parent[i + 1] >= 0 && linked(&xyz[3 * i], &xyz[3 * (i + 1)], r.gap2)) unite(parent, (int32_t)i, (int32_t)(i + 1));
            if (v + 1 < H && parent[i + W] >= 0 && linked(&xyz[3 * i], &xyz[3 * (i + W)], r.gap2)) unite(parent, (int32_t)i, (int32_t)(i + W));
        }
    // sizes at the roots; then the roots in ascending order are the anchors in ascending order
    std::vector<int32_t> size(n, 0), number(n, 0);
    for (size_t i = 0; i < n; i++)
        if (parent[i] >= 0) size[(size_t)find_root(parent, (int32_t)i)]++;
    int64_t comps = 0, kept = 0;
    for (size_t i = 0; i < n; i++) {
        if (parent[i] != (int32_t)i) continue;
        comps++;
        if (size[i] < p->min_pixels) continue;
        kept++;
        if (kept > (int64_t)p->max_labels) continue;
        number[i] = (int32_t)kept;
        if (info) {
            haf_segment_info &s = info[kept - 1];
            s.n_pixels = size[i];
            s.anchor_u = s.u_min = s.u_max = (int32_t)(i % W);
            s.anchor_v = s.v_min = s.v_max = (int32_t)(i / W);
        }
    }
    for (size_t v = 0; v < H; v++)
        for (size_t u = 0; u < W; u++) {
            const size_t i = v * W + u;
            const int32_t l = parent[i] >= 0 ? number[(size_t)parent[i]] : 0;      // (every path was shortened to its root above)
            store_label(labels, row_stride_bytes, elem_bytes, u, v, (uint32_t)l);
            if (l > 0 && info) {
                haf_segment_info &s = info[l - 1];
                if ((int32_t)u < s.u_min) s.u_min = (int32_t)u;
                if ((int32_t)u > s.u_max) s.u_max = (int32_t)u;
                if ((int32_t)v < s.v_min) s.v_min = (int32_t)v;
                if ((int32_t)v > s.v_max) s.v_max = (int32_t)v;
            }
        }
    *n_labels = (int32_t)(kept < (int64_t)p->max_labels ? kept : (int64_t)p->max_labels);
    if (stats) { stats[0] = (int64_t)n; stats[1] = fg; stats[2] = comps; stats[3] = kept; }
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

void haf_segment_default(haf_segment_params *p)
{
    if (!p) return;
    p->plane[0] = 0.0f; p->plane[1] = 0.0f; p->plane[2] = 1.0f; p->plane[3] = 0.0f;
    p->min_height = 0.01f; p->max_height = 0.0f; p->max_gap = 0.02f; p->min_pixels = 50; p->max_labels = 255;
}

// (no C++ exception may cross the C-ABI: an image too large for the host comes back as a status)
int haf_segment_ref(const haf_frame *frame, const haf_segment_params *p, void *labels, int32_t elem_bytes, size_t row_stride_bytes,
                    haf_segment_info *info, int32_t *n_labels, int64_t *stats)
{
    try {
        return haf::segment_ref_impl(frame, p, labels, elem_bytes, row_stride_bytes, info, n_labels, stats);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

}  // extern "C"
