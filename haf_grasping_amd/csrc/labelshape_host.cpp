// labelshape_host.cpp -- the host side of haf_measure_labels that needs neither a device nor an engine: the checks of the frame, the
// label image, the plane and the output (both entry points apply them), shape_finish -- THE derived fields of a shape from its
// integers, which both entry points call -- haf_measure_labels_ref, the definition of record of label_shape.h's rules (the device
// kernel of labelshape.hip is tested against it word for word), and haf_object_input.  Built with -ffp-contract=off like every unit
// (build.py: FLAGS).
#include "frame_stage.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace haf {

using namespace haf_shape_math;

namespace {
constexpr double kShapeQuantum = 4096.0;
constexpr double kShapeStepRad = 3.14159265358979323846 / 12.0;      // 15 degrees
constexpr int kMaxMarginCells = 64, kBorderCells = 7, kMinLength = 16;
}  // namespace

int check_measure(const haf_frame *frame, const haf_label_image *l, int32_t n_labels, const float *plane, const haf_label_shape *shapes,
                  std::string &err)
{
    if (!frame) { err = "null frame"; return HAF_E_ARG; }
    int rc = check_frame(*frame, err);
    if (rc != HAF_OK) return rc;
    if (!shapes) { err = "null shapes"; return HAF_E_ARG; }
    if ((rc = check_label_image(l, frame->width, n_labels, err)) != HAF_OK) return rc;
    if (plane)
        for (int i = 0; i < 4; i++)
            if (!std::isfinite(plane[i])) { err = "a plane entry is not finite"; return HAF_E_ARG; }
    return HAF_OK;
}

void shape_finish(haf_label_shape *s)
{
    const int32_t nn[kShapeDirs] = HAF_SHAPE_NN;
    s->found = s->n_points > 0 ? 1 : 0;
    s->narrow_dir = 0;
    s->reserved = 0;
    for (int j = 0; j < 3; j++) s->centroid[j] = s->box_min[j] = s->box_max[j] = 0.0f;
    for (int k = 0; k < kShapeDirs; k++) s->width[k] = 0.0f;
    s->narrow_width = s->long_width = s->yaw = s->diameter = s->height = 0.0f;
    if (!s->found) return;
    for (int j = 0; j < 3; j++) {
        s->centroid[j] = (float)((double)s->sum[j] / (kShapeQuantum * (double)s->n_points));
        s->box_min[j] = (float)((double)s->q_min[j] / kShapeQuantum);
        s->box_max[j] = (float)((double)s->q_max[j] / kShapeQuantum);
    }
    int best = 0;
    int64_t d_best = 0;
    float widest = 0.0f;
    for (int k = 0; k < kShapeDirs; k++) {
        const int64_t d = (int64_t)s->t_max[k] - (int64_t)s->t_min[k];      // 0 <= d < 2^31
        s->width[k] = (float)((double)d / (kShapeQuantum * std::sqrt((double)nn[k])));
        widest = s->width[k] > widest ? s->width[k] : widest;
        // d^2 / nn[k] < d_best^2 / nn[best]  <=>  d^2 nn[best] < d_best^2 nn[k]: below 2^89, exact in 128 bits
        if (k == 0 || (__int128)d * d * nn[best] < (__int128)d_best * d_best * nn[k]) { best = k; d_best = d; }
    }
    s->narrow_dir = best;
    s->narrow_width = s->width[best];
    s->long_width = s->width[(best + kShapeDirs / 2) % kShapeDirs];
    s->yaw = (float)((double)best * kShapeStepRad);
    s->diameter = widest;
    s->height = s->h_max;
}

namespace {

template <class SUM> void shape_from_acc(const ShapeAcc<SUM> &a, haf_label_shape *s)
{
    memset(s, 0, sizeof *s);
    s->n_pixels = a.n_pixels; s->n_points = a.n_points;
    for (int j = 0; j < 3; j++) { s->sum[j] = (int64_t)a.sum[j]; s->q_min[j] = a.q_min[j]; s->q_max[j] = a.q_max[j]; }
    for (int k = 0; k < kShapeDirs; k++) { s->t_min[k] = a.t_min[k]; s->t_max[k] = a.t_max[k]; }
    s->h_max = a.h_key == kShapeNone ? f_from_bits(kInvalidWord) : key_height(a.h_key);
    shape_finish(s);
}

}  // namespace

void shape_from_row(const uint32_t *row, haf_label_shape *s)
{
    ShapeAcc<int64_t> a;
    a.n_pixels = (int32_t)row[kShapeRowPixels]; a.n_points = (int32_t)row[kShapeRowPoints];
    memcpy(a.sum, row + kShapeRowSum, sizeof a.sum);
    for (int j = 0; j < 3; j++) { a.q_min[j] = ~shape_dec(row[kShapeRowQMin + j]); a.q_max[j] = shape_dec(row[kShapeRowQMax + j]); }
    for (int k = 0; k < kShapeDirs; k++) { a.t_min[k] = ~shape_dec(row[kShapeRowTMin + k]); a.t_max[k] = shape_dec(row[kShapeRowTMax + k]); }
    a.h_key = shape_dec(row[kShapeRowHKey]);
    shape_from_acc(a, s);
}

namespace {

int measure_labels_ref_impl(const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, const float *plane, haf_label_shape *shapes)
{
    std::string err;
    int rc = check_measure(frame, labels, n_labels, plane, shapes, err);
    if (rc != HAF_OK) return rc;
    if (frame->on_device != 0 || labels->on_device != 0) return HAF_E_ARG;      // (host memory only: this function touches no device)
    const size_t W = (size_t)frame->width, H = (size_t)frame->height;
    std::vector<float> xyz(W * H * 3);
    if ((rc = haf_frame_points(frame, xyz.data())) != HAF_OK) return rc;
    std::vector<ShapeAcc<int64_t>> acc((size_t)n_labels);
    for (auto &a : acc) shape_clear(a);
    for (size_t v = 0; v < H; v++)
        for (size_t u = 0; u < W; u++) {
            const uint32_t lab = load_label(*labels, u, v);
            if (lab < 1u || lab > (unsigned)n_labels) continue;
            shape_add_pixel(acc[lab - 1], &xyz[3 * (v * W + u)], plane, plane != nullptr);
        }
    for (int32_t l = 0; l < n_labels; l++) shape_from_acc(acc[(size_t)l], &shapes[l]);
    return HAF_OK;
}

int object_input_impl(const haf_config *cfg, const haf_grasp_input *base, const haf_label_shape *shape, int32_t margin_cells,
                      haf_grasp_input *out, int32_t *fits)
{
    if (!cfg || !base || !shape || !out || !fits) return HAF_E_ARG;
    if (!shape->found || margin_cells < 0 || margin_cells > kMaxMarginCells) return HAF_E_ARG;
    const int32_t side = cfg->grid_h < cfg->grid_w ? cfg->grid_h : cfg->grid_w;
    const int64_t upper = (int64_t)(side - (side & 1));      // the even part of the smaller grid side
    int64_t len = 2 * ((int64_t)std::ceil(50.0 * (double)shape->diameter) + margin_cells + kBorderCells);
    if (len < kMinLength) len = kMinLength;
    const bool clipped = len > upper;
    if (clipped) len = upper;
    haf_grasp_input o = *base;
    o.grasp_area_center[0] = ((double)shape->q_min[0] + (double)shape->q_max[0]) / (2.0 * kShapeQuantum);
    o.grasp_area_center[1] = ((double)shape->q_min[1] + (double)shape->q_max[1]) / (2.0 * kShapeQuantum);
    o.grasp_area_length_x = o.grasp_area_length_y = (float)len;
    *out = o;
    *fits = clipped ? 0 : 1;
    return HAF_OK;
}

}  // namespace

}  // namespace haf

extern "C" {

// (no C++ exception may cross the C-ABI: an image too large for the host comes back as a status)
int haf_measure_labels_ref(const haf_frame *frame, const haf_label_image *labels, int32_t n_labels, const float *plane, haf_label_shape *shapes)
{
    try {
        return haf::measure_labels_ref_impl(frame, labels, n_labels, plane, shapes);
    } catch (...) {
    }
    return HAF_E_INTERNAL;
}

int haf_object_input(const haf_config *cfg, const haf_grasp_input *base, const haf_label_shape *shape, int32_t margin_cells,
                     haf_grasp_input *out, int32_t *fits)
{
    return haf::object_input_impl(cfg, base, shape, margin_cells, out, fits);
}

}  // extern "C"
