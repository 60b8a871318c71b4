// label_shape.h -- the per-point rules of haf_measure_labels (include/hafgrasp.h), written once: a direction of the fan, a point's
// height and its ordered key, what one usable point adds to its label's accumulators, and the words those accumulators travel in.
//
// The same source is compiled for the device (labelshape.hip) and for the host (labelshape_host.cpp: haf_measure_labels_ref, the
// definition of record), as plane_rules.h is -- whose point_usable and coord_word these rules reuse and do not restate.  Everything here
// is integer work but the height, which is segment_rules.h's: rounded fp32 operations in a fixed order.  The derived fields of a
// haf_label_shape are ONE host function on the integers (labelshape_host.cpp: shape_finish), which both entry points call.
#pragma once
#include "../../include/hafgrasp.h"
#include "plane_rules.h"

namespace haf_shape_math {

using namespace haf_plane_math;

constexpr int kShapeDirs = HAF_SHAPE_DIRS;
constexpr int32_t kShapeNone = INT32_MIN;                 // the height key of a label without a height (no non-NaN h maps to it)

// (C, S)[k]: the table of the header, as a local constant so that an unrolled loop folds it into literals
HAF_FRAME_HD int32_t shape_cos(int k) { const int32_t c[kShapeDirs] = HAF_SHAPE_COS; return c[k]; }
HAF_FRAME_HD int32_t shape_sin(int k) { const int32_t s[kShapeDirs] = HAF_SHAPE_SIN; return s[k]; }

// h = ((plane[0] x + plane[1] y) + plane[2] z) + plane[3], left to right: foreground()'s height of segment_rules.h
HAF_FRAME_HD float shape_height(const float *plane, const float *p)
{
    return f_add(f_add(f_add(f_mul(plane[0], p[0]), f_mul(plane[1], p[1])), f_mul(plane[2], p[2])), plane[3]);
}
// the ordered key the binning kernels use for heights (device_common.h: f2key), for host and device: a < b as floats <=> key(a) < key(b)
// as int32, with -0 below +0; and its inverse
HAF_FRAME_HD int32_t height_key(float h) { const int32_t b = (int32_t)f_bits(h); return b >= 0 ? b : (b ^ 0x7FFFFFFF); }
HAF_FRAME_HD float key_height(int32_t k) { return f_from_bits((uint32_t)(k >= 0 ? k : (k ^ 0x7FFFFFFF))); }

// the accumulators of one label over some of its pixels.  SUM: int64 on the host; int32 inside a wave, which sums at most 512 words of
// magnitude <= 2^16
template <class SUM> struct ShapeAcc {
    int32_t n_pixels, n_points;
    SUM sum[3];
    int32_t q_min[3], q_max[3];
    int32_t t_min[kShapeDirs], t_max[kShapeDirs];
    int32_t h_key;
};

template <class SUM> HAF_FRAME_HD void shape_clear(ShapeAcc<SUM> &a)
{
    a.n_pixels = a.n_points = 0;
    for (int j = 0; j < 3; j++) { a.sum[j] = 0; a.q_min[j] = INT32_MAX; a.q_max[j] = INT32_MIN; }
    for (int k = 0; k < kShapeDirs; k++) { a.t_min[k] = INT32_MAX; a.t_max[k] = INT32_MIN; }
    a.h_key = kShapeNone;
}

// one pixel that carries the label: p = its point's three words; plane: four finite words, read only when use_plane
template <class SUM> HAF_FRAME_HD void shape_add_pixel(ShapeAcc<SUM> &a, const float *p, const float *plane, bool use_plane)
{
    a.n_pixels += 1;
    if (!point_usable(p)) return;
    a.n_points += 1;
    int32_t q[3];
    for (int j = 0; j < 3; j++) {
        q[j] = coord_word(p[j]);
        a.sum[j] += (SUM)q[j];
        a.q_min[j] = q[j] < a.q_min[j] ? q[j] : a.q_min[j];
        a.q_max[j] = q[j] > a.q_max[j] ? q[j] : a.q_max[j];
    }
    for (int k = 0; k < kShapeDirs; k++) {
        const int32_t t = shape_cos(k) * q[0] + shape_sin(k) * q[1];
        a.t_min[k] = t < a.t_min[k] ? t : a.t_min[k];
        a.t_max[k] = t > a.t_max[k] ? t : a.t_max[k];
    }
    if (use_plane) {
        const float h = shape_height(plane, p);
        if (!f_nan(h)) { const int32_t key = height_key(h); a.h_key = key > a.h_key ? key : a.h_key; }
    }
}

// A label's row of the device table: kShapeRowWords 32-bit words, zeroed before the launch, so every extent travels as a word whose
// ZERO is the empty value and whose unsigned maximum is the wanted one: a maximum x as shape_enc(x) (INT32_MIN <-> 0), a minimum x as
// shape_enc(~x) (INT32_MAX <-> 0; ~ reverses the order).  The three sums are 64-bit words at kShapeRowSum (8-byte aligned: a row is 160 bytes)
constexpr int kShapeRowPixels = 0, kShapeRowPoints = 1, kShapeRowSum = 2, kShapeRowQMin = 8, kShapeRowQMax = 11, kShapeRowTMin = 14,
              kShapeRowTMax = kShapeRowTMin + kShapeDirs, kShapeRowHKey = kShapeRowTMax + kShapeDirs, kShapeRowWords = 40;
static_assert(kShapeRowHKey < kShapeRowWords && kShapeRowWords % 4 == 0, "a row is whole 16-byte pieces");
HAF_FRAME_HD uint32_t shape_enc(int32_t x) { return (uint32_t)x ^ 0x80000000u; }
HAF_FRAME_HD int32_t shape_dec(uint32_t w) { return (int32_t)(w ^ 0x80000000u); }

}  // namespace haf_shape_math
