// depth_filter.h -- the per-pixel rules of haf_filter_depth (include/hafgrasp.h), written once: which sample of an exposure is valid,
// the lower median of a pixel's valid samples, the tolerance t_p and the support predicate.
//
// The same source is compiled for the device (depthfilter.hip: k_depth_filter) and for the host (depthfilter_host.cpp:
// haf_filter_depth_ref, the definition of record), as frame_points.h is -- whose validity rules and rounded fp32 operations these are:
// nothing of them is restated here.  Stage T performs no arithmetic on a sample: a sample travels as its KEY, its own bits as an unsigned
// word (a U16 sample's value, an F32 sample's word: valid F32 samples are positive and finite, so their words order as they do), and an
// invalid sample as all ones, which no valid sample is and which sorts last.
#pragma once
#include "frame_points.h"

namespace haf_depth_filter_math {

using namespace haf_frame_math;

constexpr int kMaxStack = 8;                       // HAF_MAX_STACK
constexpr uint32_t kInvalidKey = 0xFFFFFFFFu;

// z of a key as frame_points.h forms it: ONE rounded multiplication; the invalid key gives the invalid pattern (a NaN)
HAF_FRAME_HD float key_z_u16(uint32_t key, const FrameMath &m) { return key == kInvalidKey ? f_from_bits(kInvalidWord) : f_mul((float)(uint16_t)key, m.depth_scale); }
HAF_FRAME_HD float key_z_f32(uint32_t key, const FrameMath &m) { return key == kInvalidKey ? f_from_bits(kInvalidWord) : f_mul(f_from_bits(key), m.depth_scale); }

// the key of one sample: point_u16's / point_f32's `ok`
HAF_FRAME_HD uint32_t sample_key_u16(uint16_t d, const FrameMath &m)
{
    const float z = f_mul((float)d, m.depth_scale);
    return (d != 0 && depth_in_range(z, m)) ? (uint32_t)d : kInvalidKey;
}
HAF_FRAME_HD uint32_t sample_key_f32(uint32_t w, const FrameMath &m)
{
    const float d = f_from_bits(w), z = f_mul(d, m.depth_scale);
    return (f_finite(d) && d > 0.0f && depth_in_range(z, m)) ? w : kInvalidKey;
}

HAF_FRAME_HD void key_order(uint32_t &a, uint32_t &b)
{
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}

// Stage T of one pixel.  k[0..8): the keys of its samples, kInvalidKey from the stack's size on.  -> the lower median of the valid ones
// (rank (c - 1) / 2 of c in ascending order), or kInvalidKey when c < min_valid.  A fixed network of 19 compare-exchanges sorts the
// eight (the invalid keys end up last) and the rank, 0..3, picks by compare-select: every index below is a constant, so on the device
// the eight keys stay in registers.
HAF_FRAME_HD uint32_t lower_median(uint32_t (&k)[kMaxStack], int min_valid)
{
    int c = 0;
    for (int j = 0; j < kMaxStack; j++) c += k[j] != kInvalidKey;
    key_order(k[0], k[2]); key_order(k[1], k[3]); key_order(k[4], k[6]); key_order(k[5], k[7]);
    key_order(k[0], k[4]); key_order(k[1], k[5]); key_order(k[2], k[6]); key_order(k[3], k[7]);
    key_order(k[0], k[1]); key_order(k[2], k[3]); key_order(k[4], k[5]); key_order(k[6], k[7]);
    key_order(k[2], k[4]); key_order(k[3], k[5]);
    key_order(k[1], k[4]); key_order(k[3], k[6]);
    key_order(k[1], k[2]); key_order(k[3], k[4]); key_order(k[5], k[6]);
    const int rank = (c - 1) / 2;
    uint32_t m = k[0];
    m = rank == 1 ? k[1] : m;
    m = rank == 2 ? k[2] : m;
    m = rank == 3 ? k[3] : m;
    return (c >= min_valid && c > 0) ? m : kInvalidKey;
}

// Stage S: t_p of a pixel with depth z_p, and whether a neighbour at z_q supports it.  fabs clears the sign bit; a NaN z_q (an invalid
// neighbour, or one outside the image) fails the comparison by itself
HAF_FRAME_HD float support_tolerance(float tol_abs, float tol_rel, float z_p) { return f_add(tol_abs, f_mul(tol_rel, z_p)); }
HAF_FRAME_HD bool supports(float z_q, float z_p, float t_p) { return f_from_bits(f_bits(f_sub(z_q, z_p)) & 0x7FFFFFFFu) <= t_p; }

}  // namespace haf_depth_filter_math
