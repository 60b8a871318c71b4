// plane_rules.h -- the per-point and per-hypothesis rules of haf_fit_plane (include/hafgrasp.h), written once: which point is usable,
// which rank a hypothesis' corner draws, the hypothesis three points span, which point is its inlier, and a coordinate's fixed-point word.
//
// The same source is compiled for the device (plane.hip) and for the host (plane_host.cpp: haf_fit_plane_ref, the definition of record),
// as segment_rules.h is, on top of frame_points.h -- whose points and rounded fp32 operations these are.  Everything else of the
// definition (ranks, counts, the winner, the ten moments) is integer work on these rules; the plane itself is ONE host function on those
// integers (plane_host.cpp: plane_from_moments), which both entry points call.
#pragma once
#include "frame_points.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#endif

namespace haf_plane_math {

using namespace haf_frame_math;

constexpr uint32_t kPlaneRangeWord = 0x41800000u;         // 16.0f: a usable coordinate's magnitude is at most this
constexpr float kPlaneQuantum = 4096.0f;                  // fixed-point words of the refit: units of 1/4096 m
constexpr int kPlaneMoments = 10;                         // N, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz

// what the rules read of haf_plane_params: tol2, cos2 and uu are formed ONCE per call on the host (plane_rules of plane_host.cpp)
struct PlaneRules {
    float tol2, min_area2;
    float up[3];
    float cos2, uu;
    int use_up;                                           // up is not all zero
    int n_hyp;
    uint32_t seed;
};

// a hypothesis: the un-normalised normal and offset (the four words of `hyps`), and thr = tol2 * nn, a NaN for a void hypothesis -- no
// r * r is <= a NaN, so a void hypothesis counts nothing by itself
struct PlaneHyp { float n[3], d, thr; };

// finite and |w| <= 16: one integer comparison on the magnitude bits (an infinity or a NaN lies above every finite pattern)
HAF_FRAME_HD bool coord_usable(float w) { return (f_bits(w) & 0x7FFFFFFFu) <= kPlaneRangeWord; }
HAF_FRAME_HD bool point_usable(const float *p) { return coord_usable(p[0]) && coord_usable(p[1]) && coord_usable(p[2]); }

HAF_FRAME_HD uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// the rank corner j of hypothesis k draws among n_usable >= 1 usable pixels (seed + 3k + j wraps in 32 bits)
HAF_FRAME_HD uint32_t sample_rank(uint32_t seed, uint32_t k, uint32_t j, uint32_t n_usable)
{
    return (uint32_t)(((uint64_t)mix32(seed + 3u * k + j) * (uint64_t)n_usable) >> 32);
}

HAF_FRAME_HD float f_neg(float x) { return f_from_bits(f_bits(x) ^ 0x80000000u); }
HAF_FRAME_HD float f_canon(float x) { return f_nan(x) ? f_from_bits(kInvalidWord) : x; }
HAF_FRAME_HD float dot3(const float *a, float x, float y, float z) { return f_add(f_add(f_mul(a[0], x), f_mul(a[1], y)), f_mul(a[2], z)); }

// the hypothesis through p0, p1, p2 (three words each): n = (p1 - p0) x (p2 - p0), d = -((n0 x0 + n1 y0) + n2 z0),
// nn = (n0 n0 + n1 n1) + n2 n2.  same_rank: two of the three ranks coincide.  Returns whether it is void
HAF_FRAME_HD bool make_hypothesis(const float *p0, const float *p1, const float *p2, bool same_rank, const PlaneRules &r, PlaneHyp &h)
{
    const float a[3] = {f_sub(p1[0], p0[0]), f_sub(p1[1], p0[1]), f_sub(p1[2], p0[2])};
    const float b[3] = {f_sub(p2[0], p0[0]), f_sub(p2[1], p0[1]), f_sub(p2[2], p0[2])};
    const float n[3] = {f_sub(f_mul(a[1], b[2]), f_mul(a[2], b[1])), f_sub(f_mul(a[2], b[0]), f_mul(a[0], b[2])),
                        f_sub(f_mul(a[0], b[1]), f_mul(a[1], b[0]))};
    const float d = f_neg(dot3(n, p0[0], p0[1], p0[2]));
    const float nn = dot3(n, n[0], n[1], n[2]);
    bool is_void = same_rank || !f_finite(nn) || nn <= r.min_area2;
    if (r.use_up) {
        const float c = dot3(n, r.up[0], r.up[1], r.up[2]);
        if (!(f_mul(c, c) >= f_mul(r.cos2, f_mul(nn, r.uu)))) is_void = true;
    }
    h.n[0] = f_canon(n[0]); h.n[1] = f_canon(n[1]); h.n[2] = f_canon(n[2]); h.d = f_canon(d);
    h.thr = is_void ? f_from_bits(kInvalidWord) : f_canon(f_mul(r.tol2, nn));
    return is_void;
}

// r = ((n0 x + n1 y) + n2 z) + d; an inlier when r r <= thr.  An unusable point reaches this test as three NaNs and fails it
HAF_FRAME_HD bool inlier(const PlaneHyp &h, float x, float y, float z)
{
    const float r = f_add(dot3(h.n, x, y, z), h.d);
    return f_mul(r, r) <= h.thr;
}

// THE rounding of the refit: q = round-to-nearest-even(w * 4096) as int32.  |w| <= 16, so the product is exact and |q| <= 2^16
#if defined(__HIP_DEVICE_COMPILE__)
HAF_FRAME_HD int32_t coord_word(float w) { return __float2int_rn(f_mul(w, kPlaneQuantum)); }
#else
HAF_FRAME_HD int32_t coord_word(float w) { return (int32_t)lrintf(f_mul(w, kPlaneQuantum)); }      // (the default rounding mode: to nearest even)
#endif

// the ten moments of one inlier added to m
HAF_FRAME_HD void add_moments(long long *m, float x, float y, float z)
{
    const long long qx = coord_word(x), qy = coord_word(y), qz = coord_word(z);
    m[0] += 1; m[1] += qx; m[2] += qy; m[3] += qz;
    m[4] += qx * qx; m[5] += qx * qy; m[6] += qx * qz; m[7] += qy * qy; m[8] += qy * qz; m[9] += qz * qz;
}

}  // namespace haf_plane_math
