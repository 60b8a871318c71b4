// frame_points.h -- a sensor frame's pixels as base-frame points: THE arithmetic of haf_frame (include/hafgrasp.h), written once.
//
// The same source is compiled for the device (frames.hip: k_frame_points) and for the host (frames_host.cpp: haf_frame_points, the
// definition of record), as decq.h is.  Every operation below is ONE correctly rounded fp32 operation in the order the header states,
// never a fused multiply-add: the device spells them as __f*_rn intrinsics, the host build relies on -ffp-contract=off (build.py: FLAGS;
// on clang the pragma below says so once more).  The two builds therefore agree in every bit of every finite result.  A NaN result --
// an invalid pixel, or inf - inf in the transform of an absurd pose -- is written as the one pattern 0x7FC00000: which NaN an operation
// returns is the one thing x86 and gfx950 do not agree on.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HAF_FRAME_HD __host__ __device__ __forceinline__
#else
#define HAF_FRAME_HD inline
#endif

namespace haf_frame_math {

constexpr uint32_t kInvalidWord = 0x7FC00000u;

// what a pixel's arithmetic reads of its frame: 1/fx and 1/fy are formed ONCE per frame on the host (frame_math below)
struct FrameMath {
    float ifx, ify, cx, cy;
    float depth_scale, min_depth, max_depth;
    float t[12];
};

#if defined(__HIP_DEVICE_COMPILE__)
HAF_FRAME_HD float f_mul(float a, float b) { return __fmul_rn(a, b); }
HAF_FRAME_HD float f_add(float a, float b) { return __fadd_rn(a, b); }
HAF_FRAME_HD float f_sub(float a, float b) { return __fsub_rn(a, b); }
HAF_FRAME_HD uint32_t f_bits(float x) { return __float_as_uint(x); }
HAF_FRAME_HD float f_from_bits(uint32_t w) { return __uint_as_float(w); }
#else
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
HAF_FRAME_HD float f_mul(float a, float b) { return a * b; }
HAF_FRAME_HD float f_add(float a, float b) { return a + b; }
HAF_FRAME_HD float f_sub(float a, float b) { return a - b; }
HAF_FRAME_HD uint32_t f_bits(float x) { uint32_t w; memcpy(&w, &x, 4); return w; }
HAF_FRAME_HD float f_from_bits(uint32_t w) { float x; memcpy(&x, &w, 4); return x; }
#endif

HAF_FRAME_HD bool f_finite(float x) { return (f_bits(x) & 0x7F800000u) != 0x7F800000u; }
HAF_FRAME_HD bool f_nan(float x) { return (f_bits(x) & 0x7FFFFFFFu) > 0x7F800000u; }

// The functions below are straight-line code: a pixel's point is computed whatever the pixel holds and `ok` chooses between it and
// the invalid pattern at the end (no operation here can trap, and what an invalid pixel would have given is never stored).  On the
// device that is also the cheaper form: a wave's lanes do not diverge over which pixels are valid.

// z of a depth sample already converted to float and multiplied by depth_scale: the range rules both depth kinds share
HAF_FRAME_HD bool depth_in_range(float z, const FrameMath &m)
{
    const bool below = m.min_depth > 0.0f && z < m.min_depth, above = m.max_depth > 0.0f && z > m.max_depth;
    return f_finite(z) && !below && !above;
}

// p[r] = ((t[r][0] xc + t[r][1] yc) + t[r][2] z) + t[r][3], left to right: the order the project fixes for M p
HAF_FRAME_HD void to_base(const FrameMath &m, float xc, float yc, float z, bool ok, float *p)
{
    for (int r = 0; r < 3; r++) {
        const float *t = m.t + 4 * r;
        const float v = f_add(f_add(f_add(f_mul(t[0], xc), f_mul(t[1], yc)), f_mul(t[2], z)), t[3]);
        p[r] = (ok && !f_nan(v)) ? v : f_from_bits(kInvalidWord);
    }
}

// pixel (u, v) of a depth frame: z = the sample times depth_scale, ok = the sample and z passed every rule
HAF_FRAME_HD void depth_point(const FrameMath &m, uint32_t u, uint32_t v, float z, bool ok, float *p)
{
    const float xc = f_mul(f_mul(f_sub((float)u, m.cx), m.ifx), z);
    const float yc = f_mul(f_mul(f_sub((float)v, m.cy), m.ify), z);
    to_base(m, xc, yc, z, ok, p);
}
HAF_FRAME_HD void point_u16(const FrameMath &m, uint32_t u, uint32_t v, uint16_t d, float *p)
{
    const float z = f_mul((float)d, m.depth_scale);
    depth_point(m, u, v, z, d != 0 && depth_in_range(z, m), p);
}
HAF_FRAME_HD void point_f32(const FrameMath &m, uint32_t u, uint32_t v, float d, float *p)
{
    const float z = f_mul(d, m.depth_scale);
    depth_point(m, u, v, z, f_finite(d) && d > 0.0f && depth_in_range(z, m), p);
}
// a sensor-frame point of an organised cloud: intrinsics, scale and limits play no part
HAF_FRAME_HD void point_xyz(const FrameMath &m, float x, float y, float z, float *p)
{
    to_base(m, x, y, z, f_finite(x) && f_finite(y) && f_finite(z), p);
}

}  // namespace haf_frame_math
