// transfer_rules.h -- the per-pixel rules of haf_transfer_labels (include/hafgrasp.h), written once: a depth pixel's point in the label
// camera's frame, its fixed-point words, the pixel of that camera it projects to, and the visibility test against the z-buffer.
//
// The same source is compiled for the device (transfer.hip) and for the host (transfer_host.cpp: haf_transfer_labels_ref, the definition
// of record), as label_shape.h is, on top of frame_points.h -- whose points and rounded fp32 operations these are -- and of
// plane_rules.h's usable coordinate.  Only the transform into the camera's frame is floating point: twelve rounded fp32 operations in
// to_base's order.  Everything behind it is integer arithmetic on words of 1/65536 m and 1/256 pixel, so no result depends on a
// division unit, on fusing, or on the order in which the z-buffer's atomics arrive.  The constants are formed ONCE per call on the host
// (transfer_host.cpp: transfer_rules), which both entry points call.
#pragma once
#include "../../include/hafgrasp.h"
#include "plane_rules.h"

namespace haf_transfer_math {

using namespace haf_plane_math;

constexpr float kTransferQuantum = 65536.0f;              // fixed-point words of a camera-frame coordinate: units of 1/65536 m
constexpr int32_t kTransferEmpty = INT32_MAX;             // a z-buffer word no point reached

// what the rules read of haf_camera and haf_transfer_params
struct TransferRules {
    float m[12];                                          // base_to_camera
    int32_t FX, FY, CX, CY;                               // rne(. * 256)
    int32_t NEAR, TA, TR;                                 // rne(. * 65536); NEAR >= 1, TA clamped to int32
    int32_t width, height;                                // the camera image
    int32_t splat;
};

// how far a pixel gets: its output is 0 unless it PROJECTS and is visible
enum { TRANSFER_NONE = 0, TRANSFER_FRONT = 1, TRANSFER_PROJECTS = 2 };

// THE rounding of a camera-frame coordinate: round-to-nearest-even(w * 65536) as int32.  |w| <= 16, so the product is exact and |Q| <= 2^20
#if defined(__HIP_DEVICE_COMPILE__)
HAF_FRAME_HD int32_t metre_word(float w) { return __float2int_rn(f_mul(w, kTransferQuantum)); }
#else
HAF_FRAME_HD int32_t metre_word(float w) { return (int32_t)lrintf(f_mul(w, kTransferQuantum)); }      // (the default rounding mode: to nearest even)
#endif

// floor(n / d) for 0 <= n < 2^15 d, 0 < d <= 2^28.  The host divides.  The device has no 64-bit divider: it takes a float estimate --
// the conversions, the reciprocal (1 ulp) and the product are each off by at most 2^-23 of a quotient below 2^15, so the truncated
// estimate is the quotient or a neighbour of it -- and settles it with the exact remainder.  What the estimate was leaves no trace
HAF_FRAME_HD int32_t pixel_quotient(int64_t n, int64_t d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int64_t q = (int64_t)__fmul_rn((float)n, __builtin_amdgcn_rcpf((float)d));
    int64_t r = n - q * d;
    if (r < 0) { q -= 1; r += d; }
    if (r >= d) q += 1;
    return (int32_t)q;
#else
    return (int32_t)(n / d);
#endif
}

// steps 1-3 of the header for one pixel: p = its point's three words (haf_frame_points').  Straight-line code like frame_points.h's: the
// words are computed whatever the pixel holds and chosen at the end
HAF_FRAME_HD int transfer_project(const TransferRules &r, const float *p, int32_t &Qz, int32_t &uc, int32_t &vc)
{
    float q[3];
    for (int k = 0; k < 3; k++) {
        const float *t = r.m + 4 * k;
        q[k] = f_add(f_add(f_add(f_mul(t[0], p[0]), f_mul(t[1], p[1])), f_mul(t[2], p[2])), t[3]);
    }
    const bool ok = f_finite(p[0]) && f_finite(p[1]) && f_finite(p[2]) && point_usable(q);
    Qz = 0; uc = 0; vc = 0;
    if (!ok) return TRANSFER_NONE;
    const int64_t Qx = metre_word(q[0]), Qy = metre_word(q[1]), Z = metre_word(q[2]);
    if (Z < (int64_t)r.NEAR) return TRANSFER_NONE;
    Qz = (int32_t)Z;
    const int64_t d = 256 * Z;
    const int64_t nu = (int64_t)r.FX * Qx + ((int64_t)r.CX + 128) * Z, nv = (int64_t)r.FY * Qy + ((int64_t)r.CY + 128) * Z;
    if (nu < 0 || nu >= (int64_t)r.width * d || nv < 0 || nv >= (int64_t)r.height * d) return TRANSFER_FRONT;
    uc = pixel_quotient(nu, d);
    vc = pixel_quotient(nv, d);
    return TRANSFER_PROJECTS;
}

// step 5: a point of depth word Qz against the z-buffer's word at its own pixel (never above Qz once the buffer is complete)
HAF_FRAME_HD bool transfer_visible(const TransferRules &r, int32_t Qz, int32_t Z)
{
    return (int64_t)Qz - (int64_t)Z <= (int64_t)r.TA + (((int64_t)r.TR * (int64_t)Z) >> 16);
}

// step 6: a label image's value as haf_grasp_map_labels reads it: 0 and values above n_labels count as 0
HAF_FRAME_HD uint32_t transfer_label(uint32_t l, int32_t n_labels) { return l > (uint32_t)n_labels ? 0u : l; }

}  // namespace haf_transfer_math
