// frame_group.h -- how a lane of the frame kernels owns its pixels (frames.hip: k_frame_points, k_view_points; graspmap.hip: k_grasp_map):
// a GROUP of consecutive points by flat index v * width + u -- eight of a U16 frame, four of an F32 or XYZ frame, 16 bytes of pixels --
// read with one global_load_dwordx4 where the group lies inside one row at a 16-byte aligned address, pixel by pixel elsewhere, and
// turned into base-frame points by frame_points.h's arithmetic.  Device code only.
#pragma once
#include "device_common.h"
#include "../../include/hafgrasp.h"

namespace haf {

using namespace haf_frame_math;

constexpr int kFrameThreads = 256;
// the frame's two pointers come out of the descriptor, where the compiler cannot see their address space: said here, so that the
// accesses are global_load / global_store and not flat ones
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
template <class T> using global_ptr = __attribute__((address_space(1))) T *;
template <class T> __device__ __forceinline__ global_ptr<T> as_global(const void *p) { return (global_ptr<T>)(uintptr_t)p; }
template <int KIND> constexpr unsigned frame_group() { return KIND == HAF_FRAME_DEPTH_U16 ? 8u : 4u; }
// a launcher's switch over the frame kind, once: call(K) with K a std::integral_constant whose ::value is the kind (a checked frame has
// one of the three); the caller names its kernel instance as decltype(K)::value
template <class F> inline void with_frame_kind(int kind, F &&call)
{
    if (kind == HAF_FRAME_DEPTH_U16) call(std::integral_constant<int, HAF_FRAME_DEPTH_U16>{});
    else if (kind == HAF_FRAME_DEPTH_F32) call(std::integral_constant<int, HAF_FRAME_DEPTH_F32>{});
    else call(std::integral_constant<int, HAF_FRAME_XYZ_F32>{});
}

// the points of the group that starts at flat index i0 of frame f (n pixels): p[3k..3k+2] = point i0 + k; what lies beyond the frame's
// end is computed from zero words and never stored
template <int KIND>
__device__ __forceinline__ void group_points(const FrameDev &f, unsigned i0, unsigned n, float (&p)[frame_group<KIND>() * 3])
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned W = (unsigned)f.width;
    const unsigned v0 = i0 / W, u0 = i0 - v0 * W;
    const bool whole = i0 + G <= n;
    const char *src = static_cast<const char *>(f.src);
    const unsigned long long rs = f.row_stride;
    // the group's raw words first -- one wide load, or pixel by pixel from each one's own (row, column) -- then ONE pass of arithmetic
    // over them; a pixel beyond the frame's end keeps a zero word and its point is never stored
    constexpr unsigned RAW = KIND == HAF_FRAME_XYZ_F32 ? 3 * G : G;      // 32-bit words (a U16 sample per word)
    unsigned raw[RAW] = {};
    if constexpr (KIND == HAF_FRAME_XYZ_F32) {
        const char *a = src + (size_t)i0 * 12;
        if (whole && f.point_stride == 12u && rs == (unsigned long long)W * 12ull && (reinterpret_cast<uintptr_t>(a) & 15u) == 0) {
            const global_ptr<const v4u> q = as_global<const v4u>(a);
            const v4u w0 = q[0], w1 = q[1], w2 = q[2];
            raw[0] = w0.x; raw[1] = w0.y; raw[2] = w0.z; raw[3] = w0.w; raw[4] = w1.x; raw[5] = w1.y; raw[6] = w1.z; raw[7] = w1.w;
            raw[8] = w2.x; raw[9] = w2.y; raw[10] = w2.z; raw[11] = w2.w;
        } else {
            unsigned u = u0, v = v0;
#pragma unroll
            for (unsigned k = 0; k < G; k++) {
                if (i0 + k < n) {
                    const global_ptr<const unsigned> s = as_global<const unsigned>(src + (size_t)v * rs + (size_t)u * f.point_stride);
                    raw[3 * k] = s[0]; raw[3 * k + 1] = s[1]; raw[3 * k + 2] = s[2];
                }
                if (++u == W) { u = 0; v++; }
            }
        }
    } else {
        constexpr unsigned E = KIND == HAF_FRAME_DEPTH_U16 ? 2u : 4u;
        const char *a = src + (size_t)v0 * rs + (size_t)u0 * E;
        if (whole && u0 + G <= W && (reinterpret_cast<uintptr_t>(a) & 15u) == 0) {
            const v4u w4 = *as_global<const v4u>(a);
            const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (unsigned k = 0; k < G; k++) raw[k] = KIND == HAF_FRAME_DEPTH_U16 ? (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu : w[k];
        } else {
            unsigned u = u0, v = v0;
#pragma unroll
            for (unsigned k = 0; k < G; k++) {
                if (i0 + k < n) {
                    const char *s = src + (size_t)v * rs + (size_t)u * E;
                    if constexpr (KIND == HAF_FRAME_DEPTH_U16) raw[k] = *as_global<const uint16_t>(s);
                    else raw[k] = *as_global<const unsigned>(s);
                }
                if (++u == W) { u = 0; v++; }
            }
        }
    }
    unsigned u = u0, v = v0;
#pragma unroll
    for (unsigned k = 0; k < G; k++) {
        if constexpr (KIND == HAF_FRAME_DEPTH_U16) point_u16(f.m, u, v, (uint16_t)raw[k], p + 3 * k);
        else if constexpr (KIND == HAF_FRAME_DEPTH_F32) point_f32(f.m, u, v, __uint_as_float(raw[k]), p + 3 * k);
        else point_xyz(f.m, __uint_as_float(raw[3 * k]), __uint_as_float(raw[3 * k + 1]), __uint_as_float(raw[3 * k + 2]), p + 3 * k);
        if (++u == W) { u = 0; v++; }
    }
}

// the point of ONE pixel (u, v) inside the frame: for the kernels that own their pixels singly (segment.hip, plane.hip)
template <int KIND> __device__ __forceinline__ void pixel_point(const FrameDev &f, int u, int v, float *p)
{
    const char *row = static_cast<const char *>(f.src) + (size_t)v * f.row_stride;
    if constexpr (KIND == HAF_FRAME_DEPTH_U16) point_u16(f.m, (uint32_t)u, (uint32_t)v, *as_global<const uint16_t>(row + (size_t)u * 2), p);
    else if constexpr (KIND == HAF_FRAME_DEPTH_F32) point_f32(f.m, (uint32_t)u, (uint32_t)v, __uint_as_float(*as_global<const unsigned>(row + (size_t)u * 4)), p);
    else {
        const global_ptr<const unsigned> s = as_global<const unsigned>(row + (size_t)u * f.point_stride);
        point_xyz(f.m, __uint_as_float(s[0]), __uint_as_float(s[1]), __uint_as_float(s[2]), p);
    }
}

}  // namespace haf
