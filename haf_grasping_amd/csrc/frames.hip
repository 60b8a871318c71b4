// frames.hip -- k_frame_points<KIND>: the pixels of the sensor frames of a haf_score_frames batch -> packed base-frame xyz in the points
// area of the request's input block, where a staged host cloud would lie (engine_request.cpp: upload_frames).  The arithmetic is
// frame_points.h's, the same source haf_frame_points runs on the host: the two agree bit for bit (tests/test_frames_gpu.py).
//
// A streaming kernel, 2-4 bytes in and 12 out per pixel.  A lane owns a GROUP of consecutive points by flat index v * width + u: eight
// of a U16 frame, four of an F32 or XYZ frame -- 16 bytes of pixels, 96 or 48 bytes of points.
//   * loads: a group that lies inside one row at a 16-byte aligned address is ONE global_load_dwordx4 (neighbouring lanes read
//     neighbouring 16 bytes); any other group -- a row's head or tail where the width is not a multiple of the group, a base or row stride
//     that is not 16-byte aligned, the last group of the frame -- reads its pixels one by one, each from its own (row, column).  A 640-wide
//     frame at an aligned base has no such group.  A packed XYZ frame (12-byte points, no row padding) is three dwordx4 loads per group
//     whatever its width;
//   * stores: a frame's points start at a multiple of four points from a 16-byte aligned base, so a whole group is 6 (3) aligned
//     global_store_dwordx4; only the frame's last, partial group stores words.
// A staged host XYZ frame is transformed IN PLACE (src == dst): a lane reads all of its own points before it writes any, and no lane
// touches another's.  One launch per kind present in the batch covers every frame of the batch (grid.y); a block whose frame is of
// another kind or ends before it returns at once.  The per-frame constants are wave-uniform: scalar loads.
//
// k_view_points<KIND> (haf_score_views): the same group ownership, loads and arithmetic (group_points below serves both kernels), but
// only the VALID points are stored -- those whose three words are all finite, the rule of haf_view_points -- packed from the start of the
// request's region, which all its views share:
//   * a lane counts the valid points among its 8 or 4, a shuffle scan gives its prefix inside the wave, the waves' totals meet in LDS;
//   * ONE integer atomic add per workgroup advances the request's live counter (CloudDev::n, uploaded as 0) and returns the workgroup's
//     base; no workgroup waits for another, so the ORDER of the compacted points is whatever order the atomics arrive in -- their
//     multiset and their number are exact, and every later stage is order independent (binning keeps a maximum, the bucket sort groups);
//   * a lane stores its valid points one after the other at base + prefix, 12 bytes each at a 4-byte aligned address.
// A view never reads where the kernel writes: staged host views of every kind lie in raw areas of their own (engine_request.cpp).
#include "frame_group.h"

namespace haf {

template <int KIND>
__global__ __launch_bounds__(kFrameThreads) void k_frame_points(const FrameDev *__restrict__ frames)
{
    constexpr unsigned G = frame_group<KIND>();
    const FrameDev &f = frames[blockIdx.y];
    if (f.kind != KIND) return;
    const unsigned n = (unsigned)f.n;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;      // (n < 2^31 and at most 2^11 points of slack: no wrap)
    if (i0 >= n) return;
    const bool whole = i0 + G <= n;
    float p[G * 3];
    group_points<KIND>(f, i0, n, p);

    const global_ptr<float> dst = as_global<float>(f.dst + (size_t)i0 * 3);
    if (whole) {
        const global_ptr<v4f> o = as_global<v4f>(f.dst + (size_t)i0 * 3);
#pragma unroll
        for (unsigned j = 0; j < G * 3 / 4; j++) o[j] = v4f{p[4 * j], p[4 * j + 1], p[4 * j + 2], p[4 * j + 3]};
    } else {
#pragma unroll
        for (unsigned k = 0; k < G; k++)
            if (i0 + k < n) { dst[3 * k] = p[3 * k]; dst[3 * k + 1] = p[3 * k + 1]; dst[3 * k + 2] = p[3 * k + 2]; }
    }
}

// A workgroup of k_view_points stays whole until its one atomic: the lanes beyond the view's end count nothing.  Bounds: a request's
// counter ends at the number of its valid pixels, at most the pixels of its views, which is what its region holds (pack_headers).
template <int KIND>
__global__ __launch_bounds__(kFrameThreads) void k_view_points(const FrameDev *__restrict__ frames)
{
    constexpr unsigned G = frame_group<KIND>();
    constexpr unsigned kWaves = kFrameThreads / 64;
    __shared__ unsigned s_wave[kWaves];
    __shared__ unsigned s_base;
    const FrameDev &f = frames[blockIdx.y];
    if (f.kind != KIND) return;
    const unsigned n = (unsigned)f.n;
    if (blockIdx.x * (unsigned)kFrameThreads * G >= n) return;                           // (the whole workgroup: nobody misses the barriers)
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;
    float p[G * 3];
    group_points<KIND>(f, i0, n, p);
    unsigned ok = 0;                                                                     // bit k: point i0 + k exists and is finite in every word
#pragma unroll
    for (unsigned k = 0; k < G; k++)
        if (i0 + k < n && f_finite(p[3 * k]) && f_finite(p[3 * k + 1]) && f_finite(p[3 * k + 2])) ok |= 1u << k;
    const unsigned cnt = (unsigned)__popc(ok), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned incl = cnt;                                                                 // inclusive scan over the wave
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (unsigned w = 0; w < kWaves; w++) total += s_wave[w];
        s_base = total ? (unsigned)atomicAdd(f.count, (int)total) : 0u;
    }
    __syncthreads();
    unsigned pos = s_base + incl - cnt;
#pragma unroll
    for (unsigned w = 0; w + 1 < kWaves; w++) pos += w < wave ? s_wave[w] : 0u;
    global_ptr<float> dst = as_global<float>(f.dst + (size_t)pos * 3);
#pragma unroll
    for (unsigned k = 0; k < G; k++)
        if (ok & (1u << k)) { dst[0] = p[3 * k]; dst[1] = p[3 * k + 1]; dst[2] = p[3 * k + 2]; dst += 3; }
}

template <int KIND, bool VIEWS> static void launch_kind(const FrameDev *frames_dev, const FrameDev *frames_host, int n_frames, hipStream_t s)
{
    constexpr unsigned G = frame_group<KIND>();
    unsigned groups = 0;
    for (int b = 0; b < n_frames; b++)
        if (frames_host[b].kind == KIND) groups = std::max(groups, ((unsigned)frames_host[b].n + G - 1) / G);
    if (!groups) return;
    for (int b0 = 0; b0 < n_frames; b0 += 65535) {            // (grid.y holds 65535 frames)
        const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads, (unsigned)std::min(65535, n_frames - b0));
        if (VIEWS) hipLaunchKernelGGL(k_view_points<KIND>, grid, dim3(kFrameThreads), 0, s, frames_dev + b0);
        else hipLaunchKernelGGL(k_frame_points<KIND>, grid, dim3(kFrameThreads), 0, s, frames_dev + b0);
    }
}

void launch_frame_points(const FrameDev *frames_dev, const FrameDev *frames_host, int n_frames, hipStream_t s)
{
    launch_kind<HAF_FRAME_DEPTH_U16, false>(frames_dev, frames_host, n_frames, s);
    launch_kind<HAF_FRAME_DEPTH_F32, false>(frames_dev, frames_host, n_frames, s);
    launch_kind<HAF_FRAME_XYZ_F32, false>(frames_dev, frames_host, n_frames, s);
}

void launch_view_points(const FrameDev *views_dev, const FrameDev *views_host, int n_views, hipStream_t s)
{
    launch_kind<HAF_FRAME_DEPTH_U16, true>(views_dev, views_host, n_views, s);
    launch_kind<HAF_FRAME_DEPTH_F32, true>(views_dev, views_host, n_views, s);
    launch_kind<HAF_FRAME_XYZ_F32, true>(views_dev, views_host, n_views, s);
}

}  // namespace haf
