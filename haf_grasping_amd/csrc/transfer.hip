// transfer.hip -- haf_transfer_labels (include/hafgrasp.h): another camera's label image carried over to a depth frame's pixels, with the
// occlusion test a nearest-pixel lookup lacks.  The per-pixel rules are transfer_rules.h's, the same source haf_transfer_labels_ref
// runs on the host: two rounded fp32 transforms, then integers.  The z-buffer is a minimum and the counters are integer sums, which no
// order of arrival changes, so the two agree word for word (tests/test_transfer_gpu.py).
//
// A fill and two launches on one stream, each reading only what an EARLIER one wrote or what reaches it through atomics:
//   fill                          the z-buffer's r.width * r.height words = INT32_MAX.
//   k_transfer_splat<KIND>        a lane owns the group of G pixels frame_group.h gives it (eight of a U16 frame, four of the others),
//                                 projects each and sends atomicMin to the (2 splat + 1)^2 words around its pixel, clipped to the
//                                 camera image.  The minimum only ever falls: the lane LOADS the word first and skips the atomic when
//                                 what it sees is already <= Qz.  A stale read costs an atomic that was not needed, never a result.
//   k_transfer_gather<KIND, LIN, LOUT>   recomputes the projection (deterministic; 8 bytes per pixel of scratch saved), reads the
//                                 complete z-buffer at the own pixel, applies the visibility rule, reads the camera's label there and
//                                 writes the output label -- a group's labels in one store where they lie in one row at an aligned
//                                 address, pixel by pixel elsewhere.  The four counters are summed per wave by ballot and popcount,
//                                 across the workgroup's waves in LDS, and sent with ONE integer atomic per workgroup and counter.
// The quotients of the projection need no 64-bit division (transfer_rules.h: pixel_quotient): a float estimate, off by one at most,
// settled by the exact remainder in int64.  Read in the ISA of a one-quotient kernel: about 50 instructions and no branch (the int64 ->
// float conversion is most of them), where the compiler's int64 `/` is about 150 with three branches.
// Bounds: a pixel is read only for i < n (group_points).  uc < r.width and vc < r.height by the projection's own test, and a window is
// clipped to the image before it names a word, so every z-buffer index is in [0, r.width * r.height); the camera's label is read at
// (uc, vc), inside its image; an output label is stored only for i < n, at its own (row, column) or by one store inside a row.
#include "frame_group.h"
#include "kernels.h"

namespace haf {

using namespace haf_transfer_math;

typedef unsigned v2u_transfer __attribute__((ext_vector_type(2)));

template <int KIND>
__global__ __launch_bounds__(kFrameThreads) void k_transfer_splat(const TransferDev d)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned n = (unsigned)d.f.n;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;
    if (i0 >= n) return;                                  // (the kernel has no barrier)
    float p[G * 3];
    group_points<KIND>(d.f, i0, n, p);
    const int Wc = d.r.width, Hc = d.r.height, splat = d.r.splat;
#pragma unroll
    for (unsigned k = 0; k < G; k++) {
        int32_t Qz, uc, vc;
        if (i0 + k >= n || transfer_project(d.r, p + 3 * k, Qz, uc, vc) != TRANSFER_PROJECTS) continue;
        const int u_lo = max(uc - splat, 0), u_hi = min(uc + splat, Wc - 1), v_lo = max(vc - splat, 0), v_hi = min(vc + splat, Hc - 1);
        for (int v = v_lo; v <= v_hi; v++)
            for (int u = u_lo; u <= u_hi; u++) {
                int *word = d.z + (size_t)v * (size_t)Wc + (size_t)u;
                if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > Qz) atomicMin(word, Qz);
            }
    }
}

template <int LB> __device__ __forceinline__ unsigned camera_label(const TransferDev &d, int uc, int vc)
{
    const char *s = static_cast<const char *>(d.labels) + (size_t)vc * d.label_stride + (size_t)uc * LB;
    if constexpr (LB == 2) return *as_global<const uint16_t>(s);
    else return *as_global<const unsigned char>(s);
}

template <int KIND, int LIN, int LOUT>
__global__ __launch_bounds__(kFrameThreads) void k_transfer_gather(const TransferDev d)
{
    constexpr unsigned G = frame_group<KIND>();
    __shared__ unsigned s_cnt[kFrameThreads / 64][TRANSFER_CNT_WORDS];
    const unsigned n = (unsigned)d.f.n, W = (unsigned)d.f.width;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;
    unsigned lab[G] = {};
    unsigned front = 0, projects = 0, visible = 0;        // bit k: pixel i0 + k
    if (i0 < n) {
        float p[G * 3];
        group_points<KIND>(d.f, i0, n, p);
#pragma unroll
        for (unsigned k = 0; k < G; k++) {
            if (i0 + k >= n) continue;
            int32_t Qz, uc, vc;
            const int stage = transfer_project(d.r, p + 3 * k, Qz, uc, vc);
            front |= stage >= TRANSFER_FRONT ? 1u << k : 0u;
            if (stage != TRANSFER_PROJECTS) continue;
            projects |= 1u << k;
            const int Z = d.z[(size_t)vc * (size_t)d.r.width + (size_t)uc];
            if (!transfer_visible(d.r, Qz, Z)) continue;
            visible |= 1u << k;
            lab[k] = transfer_label(camera_label<LIN>(d, uc, vc), d.n_labels);
        }
        const unsigned v0 = i0 / W, u0 = i0 - v0 * W;
        char *a = static_cast<char *>(d.out) + (size_t)v0 * d.out_stride + (size_t)u0 * LOUT;
        if (i0 + G <= n && u0 + G <= W && (reinterpret_cast<uintptr_t>(a) & (G * LOUT - 1u)) == 0) {
            unsigned w[G * LOUT / 4] = {};
#pragma unroll
            for (unsigned k = 0; k < G; k++) {
                if constexpr (LOUT == 2) w[k >> 1] |= lab[k] << (16 * (k & 1));
                else w[k >> 2] |= lab[k] << (8 * (k & 3));
            }
            if constexpr (G * LOUT == 16) { v4u q; q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3]; *as_global<v4u>(a) = q; }
            else if constexpr (G * LOUT == 8) { v2u_transfer q; q.x = w[0]; q.y = w[1]; *as_global<v2u_transfer>(a) = q; }
            else *as_global<unsigned>(a) = w[0];
        } else {
            unsigned u = u0, v = v0;
#pragma unroll
            for (unsigned k = 0; k < G; k++) {
                if (i0 + k < n) {                         // (v < height: inside the output image)
                    char *o = static_cast<char *>(d.out) + (size_t)v * d.out_stride + (size_t)u * LOUT;
                    if constexpr (LOUT == 2) *as_global<uint16_t>(o) = (uint16_t)lab[k];
                    else *as_global<unsigned char>(o) = (unsigned char)lab[k];
                }
                if (++u == W) { u = 0; v++; }
            }
        }
    }
    // the wave's four sums (uniform), then the workgroup's
    unsigned sums[TRANSFER_CNT_WORDS] = {};
#pragma unroll
    for (unsigned k = 0; k < G; k++) {
        sums[TRANSFER_CNT_FRONT] += (unsigned)__popcll(__ballot((front >> k) & 1u));
        sums[TRANSFER_CNT_PROJECTS] += (unsigned)__popcll(__ballot((projects >> k) & 1u));
        sums[TRANSFER_CNT_VISIBLE] += (unsigned)__popcll(__ballot((visible >> k) & 1u));
        sums[TRANSFER_CNT_LABELLED] += (unsigned)__popcll(__ballot(lab[k] != 0u));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < TRANSFER_CNT_WORDS; c++) s_cnt[wave][c] = sums[c];
    }
    __syncthreads();
    if (threadIdx.x < TRANSFER_CNT_WORDS) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kFrameThreads / 64; w++) total += s_cnt[w][threadIdx.x];
        if (total) atomicAdd(d.counters + threadIdx.x, total);
    }
}

template <int KIND, int LIN> static void launch_gather_out(const TransferDev &d, dim3 grid, dim3 block, hipStream_t s)
{
    if (d.elem_bytes == 2) hipLaunchKernelGGL((k_transfer_gather<KIND, LIN, 2>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((k_transfer_gather<KIND, LIN, 1>), grid, block, 0, s, d);
}

template <int KIND> static void launch_transfer_kind(const TransferDev &d, hipStream_t s)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned groups = ((unsigned)d.f.n + G - 1) / G;
    if (!groups) return;
    const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads), block(kFrameThreads);
    hipLaunchKernelGGL((k_transfer_splat<KIND>), grid, block, 0, s, d);
    if (d.label_bytes == 2) launch_gather_out<KIND, 2>(d, grid, block, s);
    else launch_gather_out<KIND, 1>(d, grid, block, s);
}

hipError_t launch_transfer(const TransferDev &d, hipStream_t s)
{
    const hipError_t rc = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.z), kTransferEmpty, (size_t)d.r.width * (size_t)d.r.height, s);
    if (rc != hipSuccess) return rc;
    if (d.f.kind == HAF_FRAME_DEPTH_U16) launch_transfer_kind<HAF_FRAME_DEPTH_U16>(d, s);
    else if (d.f.kind == HAF_FRAME_DEPTH_F32) launch_transfer_kind<HAF_FRAME_DEPTH_F32>(d, s);
    else launch_transfer_kind<HAF_FRAME_XYZ_F32>(d, s);
    return hipSuccess;
}

}  // namespace haf
