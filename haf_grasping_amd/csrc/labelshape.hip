// labelshape.hip -- haf_measure_labels (include/hafgrasp.h): per instance label of a label image the integer accumulators of its points
// in the base frame -- counts, coordinate sums, the box, the extents along twelve directions, the largest height.  The per-point rules
// are label_shape.h's, the same source haf_measure_labels_ref runs on the host; every accumulator is an integer sum, minimum or maximum,
// which no order of arrival changes, so the two agree word for word (tests/test_label_shape_gpu.py).
//
// ONE launch, k_label_shape<KIND, LABEL_BYTES>.  A lane owns the group of G pixels frame_group.h gives it (eight of a U16 frame, four of
// the others) and reads the group's labels FIRST, as k_map_labels does: a wave without a label in 1..n_labels ends there -- one load,
// no deprojection, no atomic -- and a lane without one skips the deprojection.  A label carries 36 accumulators: a table per label
// does not fit LDS at 4096 labels, and a global atomic per pixel is out of the question.  So the wave works label by label, the
// wave-leader loop of segment.hip's wave_add_by_key: the first lane that still has an unretired pixel names that pixel's label, every
// lane folds those of ITS pixels that carry it into one ShapeAcc (label_shape.h: shape_add_pixel) and retires them, the wave reduces
// the accumulators by xor shuffles -- not when a single lane holds the label -- and the leader sends ONE set of integer atomics to the
// label's row of the global table, which the caller zeroed: atomicAdd for the counts and the three 64-bit sums, atomicMax for every
// extent and for the height key (label_shape.h: a minimum travels as the maximum of its complement, so that zero is the empty value).
// Compact objects cost a wave a few passes; an image whose every pixel differs costs a pass per pixel, 64 G at most, each without the
// shuffles: the loop is bounded by the pixels a wave owns.
// Bounds: a label is loaded only for a pixel i < n, at its own (row, column) or by one aligned load inside a row (label_group.h); a pixel's words by
// group_points, which k_grasp_map bounds the same way; a value above n_labels is cleared before it names a row, so a row index is in
// [0, n_labels).
#include "label_group.h"
#include "kernels.h"

namespace haf {

using namespace haf_shape_math;

typedef ShapeAcc<int> WaveAcc;

__device__ __forceinline__ int wave_sum(int x)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int wave_min(int x)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) x = min(x, __shfl_xor(x, off));
    return x;
}
__device__ __forceinline__ int wave_max(int x)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) x = max(x, __shfl_xor(x, off));
    return x;
}

// every lane's accumulators -> the wave's, in every lane (the lanes that hold nothing of the label carry the empty values)
__device__ __forceinline__ void wave_reduce(WaveAcc &a)
{
    a.n_pixels = wave_sum(a.n_pixels);
    a.n_points = wave_sum(a.n_points);
#pragma unroll
    for (int j = 0; j < 3; j++) { a.sum[j] = wave_sum(a.sum[j]); a.q_min[j] = wave_min(a.q_min[j]); a.q_max[j] = wave_max(a.q_max[j]); }
#pragma unroll
    for (int k = 0; k < kShapeDirs; k++) { a.t_min[k] = wave_min(a.t_min[k]); a.t_max[k] = wave_max(a.t_max[k]); }
    a.h_key = wave_max(a.h_key);
}

// one lane: the wave's accumulators of one label into the label's row
__device__ __forceinline__ void row_send(unsigned *row, const WaveAcc &a, bool use_plane)
{
    atomicAdd(row + kShapeRowPixels, (unsigned)a.n_pixels);
    if (a.n_points == 0) return;                          // (every other word would keep what it holds)
    atomicAdd(row + kShapeRowPoints, (unsigned)a.n_points);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(row + kShapeRowSum);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        atomicAdd(sums + j, (unsigned long long)(long long)a.sum[j]);      // (two's complement: a negative sum wraps to the right word)
        atomicMax(row + kShapeRowQMin + j, shape_enc(~a.q_min[j]));
        atomicMax(row + kShapeRowQMax + j, shape_enc(a.q_max[j]));
    }
#pragma unroll
    for (int k = 0; k < kShapeDirs; k++) {
        atomicMax(row + kShapeRowTMin + k, shape_enc(~a.t_min[k]));
        atomicMax(row + kShapeRowTMax + k, shape_enc(a.t_max[k]));
    }
    if (use_plane && a.h_key != kShapeNone) atomicMax(row + kShapeRowHKey, shape_enc(a.h_key));
}

template <int KIND, int LB>
__global__ __launch_bounds__(kFrameThreads) void k_label_shape(const ShapeDev d)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned n = (unsigned)d.f.n, Wf = (unsigned)d.f.width;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;
    unsigned lab[G];                                      // (0, or 1..n_labels: a label above n_labels is ignored like background)
    group_labels<G, LB>(d.labels, d.label_stride, Wf, n, i0, d.n_labels, lab);
    unsigned pending = 0;                                 // bit k: pixel i0 + k carries a label and is not folded yet
#pragma unroll
    for (unsigned k = 0; k < G; k++) pending |= lab[k] != 0u ? 1u << k : 0u;
    unsigned long long todo = __ballot(pending != 0u);
    if (!todo) return;                                    // (wave-uniform; the kernel has no barrier)
    float p[G * 3] = {};
    if (pending) group_points<KIND>(d.f, i0, n, p);
    const float plane[4] = {d.plane[0], d.plane[1], d.plane[2], d.plane[3]};
    const bool use_plane = d.use_plane != 0;
    while (todo) {                                        // (uniform; every pass retires at least the leader's first pending pixel)
        const unsigned leader = (unsigned)__ffsll((long long)todo) - 1u;
        unsigned mine = 0u;                               // the label of this lane's first pending pixel
#pragma unroll
        for (int k = (int)G - 1; k >= 0; k--) mine = (pending >> k) & 1u ? lab[k] : mine;
        const unsigned cur = (unsigned)__shfl((int)mine, (int)leader);
        WaveAcc acc;
        shape_clear(acc);
#pragma unroll
        for (unsigned k = 0; k < G; k++)
            if (((pending >> k) & 1u) && lab[k] == cur) {
                shape_add_pixel(acc, p + 3 * k, plane, use_plane);
                pending &= ~(1u << k);
            }
        const unsigned long long same = __ballot(acc.n_pixels != 0);
        if (__popcll(same) > 1) wave_reduce(acc);         // (uniform)
        if (lane == leader) row_send(d.table + (size_t)(cur - 1u) * kShapeRowWords, acc, use_plane);
        todo = __ballot(pending != 0u);
    }
}

template <int KIND> static void launch_label_shape_kind(const ShapeDev &d, hipStream_t s)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned groups = ((unsigned)d.f.n + G - 1) / G;
    if (!groups) return;
    const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads), block(kFrameThreads);
    if (d.label_bytes == 2) hipLaunchKernelGGL((k_label_shape<KIND, 2>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((k_label_shape<KIND, 1>), grid, block, 0, s, d);
}

void launch_label_shape(const ShapeDev &d, hipStream_t s)
{
    if (d.f.kind == HAF_FRAME_DEPTH_U16) launch_label_shape_kind<HAF_FRAME_DEPTH_U16>(d, s);
    else if (d.f.kind == HAF_FRAME_DEPTH_F32) launch_label_shape_kind<HAF_FRAME_DEPTH_F32>(d, s);
    else launch_label_shape_kind<HAF_FRAME_XYZ_F32>(d, s);
}

}  // namespace haf
