// device_common.h -- small device helpers shared by the kernel translation units (prestages.hip, features.hip, contraction.hip,
// recheck.hip, vote.hip).
#pragma once
#include "kernels.h"
#include "decq.h"
#include "screen_finish.h"
#include <string.h>
#include <type_traits>

namespace haf {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int f2key(float f)
{
    int b = __float_as_int(f);
    return b >= 0 ? b : (b ^ 0x7FFFFFFF);
}
__device__ __forceinline__ float key2f(int k)
{
    return __int_as_float(k >= 0 ? k : (k ^ 0x7FFFFFFF));
}

// The z window of cell (row, col) of one roll's height grid (pick_rules.h) by ONE WHOLE WAVE: lane l takes slots l and l + 64, a
// butterfly leaves the maximum in every lane -> the ordered key; key2f of it is the record's h_locmax.  Every lane of the wave calls it
__device__ __forceinline__ int wave_z_window(const float *__restrict__ heights_of_roll, int row, int col, int H, int W)
{
    int zk = haf_pick_math::z_window_start();
    for (int q = threadIdx.x & 63; q < haf_pick_math::kZWindowSlots; q += 64) {
        int rr, cc;
        if (haf_pick_math::z_window_slot(q, row, col, H, W, &rr, &cc)) zk = haf_pick_math::z_window_fold(zk, heights_of_roll[(size_t)rr * W + cc]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zk = max(zk, __shfl_xor(zk, o, 64));
    return zk;
}

// The record of cell (row, col) of one roll by one whole wave: the cell's vote, the cell, its z window and the roll's n_evals.  ev16_roll
// / heights_roll: that roll's grids; 0 <= row < H, 0 <= col < W.  Every lane gets the record, lane 0 is the one that stores it
__device__ __forceinline__ RollRecordDev cell_record(const short *__restrict__ ev16_roll, const float *__restrict__ heights_roll, int n_evals,
                                                     int row, int col, int H, int W)
{
    RollRecordDev q;
    q.vote = ev16_roll[(size_t)row * W + col];
    q.row = (short)row; q.col = (short)col;
    q.h_locmax = key2f(wave_z_window(heights_roll, row, col, H, W));
    q.n_evals = n_evals;
    return q;
}

// entries of a list of `total` that fall into the window [off, off + cap)
__device__ __forceinline__ int window_count(int total, int off, int cap) { return max(0, min(total - off, cap)); }

// Ordered hand-over lists (round 5).  A tier's combine kernel leaves one bit per entry of its window -- "undecided" -- in ballot words
// (word w = entries 64 w .. 64 w + 63 of the window); list_compact_body, ONE workgroup of kListCompactThreads, appends the flagged
// entries' evaluations to the next tier's list in the order of the window and publishes the new total: the list is the same from run to
// run (until then every undecided entry took its slot with an atomicAdd, whoever came first).  Windows follow each other on the
// stream, so "append" is counters[out_slot] as the previous window left it.
constexpr int kListCompactThreads = 1024;
__device__ __forceinline__ void list_compact_body(const unsigned long long *__restrict__ words, int n_entries, const int *__restrict__ src,
                                                  int *__restrict__ dst, int dst_cap, int *__restrict__ counters, int out_slot, int *s_scan)
{
    const int t = threadIdx.x;
    const int n_words = (n_entries + 63) >> 6;
    const int chunk = (n_words + kListCompactThreads - 1) / kListCompactThreads;
    const int w0 = min(t * chunk, n_words), w1 = min(w0 + chunk, n_words);
    int mine = 0;
    for (int w = w0; w < w1; w++) mine += __popcll(words[w]);
    s_scan[t] = mine;
    __syncthreads();
    for (int o = 1; o < kListCompactThreads; o <<= 1) {
        const int v = (t >= o) ? s_scan[t - o] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const int base0 = counters[out_slot];
    int slot = base0 + s_scan[t] - mine;
    const int total = s_scan[kListCompactThreads - 1];
    for (int w = w0; w < w1; w++) {
        unsigned long long m = words[w];
        while (m) {
            const int b = __ffsll((long long)m) - 1;
            m &= m - 1;
            if (slot < dst_cap) dst[slot] = src[w * 64 + b];
            slot++;
        }
    }
    __syncthreads();                                     // every thread has read the old total
    if (t == 0) counters[out_slot] = base0 + total;
}

// (sqrt_upper, exp2m1_upper: screen_finish.h, host and device)

}  // namespace haf
