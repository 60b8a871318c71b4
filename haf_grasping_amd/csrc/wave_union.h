// wave_union.h -- what the two segmenters' kernels share (segment.hip: pixels, cellsegment.hip: cells of the top-down grid): the lock-free
// union-find on a parent array, the wave's aggregation of equal keys into one atomic each, and the workgroup's prefix sum.  Device code only.
//
// The union-find: parent[x] <= x always, a root is the lowest index of its set (the component's anchor), and uniting a and b is "find
// both roots, atomicMin the larger one's parent word with the smaller; if the word held something else, go on with what it held".  Every
// pass of that loop lowers the larger of its two indices, so a lane's loop ends on its own progress; no lane waits for another lane or
// workgroup.  A stale read in a find only yields a former ancestor -- still a member of the same set -- and the atomic that follows
// returns the true word.
#pragma once
#include <hip/hip_runtime.h>

namespace haf {

constexpr int kScanThreads = 256;                         // lanes of a workgroup that calls block_scan

// a parent word as another lane may have just changed it: never kept in a register across a loop
template <bool LDS> __device__ __forceinline__ int uf_load(const int *p)
{
    if constexpr (LDS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (parent[x] < x unless x is a root: the walk goes down and ends)
template <bool LDS> __device__ __forceinline__ int uf_find(const int *parent, int a)
{
    for (;;) {
        const int p = uf_load<LDS>(parent + a);
        if (p == a) return a;
        a = p;
    }
}
// a and b are foreground.  Each pass that does not end the loop replaces the larger index by a smaller one
template <bool LDS> __device__ __forceinline__ void uf_unite(int *parent, int a, int b)
{
    for (;;) {
        a = uf_find<LDS>(parent, a);
        b = uf_find<LDS>(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + b, a);
        if (old == b) return;                             // b was a root and now hangs under a
        b = old;                                          // b had a parent already: that parent and a are still to be united
    }
}

// adds `count` of every lane with `active` to word[key] with one atomic per distinct key of the wave.  Called by all lanes of a wave
__device__ __forceinline__ void wave_add_by_key(int *word, bool active, int key)
{
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long todo = __ballot(active);
    while (todo) {                                        // (uniform; every pass retires at least the leader)
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const unsigned long long same = __ballot(active && key == k);
        if (lane == leader) atomicAdd(word + k, (int)__popcll(same));
        todo &= ~same;
    }
}

// exclusive prefix sum of x over the workgroup's 256 lanes, and the sum; s_w: one word per wave
__device__ __forceinline__ int block_scan(int x, int *s_w, int &total)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    int inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; w++) {
        const int c = s_w[w];
        if (w < wave) base += c;
        total += c;
    }
    __syncthreads();                                      // (s_w may be written again by the caller's next round)
    return base + inc - x;
}

}  // namespace haf
