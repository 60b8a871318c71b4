// grasp_lane.h -- what the two grasps x points kernels share (k_grasp_clear of clearance.hip, k_grasp_slab of opening.hip): the
// geometry of a workgroup -- grasps on LANES, 64 slots per workgroup, a tile of 256 points staged in LDS and walked in quarters by the four
// waves --, the staging of a tile, a lane's grasp and its near window.  Device code only.
#pragma once
#include "frame_group.h"
#include "kernels.h"

namespace haf {

constexpr int kClearThreads = 256;
constexpr int kClearWaves = kClearThreads / 64;
constexpr int kClearTile = 256;                           // points a workgroup stages
constexpr int kClearQuarter = kClearTile / kClearWaves;   // points a wave walks
constexpr int kClearSlots = 64;                           // grasps of a workgroup: one per lane of each wave
typedef int v4i __attribute__((ext_vector_type(4)));

// clear_near in two instructions per axis.  With lo = o - reach_q and span = 2 reach_q: |q - o| <= reach_q  <=>  0 <= q - lo <= span,
// and q - lo lies in (-2^18, 2^30 + 2^17) as an integer, so its unsigned word is <= span exactly when that holds (a negative one wraps
// above 2^31 > span).  A void grasp, and a lane without one, carries lo = INT32_MAX and span = 0: q - lo is 0 only for q = INT32_MAX,
// which no word is (|q| <= 2^30)
struct ClearWindow { unsigned lo[3], span; };

__device__ __forceinline__ bool clear_near_window(const ClearWindow &w, int x, int y, int z)
{
    return ((unsigned)x - w.lo[0] <= w.span) & ((unsigned)y - w.lo[1] <= w.span) & ((unsigned)z - w.lo[2] <= w.span);
}

// the tile of workgroup blockIdx.x: points base .. base + kClearTile - 1 of qx / qy / qz, a slot beyond n being the far word
__device__ __forceinline__ void stage_clear_tile(const ClearDev &d, int *s_x, int *s_y, int *s_z)
{
    using haf_clear_math::kClearFarWord;
    const unsigned n = (unsigned)d.f.n, base = blockIdx.x * (unsigned)kClearTile;
#pragma unroll
    for (int pass = 0; pass < kClearTile / kClearThreads; pass++) {
        const unsigned t = (unsigned)pass * kClearThreads + threadIdx.x, i = base + t;
        const bool in = i < n;
        s_x[t] = in ? d.qx[i] : kClearFarWord; s_y[t] = in ? d.qy[i] : 0; s_z[t] = in ? d.qz[i] : 0;
    }
}

// grasp k's words and its window; a lane that is not live (k >= n_grasps) reads grasp 0's words and carries reach_q = -1
__device__ __forceinline__ void load_grasp_lane(const ClearDev &d, unsigned k, bool live, haf_clear_math::GraspWords &g, ClearWindow &win)
{
    const global_ptr<const v4i> w = as_global<const v4i>(d.grasps + (size_t)(live ? k : 0u) * haf_clear_math::kClearGraspWords);
    const v4i w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    g.a[0] = w0.x; g.a[1] = w0.y; g.a[2] = w0.z; g.b[0] = w0.w; g.b[1] = w1.x; g.b[2] = w1.y; g.c[0] = w1.z; g.c[1] = w1.w;
    g.c[2] = w2.x; g.o[0] = w2.y; g.o[1] = w2.z; g.o[2] = w2.w;
    g.reach_q = live ? w3.x : -1;
    const bool valid = g.reach_q >= 0;
    win.span = valid ? 2u * (unsigned)g.reach_q : 0u;
#pragma unroll
    for (int j = 0; j < 3; j++) win.lo[j] = valid ? (unsigned)(g.o[j] - g.reach_q) : 0x7FFFFFFFu;
}

}  // namespace haf
