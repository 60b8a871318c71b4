// clearance.hip -- haf_check_grasps (include/hafgrasp.h): the scene's points inside the boxes of one parallel-jaw gripper placed at each of
// n_grasps poses.  The per-point rules are clearance_rules.h's, the same source haf_check_grasps_ref runs on the host, and all of it is
// int32 work whose result the definition fixes, so the two agree word for word (tests/test_clearance_gpu.py).
//
// Two launches on one stream, the second reading only what the first wrote:
//   1 k_clear_points<KIND>  a lane owns a GROUP of consecutive pixels (frame_group.h: eight of a U16 frame, four of an F32 or XYZ one,
//                           one 16-byte load where the group lies aligned inside a row), deprojects them and stores each pixel's three
//                           coordinate words as structure of arrays -- a whole group as aligned 16-byte stores.  An unusable or
//                           masked-out pixel is the word 2^30 in x, which fails the near test of every grasp by itself.
//   2 k_grasp_clear         the hot path, n_grasps x pixels box tests.  Grasps on LANES, as hypotheses are in k_plane_score: a lane
//                           keeps its grasp's twelve words, its reach and its eight accumulators in registers, the gripper's bounds
//                           are kernel arguments (scalar registers).  The workgroup stages a tile of 256 points in LDS; a workgroup
//                           serves 64 grasp slots (grid.y), and its four waves walk the four quarters of the tile for the SAME 64
//                           slots, so that 8 to 64 grasps still fill a workgroup.  The tile is small, 256 points: the loop is a chain
//                           of LDS reads and compares with nothing to overlap inside one wave, so a 640 x 480 frame is 1200
//                           workgroups, four to five waves per SIMD, and the waves hide one another's latency.  Every lane of a
//                           wave reads the tile at the same address -- a broadcast, four points per ds_read_b128, no bank conflict
//                           -- and nothing crosses lanes inside the loop.  The near test comes first, three subtractions and three
//                           unsigned compares (clear_near_window of grasp_lane.h); a wave whose ballot of near lanes is zero -- for four points at once, then per point -- skips the nine multiply-adds
//                           and the region tests: most points of a frame are far from most grasps.  At the end waves 1..3 hand their
//                           accumulators to wave 0 through LDS, and ONE set of integer atomics goes out per (workgroup, grasp), only
//                           where n_near > 0 and only for the words that are not empty.  The extremes travel in the zeroed rows as
//                           label_shape.h's words (a maximum x as shape_enc(x), a minimum as shape_enc(~x)): atomicMax on unsigned
//                           words whose zero is the empty value.  A void grasp, and a lane beyond n_grasps, carries reach_q = -1.
// The workgroup's geometry, the staging of a tile, a lane's grasp and its near window are grasp_lane.h's, which k_grasp_slab of opening.hip
// shares; k_clear_points is launched by that file too (launch_clear_points).
// No kernel waits for another workgroup; the rows are integer sums, minima and maxima, which do not depend on the order of arrival.
// Bounds: a pixel and its mask byte are loaded and its words stored only for i < n (a whole group has i0 + G <= n); the tile is staged
// from qx / qy / qz only for i < n, a slot beyond n being the far word; the LDS tile is indexed below kClearTile and the hand-over
// block below its 3 x 8 x 64 words; a grasp's words are loaded and its row updated only for k < n_grasps.
#include "grasp_lane.h"

namespace haf {

using namespace haf_clear_math;
using haf_shape_math::shape_enc;

template <int KIND>
__global__ __launch_bounds__(kFrameThreads) void k_clear_points(const ClearDev d)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned n = (unsigned)d.f.n, W = (unsigned)d.f.width;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;      // (n <= 2^28 and at most 2^11 pixels of slack: no wrap)
    if (i0 >= n) return;
    const bool whole = i0 + G <= n;
    float p[G * 3];
    group_points<KIND>(d.f, i0, n, p);
    int qx[G], qy[G], qz[G];
    unsigned v = i0 / W, u = i0 - v * W;
#pragma unroll
    for (unsigned k = 0; k < G; k++) {
        const bool admitted = i0 + k < n && (!d.mask || d.mask[(size_t)v * d.mask_stride + u] != 0);
        int32_t q[3];
        clear_point_words(p + 3 * k, admitted, q);
        qx[k] = q[0]; qy[k] = q[1]; qz[k] = q[2];
        if (++u == W) { u = 0; v++; }
    }
    if (whole) {                                          // (i0 is a multiple of G and the arrays are 16-byte aligned)
#pragma unroll
        for (unsigned j = 0; j < G / 4; j++) {
            as_global<v4i>(d.qx + i0)[j] = v4i{qx[4 * j], qx[4 * j + 1], qx[4 * j + 2], qx[4 * j + 3]};
            as_global<v4i>(d.qy + i0)[j] = v4i{qy[4 * j], qy[4 * j + 1], qy[4 * j + 2], qy[4 * j + 3]};
            as_global<v4i>(d.qz + i0)[j] = v4i{qz[4 * j], qz[4 * j + 1], qz[4 * j + 2], qz[4 * j + 3]};
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < G; k++)
            if (i0 + k < n) { d.qx[i0 + k] = qx[k]; d.qy[i0 + k] = qy[k]; d.qz[i0 + k] = qz[k]; }
    }
}

// a lane's accumulators: the row of clearance_rules.h with the extremes as plain int32 (INT32_MAX / INT32_MIN while empty)
struct ClearAcc { int near, f0, f1, palm, between, smin, smax, umax; };

__device__ __forceinline__ void clear_one(const ClearBounds &b, const GraspWords &g, const ClearWindow &w, int x, int y, int z, ClearAcc &a)
{
    const bool near = clear_near_window(w, x, y, z);
    if (__ballot(near) == 0) return;                      // (uniform)
    const int dx = x - g.o[0], dy = y - g.o[1], dz = z - g.o[2];
    const int s = clear_dot(g.c, dx, dy, dz), t = clear_dot(g.b, dx, dy, dz), u = clear_dot(g.a, dx, dy, dz);
    const int r = near ? clear_region(b, s, t, u) : CLEAR_REGION_NONE;
    a.near += near ? 1 : 0;
    a.f0 += r == CLEAR_REGION_FINGER0 ? 1 : 0;
    a.f1 += r == CLEAR_REGION_FINGER1 ? 1 : 0;
    a.palm += r == CLEAR_REGION_PALM ? 1 : 0;
    if (r == CLEAR_REGION_BETWEEN) {
        a.between++;
        a.smin = min(a.smin, s); a.smax = max(a.smax, s); a.umax = max(a.umax, u);
    }
}

__global__ __launch_bounds__(kClearThreads) void k_grasp_clear(const ClearDev d)
{
    __shared__ __attribute__((aligned(16))) int s_x[kClearTile];
    __shared__ __attribute__((aligned(16))) int s_y[kClearTile];
    __shared__ __attribute__((aligned(16))) int s_z[kClearTile];
    __shared__ int s_acc[kClearWaves - 1][kClearRowWords][kClearSlots];
    stage_clear_tile(d, s_x, s_y, s_z);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned k = blockIdx.y * (unsigned)kClearSlots + lane;
    const bool live = k < (unsigned)d.n_grasps;
    GraspWords g;
    ClearWindow win;
    load_grasp_lane(d, k, live, g, win);
    __syncthreads();
    ClearAcc a = {0, 0, 0, 0, 0, INT32_MAX, INT32_MIN, INT32_MIN};
    const v4i *x4 = reinterpret_cast<const v4i *>(s_x) + wave * (kClearQuarter / 4);
    const v4i *y4 = reinterpret_cast<const v4i *>(s_y) + wave * (kClearQuarter / 4);
    const v4i *z4 = reinterpret_cast<const v4i *>(s_z) + wave * (kClearQuarter / 4);
#pragma unroll 2
    for (int t = 0; t < kClearQuarter / 4; t++) {
        const v4i x = x4[t], y = y4[t], z = z4[t];
        const int any = (int)clear_near_window(win, x.x, y.x, z.x) | (int)clear_near_window(win, x.y, y.y, z.y) |
                        (int)clear_near_window(win, x.z, y.z, z.z) | (int)clear_near_window(win, x.w, y.w, z.w);
        if (__ballot(any != 0) == 0) continue;                 // (uniform)
        clear_one(d.b, g, win, x.x, y.x, z.x, a);
        clear_one(d.b, g, win, x.y, y.y, z.y, a);
        clear_one(d.b, g, win, x.z, y.z, z.z, a);
        clear_one(d.b, g, win, x.w, y.w, z.w, a);
    }
    if (wave) {
        int (*o)[kClearSlots] = s_acc[wave - 1];
        o[CLEAR_NEAR][lane] = a.near; o[CLEAR_FINGER0][lane] = a.f0; o[CLEAR_FINGER1][lane] = a.f1; o[CLEAR_PALM][lane] = a.palm;
        o[CLEAR_BETWEEN][lane] = a.between; o[CLEAR_SMIN][lane] = a.smin; o[CLEAR_SMAX][lane] = a.smax; o[CLEAR_UMAX][lane] = a.umax;
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 0; w < kClearWaves - 1; w++) {
        const int (*o)[kClearSlots] = s_acc[w];
        a.near += o[CLEAR_NEAR][lane]; a.f0 += o[CLEAR_FINGER0][lane]; a.f1 += o[CLEAR_FINGER1][lane]; a.palm += o[CLEAR_PALM][lane];
        a.between += o[CLEAR_BETWEEN][lane];
        a.smin = min(a.smin, o[CLEAR_SMIN][lane]); a.smax = max(a.smax, o[CLEAR_SMAX][lane]); a.umax = max(a.umax, o[CLEAR_UMAX][lane]);
    }
    if (!live || a.near == 0) return;
    unsigned *row = d.rows + (size_t)k * kClearRowWords;
    atomicAdd(row + CLEAR_NEAR, (unsigned)a.near);
    if (a.f0) atomicAdd(row + CLEAR_FINGER0, (unsigned)a.f0);
    if (a.f1) atomicAdd(row + CLEAR_FINGER1, (unsigned)a.f1);
    if (a.palm) atomicAdd(row + CLEAR_PALM, (unsigned)a.palm);
    if (a.between) {
        atomicAdd(row + CLEAR_BETWEEN, (unsigned)a.between);
        atomicMax(row + CLEAR_SMIN, shape_enc(~a.smin));
        atomicMax(row + CLEAR_SMAX, shape_enc(a.smax));
        atomicMax(row + CLEAR_UMAX, shape_enc(a.umax));
    }
}

void launch_clear_points(const ClearDev &d, hipStream_t s)
{
    const unsigned n = (unsigned)d.f.n;
    with_frame_kind(d.f.kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        const unsigned groups = (n + frame_group<KIND>() - 1) / frame_group<KIND>();
        hipLaunchKernelGGL(k_clear_points<KIND>, dim3((groups + kFrameThreads - 1) / kFrameThreads), dim3(kFrameThreads), 0, s, d);
    });
}

void launch_clearance(const ClearDev &d, hipStream_t s)
{
    const unsigned n = (unsigned)d.f.n;                   // (n <= 2^28: at most 2^20 tiles)
    launch_clear_points(d, s);
    const unsigned tiles = (n + kClearTile - 1) / kClearTile, slots = ((unsigned)d.n_grasps + kClearSlots - 1) / kClearSlots;
    hipLaunchKernelGGL(k_grasp_clear, dim3(tiles, slots), dim3(kClearThreads), 0, s, d);
}

}  // namespace haf
