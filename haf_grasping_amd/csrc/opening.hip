// opening.hip -- haf_fit_openings (include/hafgrasp.h): per grasp pose the smallest free opening of one parallel-jaw gripper and the
// sideways shift that goes with it.  The rules are opening_rules.h's on top of clearance_rules.h's, the same source
// haf_fit_openings_ref runs on the host, and all of it is int32 work whose result the definition fixes, so the two agree word for word
// (tests/test_opening_gpu.py).
//
// Three launches on one stream, each reading only what the one before wrote:
//   1 k_clear_points<KIND>  clearance.hip's, as it is (launch_clear_points): every pixel's three coordinate words.
//   2 k_grasp_slab          the hot path, n_grasps x pixels.  k_grasp_clear's shape (grasp_lane.h): grasps on LANES, a tile of 256 points
//                           broadcast from LDS, the four waves on its four quarters for the SAME 64 slots, the windowed near test with
//                           the ballot skip in front of the nine multiply-adds.  What differs is the accumulator: not eight registers
//                           but a histogram of s per grasp, kept per workgroup in LDS as [128 bins][64 lanes] words.  A point lies in at
//                           most one slab (u < U1 against u >= U1) and a tile holds 256 points, so both slabs share one 32-bit word --
//                           the finger slab's count in the low half, the palm slab's in the high half, neither above 256 -- 32 KB,
//                           updated by LDS atomic adds (the four waves serve the same slots, so a word has four writers).  Lane l's
//                           column is bin * 64 + l: the lanes of an add lie on distinct banks whatever their bins.  The workgroup zeroes
//                           the histogram while the tile is staged, and flushes it only when one of its lanes counted a point -- most
//                           tiles of a frame are far from every grasp --, reading it 16 bytes at a time and sending only the non-zero
//                           words out, unpacked, as global integer atomics into the grasp's two histograms.  35 KB of LDS per
//                           workgroup: four workgroups, sixteen waves per CU by LDS (the build's figures are in DESIGN.md 5).
//   3 k_open_search         one wave per grasp, four per workgroup.  A lane loads two words of each histogram; a wave scan (shuffles)
//                           makes the prefix sums, which go to LDS; the lanes walk the placements in the order of the search, lane l
//                           taking p = l, l + 64, ..: a lane stops at its first free one, and the wave's minimum over p is THE first
//                           (p runs over j ascending, |c| ascending, c ascending: open_placement).  The first free j at c = 0 the same
//                           way, lane l testing j_min + l (j_max - j_min < 63).  Lane 0 writes the row; a void grasp's is found = -1.
// No kernel waits for another workgroup; the histograms are integer sums, which do not depend on the order of arrival.
// Bounds: the tile is staged from qx / qy / qz only for i < n, a slot beyond n being the far word, and indexed below kClearTile; an LDS
// histogram word is (bin + 64) * 64 + lane with -half_bins <= bin < half_bins, half_bins <= 64 (opening_rules.h), so below 8192; a
// grasp's words are loaded, its histograms updated and read and its row written only for k < n_grasps, a histogram word being
// (2 k + slab) * 128 + bin + 64 < 256 n_grasps; the prefix arrays are indexed 64 + lo .. 64 + hi with -64 < lo <= hi < 64
// (opening_rules.h has the proof), inside their 129 words.
#include "grasp_lane.h"

namespace haf {

using namespace haf_open_math;

constexpr int kSlabWords = kOpenBins * kClearSlots;       // the LDS histogram of a workgroup
constexpr unsigned kSlabPalmOne = 1u << 16;               // a palm-slab point in a packed word
constexpr int kSearchWaves = 4;                           // grasps of a search workgroup
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool slab_one(const OpenRules &r, const GraspWords &g, const ClearWindow &w, int x, int y, int z, unsigned *column)
{
    const bool near = clear_near_window(w, x, y, z);
    if (__ballot(near) == 0) return false;                // (uniform)
    const int dx = x - g.o[0], dy = y - g.o[1], dz = z - g.o[2];
    const int s = clear_dot(g.c, dx, dy, dz), t = clear_dot(g.b, dx, dy, dz), u = clear_dot(g.a, dx, dy, dz);
    const int slab = near ? open_slab(r, t, u) : OPEN_SLAB_NONE;
    const int bin = open_bin(s, r.shift);
    const bool counted = slab != OPEN_SLAB_NONE && open_bin_counted(r, bin);
    if (counted) atomicAdd(column + (bin + kOpenZero) * kClearSlots, slab == OPEN_SLAB_PALM ? kSlabPalmOne : 1u);
    return counted;
}

__global__ __launch_bounds__(kClearThreads) void k_grasp_slab(const OpenDev d)
{
    __shared__ __attribute__((aligned(16))) int s_x[kClearTile];
    __shared__ __attribute__((aligned(16))) int s_y[kClearTile];
    __shared__ __attribute__((aligned(16))) int s_z[kClearTile];
    __shared__ __attribute__((aligned(16))) unsigned s_hist[kSlabWords];
    __shared__ unsigned s_any;
    stage_clear_tile(d.c, s_x, s_y, s_z);
    v4u32 *const h4 = reinterpret_cast<v4u32 *>(s_hist);
#pragma unroll
    for (int i = 0; i < kSlabWords / 4 / kClearThreads; i++) h4[i * kClearThreads + threadIdx.x] = v4u32{0u, 0u, 0u, 0u};
    if (threadIdx.x == 0) s_any = 0u;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned k = blockIdx.y * (unsigned)kClearSlots + lane;
    const bool live = k < (unsigned)d.c.n_grasps;
    GraspWords g;
    ClearWindow win;
    load_grasp_lane(d.c, k, live, g, win);
    __syncthreads();
    bool hit = false;
    unsigned *const column = s_hist + lane;
    const v4i *x4 = reinterpret_cast<const v4i *>(s_x) + wave * (kClearQuarter / 4);
    const v4i *y4 = reinterpret_cast<const v4i *>(s_y) + wave * (kClearQuarter / 4);
    const v4i *z4 = reinterpret_cast<const v4i *>(s_z) + wave * (kClearQuarter / 4);
#pragma unroll 2
    for (int t = 0; t < kClearQuarter / 4; t++) {
        const v4i x = x4[t], y = y4[t], z = z4[t];
        const int any = (int)clear_near_window(win, x.x, y.x, z.x) | (int)clear_near_window(win, x.y, y.y, z.y) |
                        (int)clear_near_window(win, x.z, y.z, z.z) | (int)clear_near_window(win, x.w, y.w, z.w);
        if (__ballot(any != 0) == 0) continue;                 // (uniform)
        hit |= slab_one(d.r, g, win, x.x, y.x, z.x, column);
        hit |= slab_one(d.r, g, win, x.y, y.y, z.y, column);
        hit |= slab_one(d.r, g, win, x.z, y.z, z.z, column);
        hit |= slab_one(d.r, g, win, x.w, y.w, z.w, column);
    }
    if (__ballot(hit) != 0 && lane == 0) s_any = 1u;      // (up to four writers of the same value)
    __syncthreads();
    if (s_any == 0u) return;                              // (uniform)
    // a thread reads four words of one bin: lanes l0 .. l0 + 3
#pragma unroll
    for (int i = 0; i < kSlabWords / 4 / kClearThreads; i++) {
        const unsigned q = (unsigned)i * kClearThreads + threadIdx.x, bin = q / (kClearSlots / 4), l0 = (q % (kClearSlots / 4)) * 4;
        const v4u32 w = h4[q];
        if ((w.x | w.y | w.z | w.w) == 0u) continue;
        const unsigned word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const unsigned kk = blockIdx.y * (unsigned)kClearSlots + l0 + (unsigned)e;
            if (word[e] == 0u || kk >= (unsigned)d.c.n_grasps) continue;
            unsigned *const h = d.hist + (size_t)kk * 2 * kOpenBins + bin;
            if (word[e] & 0xFFFFu) atomicAdd(h, word[e] & 0xFFFFu);
            if (word[e] >> 16) atomicAdd(h + kOpenBins, word[e] >> 16);
        }
    }
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(kSearchWaves * 64) void k_open_search(const OpenDev d)
{
    __shared__ unsigned s_pf[kSearchWaves][kOpenBins + 1];
    __shared__ unsigned s_pp[kSearchWaves][kOpenBins + 1];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned k = blockIdx.x * (unsigned)kSearchWaves + wave;
    const bool live = k < (unsigned)d.c.n_grasps;
    const unsigned *const h = d.hist + (size_t)(live ? k : 0u) * 2 * kOpenBins;
    const unsigned f0 = h[2 * lane], f1 = h[2 * lane + 1], p0 = h[kOpenBins + 2 * lane], p1 = h[kOpenBins + 2 * lane + 1];
    unsigned fs = f0 + f1, ps = p0 + p1;                  // -> the sums over the lanes up to and including this one
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned a = __shfl_up(fs, o), b = __shfl_up(ps, o);
        if (lane >= (unsigned)o) { fs += a; ps += b; }
    }
    unsigned *const pf = s_pf[wave], *const pp = s_pp[wave];
    if (lane == 0) pf[0] = pp[0] = 0u;
    pf[2 * lane + 1] = fs - f1; pf[2 * lane + 2] = fs;
    pp[2 * lane + 1] = ps - p1; pp[2 * lane + 2] = ps;
    __syncthreads();
    if (!live) return;                                    // (a whole wave; no barrier follows)
    int counts[kOpenRowWords];
    int best = INT32_MAX;
    for (int p = (int)lane, n = open_placements(d.r); p < n; p += 64) {
        int j, c;
        open_placement(d.r, p, &j, &c);
        if (open_counts(d.r, pf, pp, j, c, counts)) { best = p; break; }
    }
    best = wave_min(best);
    const int js = d.r.j_min + (int)lane;
    const int sym = wave_min(js <= d.r.j_max && open_counts(d.r, pf, pp, js, 0, counts) ? js : INT32_MAX);
    if (lane != 0) return;
    int row[kOpenRowWords] = {0};
    if (d.c.grasps[(size_t)k * kClearGraspWords + 12] < 0) {      // (GraspWords::reach_q: a void grasp)
        row[OPEN_FOUND] = -1;
    } else {
        row[OPEN_FINGER_SLAB] = (int)pf[kOpenBins]; row[OPEN_PALM_SLAB] = (int)pp[kOpenBins];
        if (best != INT32_MAX) {
            int j, c;
            open_placement(d.r, best, &j, &c);
            open_counts(d.r, pf, pp, j, c, row);
            row[OPEN_FOUND] = 1; row[OPEN_J] = j; row[OPEN_C] = c;
        }
        row[OPEN_SYM_J] = sym != INT32_MAX ? sym : 0;
    }
    v4i *const out = reinterpret_cast<v4i *>(d.rows + (size_t)k * kOpenRowWords);
#pragma unroll
    for (int i = 0; i < kOpenRowWords / 4; i++) out[i] = v4i{row[4 * i], row[4 * i + 1], row[4 * i + 2], row[4 * i + 3]};
}

void launch_openings(const OpenDev &d, hipStream_t s)
{
    const unsigned n = (unsigned)d.c.f.n, K = (unsigned)d.c.n_grasps;      // (n <= 2^28: at most 2^20 tiles)
    launch_clear_points(d.c, s);
    const unsigned tiles = (n + kClearTile - 1) / kClearTile, slots = (K + kClearSlots - 1) / kClearSlots;
    hipLaunchKernelGGL(k_grasp_slab, dim3(tiles, slots), dim3(kClearThreads), 0, s, d);
    hipLaunchKernelGGL(k_open_search, dim3((K + kSearchWaves - 1) / kSearchWaves), dim3(kSearchWaves * 64), 0, s, d);
}

}  // namespace haf
