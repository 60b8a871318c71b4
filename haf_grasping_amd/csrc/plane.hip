// plane.hip -- haf_fit_plane (include/hafgrasp.h): the dominant plane of one sensor frame by a fixed set of three-point hypotheses.  The
// per-point and per-hypothesis rules are plane_rules.h's, the same source haf_fit_plane_ref runs on the host; all the rest is integer work
// whose result the definition fixes, so the two agree word for word (tests/test_plane_gpu.py).
//
// Five launches on one stream, each reading only what an EARLIER launch wrote or what reaches it through integer atomics:
//   1 k_plane_points<KIND>  one workgroup of 256 lanes per block of 1024 pixels.  Deprojects the pixels, writes every point -- an unusable
//                           or masked-out one as three NaNs -- the usable pixels as one ballot word per 64 pixels, and the block's usable
//                           count (popcounts, no atomics).
//   2 k_plane_scan          one workgroup: exclusive prefix sum of the block counts, their sum -> counters[0] = n_usable.
//   3 k_plane_hyp           one lane per hypothesis: its three ranks -> the block by binary search in the prefix sums (staged in LDS:
//                           the kernel is a handful of waves and all latency), the pixel inside the block by popcounts over its
//                           sixteen ballot words; the hypothesis' four words and its threshold tol2 * nn (a NaN when it is void).
//   4 k_plane_score         the hot path, n_hyp x pixels point-plane tests.  Hypotheses on LANES: a lane keeps its hypothesis in
//                           registers, the workgroup stages its tile of 512 points in LDS and every lane walks them at the same
//                           address -- a broadcast read, no bank conflict, no cross-lane reduction.  One integer atomicAdd per
//                           (workgroup, hypothesis) at the end.  An unusable point is three NaNs and fails `<=` by itself; so does every point
//                           against a void hypothesis' NaN threshold.
//   5 k_plane_moments       every workgroup finds the winner itself from the counts (largest count, ties to the lowest k: the maximum
//                           of (count << 32 | ~k)), tests its 1024 points against it and adds the ten int64 moments of its inliers with
//                           ten 64-bit integer atomicAdds.
// No kernel waits for another workgroup; counts and moments are integer sums, which do not depend on the order of arrival.
// Bounds: a pixel is loaded and a point stored only for i < n; the ballot words of a block are all written (zero beyond the image), so
// the words and prefix entries of plane_blocks(n) blocks are; a rank is < n_usable, so the block search ends inside a block that holds
// the pixel, and a set bit only stands for a pixel inside the image; k indexes hyps, thr and counts only below n_hyp.
#include "frame_group.h"
#include "kernels.h"

namespace haf {

using namespace haf_plane_math;

constexpr int kPlaneThreads = 256;
constexpr int kPlanePasses = kPlaneBlockPixels / kPlaneThreads;           // 4: pixel = block * 1024 + pass * 256 + thread
constexpr int kPlaneBlockWords = kPlaneBlockPixels / 64;                  // 16 ballot words per block
constexpr int kPlaneHypThreads = 64;
constexpr int kPlaneLdsBlocks = 4096;                                     // k_plane_hyp: prefix words it stages in LDS (16 KB)
constexpr int kPlaneScoreTile = 512;                                      // k_plane_score: points a workgroup stages and walks

template <int KIND>
__global__ __launch_bounds__(kPlaneThreads) void k_plane_points(const PlaneDev d)
{
    __shared__ unsigned s_cnt[kPlaneThreads / 64];
    const unsigned n = (unsigned)d.f.n, W = (unsigned)d.f.width;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned cnt = 0;                                     // the wave's total (uniform)
#pragma unroll
    for (int pass = 0; pass < kPlanePasses; pass++) {
        const unsigned i = blockIdx.x * (unsigned)kPlaneBlockPixels + (unsigned)pass * kPlaneThreads + threadIdx.x;   // (n <= 2^28: no wrap)
        bool ok = false;
        if (i < n) {
            const unsigned v = i / W, u = i - v * W;
            float p[3];
            pixel_point<KIND>(d.f, (int)u, (int)v, p);
            ok = point_usable(p) && (!d.mask || d.mask[(size_t)v * d.mask_stride + u] != 0);
            const float bad = __uint_as_float(kInvalidWord);
            d.x[i] = ok ? p[0] : bad; d.y[i] = ok ? p[1] : bad; d.z[i] = ok ? p[2] : bad;
        }
        const unsigned long long word = __ballot(ok);
        if (lane == 0) d.bits[(size_t)blockIdx.x * kPlaneBlockWords + (unsigned)pass * (kPlaneThreads / 64) + wave] = word;
        cnt += (unsigned)__popcll(word);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kPlaneThreads / 64; w++) total += s_cnt[w];
        d.prefix[blockIdx.x] = (int)total;
    }
}

// exclusive prefix sum of x over the workgroup's 256 lanes, and the sum; s_w: one word per wave
__device__ __forceinline__ int plane_block_scan(int x, int *s_w, int &total)
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
    for (int w = 0; w < kPlaneThreads / 64; w++) {
        const int c = s_w[w];
        if (w < wave) base += c;
        total += c;
    }
    __syncthreads();                                      // (s_w is written again by the next round)
    return base + inc - x;
}

__global__ __launch_bounds__(kPlaneThreads) void k_plane_scan(const PlaneDev d, int n_blocks)
{
    __shared__ int s_w[kPlaneThreads / 64];
    int carry = 0;
    for (int c0 = 0; c0 < n_blocks; c0 += kPlaneThreads) {   // (uniform)
        const int i = c0 + (int)threadIdx.x;
        const int x = i < n_blocks ? d.prefix[i] : 0;
        int total;
        const int ex = plane_block_scan(x, s_w, total);
        if (i < n_blocks) d.prefix[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) d.counters[0] = (unsigned)carry;
}

// the pixel of rank `rank` < n_usable: the last block whose prefix is <= rank holds it (an empty block shares its prefix with the next
// one, which is later), then the word inside the block, then the bit inside the word.  prefix: d.prefix, or its copy in LDS.  The
// sixteen words are loaded at once -- their addresses do not depend on one another -- and the walk over them is arithmetic
__device__ __forceinline__ unsigned plane_pixel_of_rank(const PlaneDev &d, const int *prefix, int n_blocks, unsigned rank)
{
    int lo = 0, hi = n_blocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((unsigned)prefix[mid] <= rank) lo = mid; else hi = mid - 1;
    }
    unsigned rem = rank - (unsigned)prefix[lo];
    const unsigned long long *words = d.bits + (size_t)lo * kPlaneBlockWords;
    unsigned long long w[kPlaneBlockWords];
#pragma unroll
    for (int j = 0; j < kPlaneBlockWords; j++) w[j] = words[j];
    unsigned long long word = 0;
    unsigned at = 0;
    bool hit = false;
#pragma unroll
    for (int j = 0; j < kPlaneBlockWords; j++) {
        const unsigned c = (unsigned)__popcll(w[j]);
        const bool here = !hit && rem < c;
        if (here) { word = w[j]; at = (unsigned)j; hit = true; }
        if (!hit) rem -= c;
    }
    if (!hit) return 0;                                   // (not reached: the block holds more than rem usable pixels)
    for (; rem; rem--) word &= word - 1;                  // (rem < 64)
    return (unsigned)lo * kPlaneBlockPixels + at * 64u + (unsigned)(__ffsll((long long)word) - 1);
}

__global__ __launch_bounds__(kPlaneHypThreads) void k_plane_hyp(const PlaneDev d, int n_blocks)
{
    __shared__ int s_prefix[kPlaneLdsBlocks];             // the block prefixes of frames up to 4 M pixels: the searches' loads stay in the CU
    const unsigned k = blockIdx.x * (unsigned)kPlaneHypThreads + threadIdx.x;
    const unsigned nu = d.counters[0];
    const bool staged = n_blocks <= kPlaneLdsBlocks;      // (uniform)
    if (staged) {
        for (int b = (int)threadIdx.x; b < n_blocks; b += kPlaneHypThreads) s_prefix[b] = d.prefix[b];
        __syncthreads();
    }
    const int *prefix = staged ? s_prefix : d.prefix;
    bool live = false;
    if (k < (unsigned)d.r.n_hyp) {
        PlaneHyp h;
        h.n[0] = h.n[1] = h.n[2] = h.d = h.thr = __uint_as_float(kInvalidWord);
        if (nu) {
            unsigned rk[3];
            float p[9];
#pragma unroll
            for (unsigned j = 0; j < 3; j++) {
                rk[j] = sample_rank(d.r.seed, k, j, nu);
                const unsigned i = plane_pixel_of_rank(d, prefix, n_blocks, rk[j]);
                p[3 * j] = d.x[i]; p[3 * j + 1] = d.y[i]; p[3 * j + 2] = d.z[i];
            }
            live = !make_hypothesis(p, p + 3, p + 6, rk[0] == rk[1] || rk[0] == rk[2] || rk[1] == rk[2], d.r, h);
        }
        float *o = d.hyps + 4 * (size_t)k;
        o[0] = h.n[0]; o[1] = h.n[1]; o[2] = h.n[2]; o[3] = h.d;
        d.thr[k] = h.thr;
    }
    const unsigned n_live = (unsigned)__popcll(__ballot(live));
    if (threadIdx.x == 0 && n_live) atomicAdd(d.counters + 1, n_live);
}

__global__ __launch_bounds__(kPlaneThreads) void k_plane_score(const PlaneDev d)
{
    __shared__ float s_x[kPlaneScoreTile], s_y[kPlaneScoreTile], s_z[kPlaneScoreTile];
    const unsigned n = (unsigned)d.f.n, base = blockIdx.x * (unsigned)kPlaneScoreTile;
#pragma unroll
    for (int pass = 0; pass < kPlaneScoreTile / kPlaneThreads; pass++) {
        const unsigned t = (unsigned)pass * kPlaneThreads + threadIdx.x, i = base + t;
        const float bad = __uint_as_float(kInvalidWord);
        s_x[t] = i < n ? d.x[i] : bad; s_y[t] = i < n ? d.y[i] : bad; s_z[t] = i < n ? d.z[i] : bad;
    }
    __syncthreads();
    const unsigned k = blockIdx.y * (unsigned)kPlaneThreads + threadIdx.x;
    if (k >= (unsigned)d.r.n_hyp) return;
    PlaneHyp h;
    const float *w = d.hyps + 4 * (size_t)k;
    h.n[0] = w[0]; h.n[1] = w[1]; h.n[2] = w[2]; h.d = w[3]; h.thr = d.thr[k];
    int c = 0;
#pragma unroll 8
    for (int t = 0; t < kPlaneScoreTile; t++) c += inlier(h, s_x[t], s_y[t], s_z[t]) ? 1 : 0;
    if (c) atomicAdd(d.counts + k, c);
}

__global__ __launch_bounds__(kPlaneThreads) void k_plane_moments(const PlaneDev d)
{
    __shared__ unsigned long long s_key[kPlaneThreads / 64];
    __shared__ long long s_m[kPlaneThreads / 64][kPlaneMoments];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long key = 0;
    for (unsigned k = threadIdx.x; k < (unsigned)d.r.n_hyp; k += kPlaneThreads) {
        const unsigned long long kk = ((unsigned long long)(unsigned)d.counts[k] << 32) | (unsigned long long)(0xFFFFFFFFu - k);
        key = kk > key ? kk : key;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kPlaneThreads / 64; w++) key = s_key[w] > key ? s_key[w] : key;
    if ((key >> 32) == 0) return;                         // (uniform: no hypothesis has an inlier, the moments stay zero)
    const unsigned win = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);      // (a key that counts something came from a k < n_hyp)
    PlaneHyp h;
    const float *hw = d.hyps + 4 * (size_t)win;
    h.n[0] = hw[0]; h.n[1] = hw[1]; h.n[2] = hw[2]; h.d = hw[3]; h.thr = d.thr[win];
    const unsigned n = (unsigned)d.f.n;
    long long m[kPlaneMoments] = {};
#pragma unroll
    for (int pass = 0; pass < kPlanePasses; pass++) {
        const unsigned i = blockIdx.x * (unsigned)kPlaneBlockPixels + (unsigned)pass * kPlaneThreads + threadIdx.x;
        if (i >= n) continue;
        const float x = d.x[i], y = d.y[i], z = d.z[i];
        if (inlier(h, x, y, z)) add_moments(m, x, y, z);
    }
#pragma unroll
    for (int j = 0; j < kPlaneMoments; j++) {
#pragma unroll
        for (int off = 32; off; off >>= 1) m[j] += __shfl_xor(m[j], off);
        if (lane == 0) s_m[wave][j] = m[j];
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)kPlaneMoments) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < kPlaneThreads / 64; w++) sum += s_m[w][threadIdx.x];
        if (sum) atomicAdd(d.moments + threadIdx.x, (unsigned long long)sum);      // (two's complement: a negative sum wraps to the right word)
    }
}

void launch_plane(const PlaneDev &d, hipStream_t s)
{
    const unsigned blocks = (unsigned)plane_blocks((size_t)d.f.n);       // (n <= 2^28: at most 2^18 blocks)
    const unsigned n_hyp = (unsigned)d.r.n_hyp;
    const unsigned tiles = ((unsigned)d.f.n + kPlaneScoreTile - 1) / kPlaneScoreTile;
    if (d.f.kind == HAF_FRAME_DEPTH_U16) hipLaunchKernelGGL((k_plane_points<HAF_FRAME_DEPTH_U16>), dim3(blocks), dim3(kPlaneThreads), 0, s, d);
    else if (d.f.kind == HAF_FRAME_DEPTH_F32) hipLaunchKernelGGL((k_plane_points<HAF_FRAME_DEPTH_F32>), dim3(blocks), dim3(kPlaneThreads), 0, s, d);
    else hipLaunchKernelGGL((k_plane_points<HAF_FRAME_XYZ_F32>), dim3(blocks), dim3(kPlaneThreads), 0, s, d);
    hipLaunchKernelGGL(k_plane_scan, dim3(1), dim3(kPlaneThreads), 0, s, d, (int)blocks);
    hipLaunchKernelGGL(k_plane_hyp, dim3((n_hyp + kPlaneHypThreads - 1) / kPlaneHypThreads), dim3(kPlaneHypThreads), 0, s, d, (int)blocks);
    hipLaunchKernelGGL(k_plane_score, dim3(tiles, (n_hyp + kPlaneThreads - 1) / kPlaneThreads), dim3(kPlaneThreads), 0, s, d);
    hipLaunchKernelGGL(k_plane_moments, dim3(blocks), dim3(kPlaneThreads), 0, s, d);
}

}  // namespace haf
