// topgrasps.hip -- k_top_grasps: the ranked grasp candidates of haf_top_grasps (engine_topgrasps.cpp) on the vote grids of the last
// scored batch.  For every (cloud, roll): the maximal horizontal runs of equal vote v >= min_vote, each at the reference's run centre
// (row, end - len/2; server.cpp:904-932), in the order vote desc, len desc, row asc, col asc, and the first D entries of the roll's
// greedy sequence under in-roll Chebyshev suppression, with the 9x8 z window of k_vote_record for each kept entry.
//
// One workgroup per (cloud, roll) slot; a slot owns 2 x H*W 64-bit words of scratch (two run lists for the sort's ping-pong), so a
// grid of any size the engine accepts fits: a row holds at most W-8 scoring runs.  Everything is ordered by construction -- the run
// list by row-major emission through per-row counts and a scan, the sort by a stable LSD radix pass per 8-bit digit -- so the result
// does not depend on scheduling.
#include "device_common.h"

namespace haf {

constexpr int kTopThreads = 1024, kTopWaves = kTopThreads / 64;
constexpr int kTopMaxRows = 4096;        // grid_h <= 4096 (haf_create)
constexpr int kTopKeptLds = 4096;        // kept centres held in LDS; beyond that the kernel reads them back from its own output
constexpr int kTopNoVote = -65536;       // outside the grid (no short vote equals it)

// run list entry: high word the sort key ((top - vote) << lbits | (W - len)), low word (row << 16) | centre column
__device__ __forceinline__ unsigned long long top_pack(unsigned key, int row, int col)
{
    return ((unsigned long long)key << 32) | ((unsigned)row << 16) | (unsigned)col;
}

// the runs of one grid row, 64 columns at a time: a run starts where the vote differs from its left neighbour and ends where it
// differs from its right one; the start of the run an end lane closes is the highest start bit at or below the lane (or the carry of
// the previous piece).  emit(mask of the lanes that end a scoring run, this lane ends one, vote, length, end column) per piece.
template <class F>
__device__ __forceinline__ void top_row_runs(const short *__restrict__ er, int W, int min_vote, int lane, F &&emit)
{
    int carry = 0;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < W;
        const int v = in ? (int)er[c] : kTopNoVote;
        int left = __shfl_up(v, 1, 64), right = __shfl_down(v, 1, 64);
        if (lane == 0) left = c0 > 0 ? (int)er[c0 - 1] : kTopNoVote;
        if (lane == 63) right = c + 1 < W ? (int)er[c + 1] : kTopNoVote;
        const unsigned long long sm = __ballot(in && v != left);
        const unsigned long long upto = sm & ((2ull << lane) - 1ull);      // (lane 63: 2 << 63 wraps to 0, the mask is all ones)
        const int start = upto ? c0 + 63 - __clzll((long long)upto) : carry;
        const bool em = in && v != right && v >= min_vote;
        const unsigned long long emask = __ballot(em);
        emit(emask, em, v, c - start + 1, c);
        if (sm) carry = c0 + 63 - __clzll((long long)sm);
    }
}

__device__ __forceinline__ int top_cheb(int r0, int c0, int r1, int c1) { return max(abs(r0 - r1), abs(c0 - c1)); }

__global__ __launch_bounds__(kTopThreads) void k_top_grasps(const short *__restrict__ ev16, const float *__restrict__ heights,
                                                            const RollRecordDev *__restrict__ rec, unsigned long long *__restrict__ scratch,
                                                            size_t slot_words, int *__restrict__ hdr, TopCandDev *__restrict__ cand, int D,
                                                            int min_vote, int radius, Dims d)
{
    __shared__ int s_row[kTopMaxRows];
    __shared__ int s_hist[kTopWaves][256];
    __shared__ int s_tot[256];
    __shared__ int s_kept[kTopKeptLds];
    __shared__ unsigned char s_ok[kTopThreads];
    __shared__ int s_n, s_nk, s_last;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int H = d.H, W = d.W, BR = d.B * d.R;
    const size_t HW = (size_t)H * W;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int br = blockIdx.x; br < BR; br += gridDim.x) {
        const int top = rec[br].vote;
        if (top < min_vote) {                                    // (uniform across the workgroup) no run reaches min_vote
            if (t == 0) { hdr[4 * br] = 0; hdr[4 * br + 1] = 0; hdr[4 * br + 2] = rec[br].n_evals; hdr[4 * br + 3] = top; }
            continue;
        }
        const short *ev = ev16 + (size_t)br * HW;
        unsigned long long *src = scratch + (size_t)blockIdx.x * 2 * slot_words, *dst = src + slot_words;
        const int lbits = 32 - __clz(W), vbits = 32 - __clz(top - min_vote);
        auto key_of = [&](int v, int len) { return ((unsigned)(top - v) << lbits) | (unsigned)(W - len); };

        // ---- runs: per-row counts, exclusive scan, row-major emission ----
        for (int row = wave; row < H; row += kTopWaves) {
            int cnt = 0;
            top_row_runs(ev + (size_t)row * W, W, min_vote, lane, [&](unsigned long long m, bool, int, int, int) { cnt += __popcll(m); });
            if (lane == 0) s_row[row] = cnt;
        }
        __syncthreads();
        if (wave == 0) {
            const int per = (H + 63) / 64, lo = min(H, lane * per), hi = min(H, lo + per);
            int sum = 0;
            for (int r = lo; r < hi; r++) sum += s_row[r];
            int inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
            int run = inc - sum;
            for (int r = lo; r < hi; r++) { const int c = s_row[r]; s_row[r] = run; run += c; }
            if (lane == 63) s_n = inc;
        }
        __syncthreads();
        const int N = s_n;
        for (int row = wave; row < H; row += kTopWaves) {
            int done = s_row[row];
            top_row_runs(ev + (size_t)row * W, W, min_vote, lane, [&](unsigned long long m, bool em, int v, int len, int end) {
                if (em) src[done + __popcll(m & lt)] = top_pack(key_of(v, len), row, end - len / 2);
                done += __popcll(m);
            });
        }
        __syncthreads();

        // ---- stable LSD radix sort on the key, 8 bits per pass: every wave owns a contiguous segment and its own digit cursors ----
        const int passes = (lbits + vbits + 7) / 8;
        const int seg = (N + kTopWaves - 1) / kTopWaves, slo = min(N, wave * seg), shi = min(N, slo + seg);
        for (int p = 0; p < passes; p++) {
            const int sh = 32 + 8 * p;
            for (int k = t; k < kTopWaves * 256; k += kTopThreads) (&s_hist[0][0])[k] = 0;
            __syncthreads();
            for (int i = slo + lane; i < shi; i += 64) atomicAdd(&s_hist[wave][(int)(src[i] >> sh) & 255], 1);
            __syncthreads();
            if (t < 256) {
                int s = 0;
                for (int w = 0; w < kTopWaves; w++) s += s_hist[w][t];
                s_tot[t] = s;
            }
            __syncthreads();
            if (wave == 0) {                                     // exclusive scan of the 256 digit totals, four per lane
                int a[4], sum = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) { a[k] = s_tot[4 * lane + k]; sum += a[k]; }
                int inc = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
                int run = inc - sum;
#pragma unroll
                for (int k = 0; k < 4; k++) { s_tot[4 * lane + k] = run; run += a[k]; }
            }
            __syncthreads();
            if (t < 256) {
                int run = s_tot[t];
                for (int w = 0; w < kTopWaves; w++) { const int h = s_hist[w][t]; s_hist[w][t] = run; run += h; }
            }
            __syncthreads();
            for (int i0 = slo; i0 < shi; i0 += 64) {
                const int i = i0 + lane;
                const bool valid = i < shi;
                const unsigned long long x = valid ? src[i] : 0ull;
                const int dg = (int)(x >> sh) & 255;
                unsigned long long peers = __ballot(valid);
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    const unsigned long long bm = __ballot(valid && ((dg >> b) & 1));
                    peers &= ((dg >> b) & 1) ? bm : ~bm;
                }
                const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
                int base = 0;
                if (valid && lane == leader) { base = s_hist[wave][dg]; s_hist[wave][dg] = base + __popcll(peers); }
                base = __shfl(base, leader, 64);
                if (valid) dst[base + __popcll(peers & lt)] = x;
            }
            __syncthreads();
            unsigned long long *tmp = src; src = dst; dst = tmp;
        }

        // ---- greedy in-roll suppression in key order, a chunk of kTopThreads candidates at a time, until D are kept ----
        TopCandDev *out = cand + (size_t)br * D;
        if (t == 0) { s_nk = 0; s_last = -1; }
        __syncthreads();
        for (int c0 = 0; c0 < N; c0 += kTopThreads) {
            const int nk0 = s_nk;
            if (nk0 >= D) break;
            {
                const int i = c0 + t;
                bool ok = i < N;
                if (ok) {
                    const unsigned lo = (unsigned)src[i];
                    const int r = (int)(lo >> 16), c = (int)(lo & 0xFFFF);
                    for (int j = 0; j < nk0 && ok; j++) {
                        int kr, kc;
                        if (j < kTopKeptLds) { kr = s_kept[j] >> 16; kc = s_kept[j] & 0xFFFF; } else { kr = out[j].row; kc = out[j].col; }
                        ok = top_cheb(r, c, kr, kc) > radius;
                    }
                }
                s_ok[t] = ok ? 1 : 0;
            }
            __syncthreads();
            if (wave == 0) {
                int nk = nk0, last = s_last;
                for (int s = 0; s < kTopWaves && nk < D; s++) {
                    const int i = c0 + s * 64 + lane;
                    bool ok = s_ok[s * 64 + lane] != 0;
                    unsigned long long x = ok ? src[i] : 0ull;
                    const int r = (int)(((unsigned)x) >> 16), c = (int)(x & 0xFFFF);
                    for (int j = nk0; j < nk && ok; j++) {               // kept earlier in this chunk
                        int kr, kc;
                        if (j < kTopKeptLds) { kr = s_kept[j] >> 16; kc = s_kept[j] & 0xFFFF; } else { kr = out[j].row; kc = out[j].col; }
                        ok = top_cheb(r, c, kr, kc) > radius;
                    }
                    unsigned long long m = __ballot(ok);
                    while (m && nk < D) {
                        const int l = __ffsll((long long)m) - 1;
                        const int kr = __shfl(r, l, 64), kc = __shfl(c, l, 64);
                        if (lane == l) {
                            const unsigned key = (unsigned)(x >> 32);
                            TopCandDev q;
                            q.vote = top - (int)(key >> lbits);
                            q.row = (short)r; q.col = (short)c;
                            q.len = W - (int)(key & ((1u << lbits) - 1u));
                            q.h_locmax = 0.0f;
                            out[nk] = q;
                            if (nk < kTopKeptLds) s_kept[nk] = (r << 16) | c;
                            ok = false;
                        } else if (ok && top_cheb(r, c, kr, kc) <= radius) {
                            ok = false;
                        }
                        last = c0 + s * 64 + l;
                        nk++;
                        m = __ballot(ok);
                    }
                }
                if (lane == 0) { s_nk = nk; s_last = last; }
            }
            __syncthreads();
        }
        const int nk = s_nk;
        // the z window of every kept entry (pick_rules.h; k_vote_record's, 1342-1351): a lane owns an entry and walks its slots itself
        for (int j = t; j < nk; j += kTopThreads) {
            const int r = out[j].row, c = out[j].col;
            int zk = haf_pick_math::z_window_start();
            for (int q = 0; q < haf_pick_math::kZWindowSlots; q++) {
                int rr, cc;
                if (haf_pick_math::z_window_slot(q, r, c, H, W, &rr, &cc)) zk = haf_pick_math::z_window_fold(zk, heights[(size_t)br * HW + (size_t)rr * W + cc]);
            }
            out[j].h_locmax = key2f(zk);
        }
        if (t == 0) {
            hdr[4 * br] = nk;
            hdr[4 * br + 1] = (nk >= D && s_last + 1 < N) ? 1 : 0;    // unvisited candidates remain: the sequence may go on
            hdr[4 * br + 2] = rec[br].n_evals;
            hdr[4 * br + 3] = top;
        }
        __syncthreads();
    }
}

void launch_top_grasps(const short *ev16, const float *heights, const RollRecordDev *rec, unsigned long long *scratch, size_t slot_words,
                       int n_slots, int *hdr, TopCandDev *cand, int D, int min_vote, int radius, Dims d, hipStream_t s)
{
    hipLaunchKernelGGL(k_top_grasps, dim3(n_slots), dim3(kTopThreads), 0, s, ev16, heights, rec, scratch, slot_words, hdr, cand, D,
                       min_vote, radius, d);
}

}  // namespace haf
