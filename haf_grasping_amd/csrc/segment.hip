// segment.hip -- haf_segment_frame (include/hafgrasp.h): one sensor frame -> an image of object labels, by connected components of the
// link graph segment_rules.h defines.  The per-pixel predicates are that header's, the same source haf_segment_ref runs on the host; all
// the rest is integer work whose result the definition fixes, so the two agree word for word (tests/test_segment_gpu.py).
//
// Seven launches on one stream, each reading only what an EARLIER launch wrote or what reaches it through atomics:
//   1 k_segment_tile<KIND>  one workgroup of 256 lanes per 64 x 16 tile (k_depth_filter's geometry).  Deprojects the tile and a one-pixel
//                           right and bottom halo into LDS, forms each pixel's foreground bit and its right / down link bits, and runs a
//                           union-find over the tile in LDS.  Writes parent[i] = the global index of the tile-local root (-1: background)
//                           and, for the tile's last column and last row, the link bits that cross the border into size[i] (0 elsewhere).
//   2 k_segment_seam        only those border pixels: unite the roots on both sides in the global parent array.
//   3 k_segment_flatten     every foreground pixel finds its root, stores it and counts itself on the root's size word.
//   4 k_segment_totals      mark = "a root of size >= min_pixels"; the marks of 1024 consecutive pixels -> totals[block]; counts roots.
//   5 k_segment_scan        one workgroup: exclusive prefix sum of the totals, their sum -> counters.
//   6 k_segment_number      rank of every marked root in raster order = totals[block] + its place in the block.  The root's size word
//                           becomes its label (rank + 1, or 0 above max_labels); its table entry gets size, anchor, and the anchor as
//                           the first bounding box.
//   7 k_segment_write       every pixel: label = size[parent[i]], stored in the requested element size; the bounding boxes grow by
//                           integer atomicMin / atomicMax, one lane per (wave, label), skipped where they would change nothing.
//
// The union-find (wave_union.h, shared with cellsegment.hip) is the lock-free kind: parent[x] <= x always, a root is the lowest index of its set (the component's anchor), and
// uniting a and b is "find both roots, atomicMin the larger one's parent word with the smaller; if the word held something else, go on
// with what it held".  Every pass of that loop lowers the larger of its two indices, so a lane's loop ends on its own progress; no lane
// waits for another lane or workgroup anywhere in this file.  A stale read in a find only yields a former ancestor -- still a member of
// the same set -- and the atomic that follows returns the true word.  min, max and integer sums do not depend on the order of arrival.
// Bounds: a pixel is loaded and a word stored only inside the image; every LDS index is inside the tile plus halo by construction;
// a label indexes the table only when it is in 1..max_labels.
#include "frame_group.h"
#include "kernels.h"
#include "wave_union.h"       // uf_find / uf_unite, wave_add_by_key, block_scan

namespace haf {

using namespace haf_segment_math;

constexpr int kSegTileW = 64, kSegTileH = 16, kSegThreads = 256;
static_assert(kSegThreads == kScanThreads, "block_scan sums over the four waves of a workgroup");
constexpr int kSegRowsPerLane = kSegTileW * kSegTileH / kSegThreads;      // 4
constexpr int kSegPW = kSegTileW + 1, kSegPH = kSegTileH + 1;             // the tile with its right and bottom halo
constexpr int kSegSeamThreads = 128;                                      // 64 pixels of the last row + 16 of the last column
constexpr int kSegInfoInts = 7;                                           // haf_segment_info
constexpr int kSegWriteRows = kSegThreads / 64;                           // k_segment_write: a wave per row of 64 pixels

__device__ __forceinline__ int seg_tiles_x(int width) { return (width + kSegTileW - 1) / kSegTileW; }

template <int KIND>
__global__ __launch_bounds__(kSegThreads) void k_segment_tile(const SegmentDev d)
{
    __shared__ float s_x[kSegPH * kSegPW], s_y[kSegPH * kSegPW], s_z[kSegPH * kSegPW];
    __shared__ unsigned char s_fg[kSegPH * kSegPW];
    __shared__ int s_parent[kSegTileW * kSegTileH];
    __shared__ unsigned s_cnt[kSegThreads / 64];
    const int W = d.f.width, H = d.height;
    const int tiles_x = seg_tiles_x(W);
    const int u0 = (int)(blockIdx.x % (unsigned)tiles_x) * kSegTileW, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * kSegTileH;
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);

    for (int h = (int)threadIdx.x; h < kSegPH * kSegPW; h += kSegThreads) {
        const int ty = h / kSegPW, tx = h - ty * kSegPW, u = u0 + tx, v = v0 + ty;
        float p[3] = {__uint_as_float(kInvalidWord), __uint_as_float(kInvalidWord), __uint_as_float(kInvalidWord)};
        bool fg = false;
        if (u < W && v < H) {
            pixel_point<KIND>(d.f, u, v, p);
            fg = foreground(p, d.r);
        }
        s_x[h] = p[0]; s_y[h] = p[1]; s_z[h] = p[2];
        s_fg[h] = fg ? 1 : 0;
    }
    __syncthreads();

    // bit 0 foreground, bit 1 linked to the right neighbour, bit 2 linked to the one below (a neighbour outside the image is no foreground)
    unsigned bits[kSegRowsPerLane];
    unsigned n_fg = 0;                                    // the wave's total (uniform)
#pragma unroll
    for (int i = 0; i < kSegRowsPerLane; i++) {
        const int y = ly + 4 * i, c = y * kSegPW + lx, cr = c + 1, cd = c + kSegPW;
        const bool fg = s_fg[c] != 0;
        const float p[3] = {s_x[c], s_y[c], s_z[c]}, qr[3] = {s_x[cr], s_y[cr], s_z[cr]}, qd[3] = {s_x[cd], s_y[cd], s_z[cd]};
        const bool right = fg && s_fg[cr] != 0 && linked(p, qr, d.r.gap2), down = fg && s_fg[cd] != 0 && linked(p, qd, d.r.gap2);
        bits[i] = (fg ? 1u : 0u) | (right ? 2u : 0u) | (down ? 4u : 0u);
        s_parent[y * kSegTileW + lx] = fg ? y * kSegTileW + lx : -1;
        n_fg += (unsigned)__popcll(__ballot(fg));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSegRowsPerLane; i++) {
        const int y = ly + 4 * i, l = y * kSegTileW + lx;
        if ((bits[i] & 2u) && lx < kSegTileW - 1) uf_unite<true>(s_parent, l, l + 1);
        if ((bits[i] & 4u) && y < kSegTileH - 1) uf_unite<true>(s_parent, l, l + kSegTileW);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSegRowsPerLane; i++) {
        const int y = ly + 4 * i, l = y * kSegTileW + lx;
        if (u0 + lx >= W || v0 + y >= H) continue;
        const int gi = (v0 + y) * W + u0 + lx;            // (< width * height <= INT32_MAX)
        int parent = -1;
        if (bits[i] & 1u) {
            const int root = uf_find<true>(s_parent, l);
            parent = (v0 + (root >> 6)) * W + u0 + (root & 63);
        }
        d.parent[gi] = parent;
        d.size[gi] = (int)((((bits[i] & 2u) && lx == kSegTileW - 1) ? 1u : 0u) | (((bits[i] & 4u) && y == kSegTileH - 1) ? 2u : 0u));
    }
    if (lx == 0) s_cnt[ly] = n_fg;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kSegThreads / 64; w++) total += s_cnt[w];
        if (total) atomicAdd(d.counters + 0, total);
    }
}

// one workgroup per tile again: lanes 0..63 own the tile's last row (their link down leaves the tile), lanes 64..79 its last column
__global__ __launch_bounds__(kSegSeamThreads) void k_segment_seam(const SegmentDev d)
{
    const int W = d.f.width, H = d.height;
    const int tiles_x = seg_tiles_x(W);
    const int u0 = (int)(blockIdx.x % (unsigned)tiles_x) * kSegTileW, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * kSegTileH;
    const int t = (int)threadIdx.x;
    const bool row_lane = t < kSegTileW;
    const int u = u0 + (row_lane ? t : kSegTileW - 1), v = v0 + (row_lane ? kSegTileH - 1 : t - kSegTileW);
    int gi = -1;
    unsigned bits = 0;
    if (t < kSegTileW + kSegTileH && u < W && v < H) {
        gi = v * W + u;
        bits = (unsigned)d.size[gi];
    }
    __syncthreads();                                      // (the corner pixel has two lanes: both have read its bits before either clears them)
    if (gi < 0 || bits == 0) return;
    d.size[gi] = 0;
    if (row_lane) { if (bits & 2u) uf_unite<false>(d.parent, gi, gi + W); }       // (linked: the neighbour is foreground, so inside the image)
    else if (bits & 1u) uf_unite<false>(d.parent, gi, gi + 1);
}

__global__ __launch_bounds__(kSegThreads) void k_segment_flatten(const SegmentDev d)
{
    const unsigned i = blockIdx.x * (unsigned)kSegThreads + threadIdx.x;
    const bool active = i < (unsigned)d.f.n && d.parent[i] >= 0;
    int root = 0;
    if (active) {
        root = uf_find<false>(d.parent, (int)i);
        d.parent[i] = root;                               // (a lane whose walk passes here reads the old ancestor or the root: both lead to the root)
    }
    wave_add_by_key(d.size, active, root);
}

// the marks of a lane's four consecutive pixels from i0: bit k = pixel i0 + k is a root whose size passes the rule; roots: how many are roots
__device__ __forceinline__ unsigned lane_marks(const SegmentDev &d, unsigned i0, int &roots)
{
    unsigned m = 0;
    roots = 0;
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const unsigned i = i0 + k;
        if (i >= (unsigned)d.f.n) break;
        if (d.parent[i] != (int)i) continue;
        roots++;
        if (d.size[i] >= d.min_pixels) m |= 1u << k;
    }
    return m;
}

__global__ __launch_bounds__(kSegThreads) void k_segment_totals(const SegmentDev d)
{
    __shared__ int s_w[kSegThreads / 64];
    const unsigned i0 = blockIdx.x * (unsigned)kSegScanPixels + threadIdx.x * 4u;      // (n < 2^31 and at most 2^10 pixels of slack: no wrap)
    int roots, marks_total, roots_total;
    const unsigned m = lane_marks(d, i0, roots);
    (void)block_scan(__popc(m), s_w, marks_total);
    (void)block_scan(roots, s_w, roots_total);
    if (threadIdx.x == 0) {
        d.totals[blockIdx.x] = marks_total;
        if (roots_total) atomicAdd(d.counters + 1, (unsigned)roots_total);
    }
}

__global__ __launch_bounds__(kSegThreads) void k_segment_scan(const SegmentDev d, int n_blocks)
{
    __shared__ int s_w[kSegThreads / 64];
    int carry = 0;
    for (int c0 = 0; c0 < n_blocks; c0 += kSegThreads) {   // (uniform)
        const int i = c0 + (int)threadIdx.x;
        const int x = i < n_blocks ? d.totals[i] : 0;
        int total;
        const int ex = block_scan(x, s_w, total);
        if (i < n_blocks) d.totals[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) d.counters[2] = (unsigned)carry;
}

__global__ __launch_bounds__(kSegThreads) void k_segment_number(const SegmentDev d)
{
    __shared__ int s_w[kSegThreads / 64];
    const unsigned i0 = blockIdx.x * (unsigned)kSegScanPixels + threadIdx.x * 4u;
    int roots, total;
    const unsigned m = lane_marks(d, i0, roots);
    int rank = d.totals[blockIdx.x] + block_scan(__popc(m), s_w, total);
    if (!roots) return;
    const int W = d.f.width;
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const unsigned i = i0 + k;
        if (i >= (unsigned)d.f.n) break;
        if (d.parent[i] != (int)i) continue;
        int label = 0;
        if (m & (1u << k)) {
            label = rank < d.max_labels ? rank + 1 : 0;
            rank++;
        }
        if (label) {                                      // (1 <= label <= max_labels: inside the table)
            const int u = (int)(i % (unsigned)W), v = (int)(i / (unsigned)W);
            int *t = d.table + (size_t)(label - 1) * kSegInfoInts;
            t[0] = d.size[i]; t[1] = u; t[2] = v; t[3] = u; t[4] = v; t[5] = u; t[6] = v;
        }
        d.size[i] = label;
    }
}

// one wave per 64 pixels of a row: lane = column
__global__ __launch_bounds__(kSegThreads) void k_segment_write(const SegmentDev d)
{
    const int W = d.f.width, H = d.height;
    const int tiles_x = seg_tiles_x(W);
    const int lane = (int)(threadIdx.x & 63u);
    const int ub = (int)(blockIdx.x % (unsigned)tiles_x) * kSegTileW, u = ub + lane;
    const int v = (int)(blockIdx.x / (unsigned)tiles_x) * kSegWriteRows + (int)(threadIdx.x >> 6);
    int label = 0;
    if (u < W && v < H) {
        const int i = v * W + u, root = d.parent[i];
        if (root >= 0) label = d.size[root];
        char *o = static_cast<char *>(d.out) + (size_t)v * d.out_stride + (size_t)u * (size_t)d.elem_bytes;
        if (d.elem_bytes == 1) *as_global<unsigned char>(o) = (unsigned char)label;
        else *as_global<uint16_t>(o) = (uint16_t)label;
    }
    const bool active = label > 0;
    unsigned long long todo = __ballot(active);
    while (todo) {                                        // (uniform; every pass retires at least the leader)
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, leader);
        const unsigned long long same = __ballot(active && label == l);
        if (lane == leader) {
            const int lo = ub + __ffsll((long long)same) - 1, hi = ub + 63 - __clzll((long long)same);
            int *t = d.table + (size_t)(l - 1) * kSegInfoInts;
            // (a box only grows: a word read too old is further in than the true one, and the atomic is then merely superfluous)
            if (lo < t[3]) atomicMin(t + 3, lo);
            if (v < t[4]) atomicMin(t + 4, v);
            if (hi > t[5]) atomicMax(t + 5, hi);
            if (v > t[6]) atomicMax(t + 6, v);
        }
        todo &= ~same;
    }
}

void launch_segment_numbering(const SegmentDev &d, hipStream_t s)
{
    const unsigned scan_blocks = (unsigned)segment_scan_blocks((unsigned)d.f.n);
    hipLaunchKernelGGL(k_segment_totals, dim3(scan_blocks), dim3(kSegThreads), 0, s, d);
    hipLaunchKernelGGL(k_segment_scan, dim3(1), dim3(kSegThreads), 0, s, d, (int)scan_blocks);
    hipLaunchKernelGGL(k_segment_number, dim3(scan_blocks), dim3(kSegThreads), 0, s, d);
}

void launch_segment(const SegmentDev &d, hipStream_t s)
{
    // (width * height < 2^31, so the tiles of the image are fewer than 2^31 / 64 + 2^31 / 16, and the rows' segments fewer than 2^31 / 4
    // + 2^31 / 64: they fit grid.x)
    const unsigned tiles_x = (unsigned)((d.f.width + kSegTileW - 1) / kSegTileW);
    const unsigned tiles = tiles_x * (unsigned)((d.height + kSegTileH - 1) / kSegTileH);
    const unsigned n = (unsigned)d.f.n;
    if (d.f.kind == HAF_FRAME_DEPTH_U16) hipLaunchKernelGGL((k_segment_tile<HAF_FRAME_DEPTH_U16>), dim3(tiles), dim3(kSegThreads), 0, s, d);
    else if (d.f.kind == HAF_FRAME_DEPTH_F32) hipLaunchKernelGGL((k_segment_tile<HAF_FRAME_DEPTH_F32>), dim3(tiles), dim3(kSegThreads), 0, s, d);
    else hipLaunchKernelGGL((k_segment_tile<HAF_FRAME_XYZ_F32>), dim3(tiles), dim3(kSegThreads), 0, s, d);
    hipLaunchKernelGGL(k_segment_seam, dim3(tiles), dim3(kSegSeamThreads), 0, s, d);
    hipLaunchKernelGGL(k_segment_flatten, dim3((n + kSegThreads - 1) / kSegThreads), dim3(kSegThreads), 0, s, d);
    launch_segment_numbering(d, s);
    const unsigned segs = tiles_x * (unsigned)((d.height + kSegWriteRows - 1) / kSegWriteRows);
    hipLaunchKernelGGL(k_segment_write, dim3(segs), dim3(kSegThreads), 0, s, d);
}

}  // namespace haf
