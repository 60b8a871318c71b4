// cellsegment.hip -- haf_segment_cells (include/hafgrasp.h): one sensor frame of any shape -> an image of object labels, by connected
// components of the occupied cells of the top-down grid.  The per-point and per-cell rules are cell_segment_rules.h's, the same source
// haf_segment_cells_ref runs on the host; all the rest is integer work whose result the definition fixes, so the two agree word for
// word (tests/test_cell_segment_gpu.py).
//
// Nine launches on one stream, each reading only what an EARLIER launch wrote or what reaches it through atomics:
//   1 k_cell_bin<KIND>   one-dimensional over pixel groups (frame_group.h), like k_label_shape.  Deprojects the group, applies the
//                        predicates and stores every pixel's cell word (-1: none).  Neighbouring pixels mostly share a cell -- a
//                        640-wide view of one metre puts about six pixels into each centimetre -- so the wave first groups equal cells,
//                        the wave-leader loop of k_label_shape, and sends ONE atomicAdd to the cell's count and ONE atomicMax to its top
//                        per distinct cell; the pixel counters go through wave sums and one atomic per workgroup.
//   2 k_cell_tile        one workgroup of 256 lanes per 64 x 16 cells.  The cells' tops (0: not occupied) sit in LDS with a one-cell
//                        halo left, right and below; each cell forms its link bits right, down, down-right and down-left, and the
//                        union-find of wave_union.h runs over the tile in LDS.  Writes parent[c] = the global index of the tile-local
//                        root (-1: not occupied) and into size[c] the link bits that leave the tile (0 elsewhere).
//   3 k_cell_seam        every cell with such bits: unite the roots on both sides in the global parent array, corner links included.
//   4 k_cell_flatten     every occupied cell finds its root, stores it and adds its point count to the root's size word.
//   5-7                  launch_segment_numbering (segment.hip: totals, one-workgroup scan, number) over the cells: the root's size
//                        word becomes its label, its table entry gets the point count, the anchor, and the anchor as the first box.
//   8 k_cell_table       one wave per 64 cells of a row: cells, box and largest top per label by integer atomics, one lane per (wave,
//                        label); the top-down label grid when the caller asked for it.
//   9 k_cell_write       every pixel takes the label of its cell word, stored in the requested element size.
// No kernel waits for another workgroup; there are no float atomics: counts are integer sums, heights maxima through label_shape.h's
// ordered key, unions atomicMin, so nothing depends on the order in which atomics arrive.
// Bounds: a pixel's words by group_points, bounded as in k_label_shape; a cell index comes from cell_of, which yields -1 or a value
// in [0, nx * ny); every LDS index is inside the tile plus halo by construction, and a cell is loaded only inside the grid; a link
// bit is set only towards an occupied cell, which lies inside the grid; a label indexes the tables only when it is in 1..max_labels;
// a label word is stored only for a pixel i < n at its own (row, column).
#include "frame_group.h"
#include "kernels.h"
#include "wave_union.h"

namespace haf {

using namespace haf_cell_math;

constexpr int kCellTileW = 64, kCellTileH = 16, kCellThreads = 256;
constexpr int kCellRowsPerLane = kCellTileW * kCellTileH / kCellThreads;      // 4
constexpr int kCellPW = kCellTileW + 2, kCellPH = kCellTileH + 1;             // the tile with its left, right and bottom halo
constexpr int kCellInfoInts = 7;                                              // a table entry of k_segment_number
constexpr int kCellTableRows = kCellThreads / 64;                             // k_cell_table: a wave per row of 64 cells
static_assert(kCellThreads == kFrameThreads && kCellThreads == kScanThreads, "one workgroup size throughout");

typedef int v4i_cell __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned wave_sum_u(unsigned x)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) x += (unsigned)__shfl_xor((int)x, off);
    return x;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned x)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, off));
    return x;
}

// lane 0 of every wave holds the wave's a and b: their sums over the workgroup go to word_a and word_b, one atomic each.  Called by
// all lanes of the workgroup
__device__ __forceinline__ void block_count2(unsigned a, unsigned b, unsigned *word_a, unsigned *word_b)
{
    __shared__ unsigned s_a[kCellThreads / 64], s_b[kCellThreads / 64];
    if ((threadIdx.x & 63u) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned ta = 0, tb = 0;
#pragma unroll
        for (int w = 0; w < kCellThreads / 64; w++) { ta += s_a[w]; tb += s_b[w]; }
        if (ta) atomicAdd(word_a, ta);
        if (tb) atomicAdd(word_b, tb);
    }
}

template <int KIND>
__global__ __launch_bounds__(kCellThreads) void k_cell_bin(const CellSegDev d)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned n = (unsigned)d.f.n;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned i0 = (blockIdx.x * (unsigned)kCellThreads + threadIdx.x) * G;      // (n < 2^31 and one workgroup of slack: no wrap)
    float p[G * 3] = {};
    if (i0 < n) group_points<KIND>(d.f, i0, n, p);
    int cell[G];
    unsigned top[G];
    unsigned pending = 0, n_fg = 0, n_out = 0;            // bit k: pixel i0 + k has a cell and is not folded yet
#pragma unroll
    for (unsigned k = 0; k < G; k++) {
        cell[k] = -1;
        top[k] = 0u;
        if (i0 + k < n && cell_foreground(p + 3 * k, d.r)) {
            n_fg++;
            const int c = cell_of(p + 3 * k, d.r);
            if (c < 0) n_out++;
            else { cell[k] = c; top[k] = shape_enc(cell_height_key(p + 3 * k, d.r)); pending |= 1u << k; }
        }
    }
    if (i0 + G <= n) {                                    // (the cell words start at a multiple of 16 bytes, i0 is a multiple of four)
#pragma unroll
        for (unsigned k = 0; k < G; k += 4) {
            const v4i_cell w = {cell[k], cell[k + 1], cell[k + 2], cell[k + 3]};
            *as_global<v4i_cell>(d.cell + i0 + k) = w;
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < G; k++)
            if (i0 + k < n) d.cell[i0 + k] = cell[k];
    }
    unsigned long long todo = __ballot(pending != 0u);
    while (todo) {                                        // (uniform; every pass retires at least the leader's first pending pixel)
        const unsigned leader = (unsigned)__ffsll((long long)todo) - 1u;
        int mine = -1;                                    // the cell of this lane's first pending pixel
#pragma unroll
        for (int k = (int)G - 1; k >= 0; k--) mine = (pending >> k) & 1u ? cell[k] : mine;
        const int cur = __shfl(mine, (int)leader);
        unsigned cnt = 0, t = 0;
#pragma unroll
        for (unsigned k = 0; k < G; k++)
            if (((pending >> k) & 1u) && cell[k] == cur) {
                cnt++;
                t = max(t, top[k]);
                pending &= ~(1u << k);
            }
        const unsigned long long same = __ballot(cnt != 0u);
        if (__popcll(same) > 1) { cnt = wave_sum_u(cnt); t = wave_max_u(t); }      // (uniform)
        if (lane == leader) {                             // (0 <= cur < nx * ny: cell_of's)
            atomicAdd(d.count + cur, cnt);
            atomicMax(d.top + cur, t);
        }
        todo = __ballot(pending != 0u);
    }
    block_count2(wave_sum_u(n_fg), wave_sum_u(n_out), d.counters + CELL_CNT_FG, d.counters + CELL_CNT_OUTSIDE);
}

__device__ __forceinline__ int cell_tiles_x(int nx) { return (nx + kCellTileW - 1) / kCellTileW; }

__global__ __launch_bounds__(kCellThreads) void k_cell_tile(const CellSegDev d)
{
    // an occupied cell's top is never 0: every foreground point has a height that is no NaN, whose key lies above INT32_MIN
    __shared__ unsigned s_top[kCellPH * kCellPW];
    __shared__ int s_parent[kCellTileW * kCellTileH];
    const int nx = d.r.nx, ny = d.r.ny;
    const int tiles_x = cell_tiles_x(nx);
    const int u0 = (int)(blockIdx.x % (unsigned)tiles_x) * kCellTileW, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * kCellTileH;
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);

    for (int h = (int)threadIdx.x; h < kCellPH * kCellPW; h += kCellThreads) {
        const int ty = h / kCellPW, tx = h - ty * kCellPW, gx = u0 - 1 + tx, gy = v0 + ty;
        unsigned t = 0u;
        if (gx >= 0 && gx < nx && gy < ny) {
            const int c = gy * nx + gx;
            if (d.count[c] > 0u) t = d.top[c];
        }
        s_top[h] = t;
    }
    __syncthreads();

    // bit 0 occupied; bits 1..4 linked to the neighbour right, down, down-right, down-left (a neighbour outside the grid is not occupied)
    const bool corners = d.r.connectivity == 8;
    const float max_step = d.r.max_step;
    unsigned bits[kCellRowsPerLane];
#pragma unroll
    for (int i = 0; i < kCellRowsPerLane; i++) {
        const int y = ly + 4 * i, c = y * kCellPW + lx + 1;
        const unsigned t = s_top[c], tr = s_top[c + 1], td = s_top[c + kCellPW], tdr = s_top[c + kCellPW + 1], tdl = s_top[c + kCellPW - 1];
        const bool occ = t != 0u;
        const bool right = occ && tr != 0u && cells_linked(t, tr, max_step), down = occ && td != 0u && cells_linked(t, td, max_step);
        const bool dr = corners && occ && tdr != 0u && cells_linked(t, tdr, max_step);
        const bool dl = corners && occ && tdl != 0u && cells_linked(t, tdl, max_step);
        bits[i] = (occ ? 1u : 0u) | (right ? 2u : 0u) | (down ? 4u : 0u) | (dr ? 8u : 0u) | (dl ? 16u : 0u);
        s_parent[y * kCellTileW + lx] = occ ? y * kCellTileW + lx : -1;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCellRowsPerLane; i++) {
        const int y = ly + 4 * i, l = y * kCellTileW + lx;
        const bool in_x = lx < kCellTileW - 1, in_y = y < kCellTileH - 1;
        if ((bits[i] & 2u) && in_x) uf_unite<true>(s_parent, l, l + 1);
        if ((bits[i] & 4u) && in_y) uf_unite<true>(s_parent, l, l + kCellTileW);
        if ((bits[i] & 8u) && in_x && in_y) uf_unite<true>(s_parent, l, l + kCellTileW + 1);
        if ((bits[i] & 16u) && lx > 0 && in_y) uf_unite<true>(s_parent, l, l + kCellTileW - 1);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCellRowsPerLane; i++) {
        const int y = ly + 4 * i, l = y * kCellTileW + lx;
        if (u0 + lx >= nx || v0 + y >= ny) continue;
        const int gi = (v0 + y) * nx + u0 + lx;            // (< nx * ny <= 2^22)
        int parent = -1;
        if (bits[i] & 1u) {
            const int root = uf_find<true>(s_parent, l);
            parent = (v0 + (root >> 6)) * nx + u0 + (root & 63);
        }
        const bool last_x = lx == kCellTileW - 1, last_y = y == kCellTileH - 1;
        d.parent[gi] = parent;
        // the links that leave the tile: bit 0 right, 1 down, 2 down-right, 3 down-left
        d.size[gi] = (int)((((bits[i] & 2u) && last_x) ? 1u : 0u) | (((bits[i] & 4u) && last_y) ? 2u : 0u) |
                           (((bits[i] & 8u) && (last_x || last_y)) ? 4u : 0u) | (((bits[i] & 16u) && (lx == 0 || last_y)) ? 8u : 0u));
    }
}

// one lane per cell; only a cell on a tile's border holds bits.  A lane clears its own cell's word and no other
__global__ __launch_bounds__(kCellThreads) void k_cell_seam(const CellSegDev d)
{
    const int nx = d.r.nx;
    const unsigned i = blockIdx.x * (unsigned)kCellThreads + threadIdx.x;
    if (i >= (unsigned)(nx * d.r.ny)) return;
    const unsigned bits = (unsigned)d.size[i];
    if (bits == 0u) return;
    d.size[i] = 0;
    const int c = (int)i;                                 // (linked: the neighbour is occupied, so inside the grid)
    if (bits & 1u) uf_unite<false>(d.parent, c, c + 1);
    if (bits & 2u) uf_unite<false>(d.parent, c, c + nx);
    if (bits & 4u) uf_unite<false>(d.parent, c, c + nx + 1);
    if (bits & 8u) uf_unite<false>(d.parent, c, c + nx - 1);
}

// wave_add_by_key with a value per lane: adds the values of the lanes that share a key with one atomic per distinct key of the wave
__device__ __forceinline__ void wave_sum_by_key(int *word, bool active, int key, unsigned value)
{
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long todo = __ballot(active);
    while (todo) {                                        // (uniform; every pass retires at least the leader)
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const bool mine = active && key == k;
        const unsigned long long same = __ballot(mine);
        unsigned v = mine ? value : 0u;
        if (__popcll(same) > 1) v = wave_sum_u(v);        // (uniform)
        if (lane == leader) atomicAdd(word + k, (int)v);
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kCellThreads) void k_cell_flatten(const CellSegDev d)
{
    const unsigned i = blockIdx.x * (unsigned)kCellThreads + threadIdx.x;
    const bool active = i < (unsigned)(d.r.nx * d.r.ny) && d.parent[i] >= 0;
    int root = 0;
    unsigned cnt = 0;
    if (active) {
        root = uf_find<false>(d.parent, (int)i);
        d.parent[i] = root;                               // (a lane whose walk passes here reads the old ancestor or the root: both lead to the root)
        cnt = d.count[i];
    }
    wave_sum_by_key(d.size, active, root, cnt);           // (a component's points are a frame's at most: < 2^31)
    block_count2((unsigned)__popcll(__ballot(active)), 0u, d.counters + CELL_CNT_OCCUPIED, d.counters + CELL_CNT_OCCUPIED);
}

// one wave per 64 cells of a row: lane = column
__global__ __launch_bounds__(kCellThreads) void k_cell_table(const CellSegDev d)
{
    const int nx = d.r.nx, ny = d.r.ny;
    const int tiles_x = cell_tiles_x(nx);
    const int lane = (int)(threadIdx.x & 63u);
    const int ub = (int)(blockIdx.x % (unsigned)tiles_x) * kCellTileW, ix = ub + lane;
    const int iy = (int)(blockIdx.x / (unsigned)tiles_x) * kCellTableRows + (int)(threadIdx.x >> 6);
    int label = 0;
    unsigned top = 0u;
    if (ix < nx && iy < ny) {
        const int c = iy * nx + ix, root = d.parent[c];
        if (root >= 0) { label = d.size[root]; top = d.top[c]; }
        if (d.cell_labels) d.cell_labels[c] = (uint16_t)label;
    }
    const bool active = label > 0;
    unsigned long long todo = __ballot(active);
    while (todo) {                                        // (uniform; every pass retires at least the leader)
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, leader);
        const bool mine = active && label == l;
        const unsigned long long same = __ballot(mine);
        unsigned t = mine ? top : 0u;
        if (__popcll(same) > 1) t = wave_max_u(t);        // (uniform)
        if (lane == leader) {                             // (1 <= l <= max_labels: inside both tables)
            const int lo = ub + __ffsll((long long)same) - 1, hi = ub + 63 - __clzll((long long)same);
            int *b = d.table + (size_t)(l - 1) * kCellInfoInts;
            unsigned *x = d.extra + (size_t)(l - 1) * 2;
            atomicAdd(x, (unsigned)__popcll(same));
            // (a box and a top only grow: a word read too old is further in than the true one, and the atomic is then merely superfluous)
            if (t > x[1]) atomicMax(x + 1, t);
            if (lo < b[3]) atomicMin(b + 3, lo);
            if (iy < b[4]) atomicMin(b + 4, iy);
            if (hi > b[5]) atomicMax(b + 5, hi);
            if (iy > b[6]) atomicMax(b + 6, iy);
        }
        todo &= ~same;
    }
}

// one lane per pixel
__global__ __launch_bounds__(kCellThreads) void k_cell_write(const CellSegDev d)
{
    const unsigned i = blockIdx.x * (unsigned)kCellThreads + threadIdx.x;
    if (i >= (unsigned)d.f.n) return;
    const int c = d.cell[i];
    const int label = c >= 0 ? d.size[d.parent[c]] : 0;   // (a pixel's cell holds that pixel: it is occupied and its parent word is its root)
    const unsigned W = (unsigned)d.f.width, v = i / W, u = i - v * W;
    char *o = static_cast<char *>(d.out) + (size_t)v * d.out_stride + (size_t)u * (size_t)d.elem_bytes;
    if (d.elem_bytes == 1) *as_global<unsigned char>(o) = (unsigned char)label;
    else *as_global<uint16_t>(o) = (uint16_t)label;
}

template <int KIND> static void launch_cell_bin(const CellSegDev &d, hipStream_t s)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned groups = ((unsigned)d.f.n + G - 1) / G;
    hipLaunchKernelGGL((k_cell_bin<KIND>), dim3((groups + kCellThreads - 1) / kCellThreads), dim3(kCellThreads), 0, s, d);
}

void launch_cell_segment(const CellSegDev &d, hipStream_t s)
{
    // (nx * ny <= 2^22 and width * height < 2^31: every grid below fits grid.x)
    const unsigned nx = (unsigned)d.r.nx, ny = (unsigned)d.r.ny, nc = nx * ny, n = (unsigned)d.f.n;
    const unsigned tiles_x = (nx + kCellTileW - 1) / kCellTileW;
    const unsigned cell_blocks = (nc + kCellThreads - 1) / kCellThreads;
    if (d.f.kind == HAF_FRAME_DEPTH_U16) launch_cell_bin<HAF_FRAME_DEPTH_U16>(d, s);
    else if (d.f.kind == HAF_FRAME_DEPTH_F32) launch_cell_bin<HAF_FRAME_DEPTH_F32>(d, s);
    else launch_cell_bin<HAF_FRAME_XYZ_F32>(d, s);
    hipLaunchKernelGGL(k_cell_tile, dim3(tiles_x * ((ny + kCellTileH - 1) / kCellTileH)), dim3(kCellThreads), 0, s, d);
    hipLaunchKernelGGL(k_cell_seam, dim3(cell_blocks), dim3(kCellThreads), 0, s, d);
    hipLaunchKernelGGL(k_cell_flatten, dim3(cell_blocks), dim3(kCellThreads), 0, s, d);
    // the numbering of segment.hip over the cells: a "frame" nx wide of nx * ny "pixels", the size rule on the summed point counts
    SegmentDev sd;
    memset(&sd, 0, sizeof sd);
    sd.f.width = (int)nx; sd.f.n = (int)nc;
    sd.height = (int)ny;
    sd.min_pixels = d.min_points; sd.max_labels = d.max_labels;
    sd.parent = d.parent; sd.size = d.size; sd.totals = d.totals;
    sd.counters = d.counters;                             // (its slots 1 and 2: CELL_CNT_COMPS, CELL_CNT_KEPT)
    sd.table = d.table;
    launch_segment_numbering(sd, s);
    hipLaunchKernelGGL(k_cell_table, dim3(tiles_x * ((ny + kCellTableRows - 1) / kCellTableRows)), dim3(kCellThreads), 0, s, d);
    hipLaunchKernelGGL(k_cell_write, dim3((n + kCellThreads - 1) / kCellThreads), dim3(kCellThreads), 0, s, d);
}

}  // namespace haf
