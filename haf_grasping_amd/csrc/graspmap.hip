// graspmap.hip -- k_grasp_map<KIND>: the per-pixel grasp map of haf_grasp_map (engine_graspmap.cpp) -- for every pixel of a sensor frame
// the best vote any roll of a request of the last scored batch gives the cell the pixel's point falls into, that roll and that cell.
// The definition is haf_grasp_map_ref's (graspmap_host.cpp), compiled from the same two headers: frame_points.h (pixel -> base-frame
// point) and grasp_cells.h (point -> cell of a roll).  The two agree in every pixel (tests/test_grasp_map_gpu.py).
//
// A streaming kernel with R gathers per pixel.  A lane owns a GROUP of consecutive pixels exactly as in k_frame_points (frame_group.h):
// eight of a U16 frame, four of an F32 or XYZ frame, one global_load_dwordx4 where the group is aligned.
//   * the frame's constants arrive as a kernel argument and the R roll transforms (64 bytes each) are read by a wave-uniform index:
//     both are scalar loads, a roll costs a lane no vector load but its gathers;
//   * per roll the lane computes its G cells, then issues its G gathers from the request's vote grids (2 bytes each; R grids of H*W
//     shorts -- 125 KB at 56 x 56 x 20, 18 MB at 512 x 512 x 36 -- which neighbouring pixels share: they mostly hit L2), then keeps the
//     larger vote with a strict '>' (rolls ascend: the lowest roll wins a tie);
//   * the three images are packed width * height arrays and a group starts at a multiple of G pixels, so a whole group is ONE
//     global_store_dwordx4 (dwordx2 for G = 4) per 16-bit image and two (one) dwordx4 for the cells when the caller's base is aligned
//     accordingly; a misaligned base or the frame's last, partial group stores element by element.
// Floor per pixel: 2-12 bytes read, 8 written, R two-byte gathers.  It reads the vote grids and nothing else of the request.
//
// k_map_best: the masked best pixel of haf_grasp_map_best -- a wave-level maximum of a packed 64-bit key over the pixels whose mask
// byte is not zero and that qualify (pick_rules.h: pick_qualifies), then one 64-bit atomicMax per wave.  The key is pick_rules.h's
// pick_key: its maximum is vote descending, roll ascending, then v, then u ascending.
// k_cell_record: the record of one arbitrary cell for haf_cell_pose (device_common.h: cell_record), with the 9 x 8 z window of k_top_grasps.
// k_map_labels / k_label_records: haf_grasp_map_labels -- the masked best of every label of an instance-label image in one pass over the
// frame (a segmented arg-max of the same key in a per-workgroup LDS table), then one wave per label for its pick and its record.
// k_map_labels_objects / k_object_records: haf_score_objects -- the same pass ACROSS the requests of a batch that share one frame: a pixel
// of label l gathers from the grids of the request l belongs to, and the tables are indexed by request.
#include "object_group.h"

namespace haf {

using haf_cell_math::CellGeo;
using haf_pick_math::pick_key;
using haf_pick_math::pick_qualifies;

// The roll loop of a group: for each of its G points that takes part (usable[k]) the best vote over the R rolls, that roll (global index)
// and that cell; kNoCellVote, -1, -1 where no roll has a cell.  k_grasp_map and k_map_labels both call it: one arithmetic, one order
template <unsigned G>
__device__ __forceinline__ void group_best(const float (&p)[G * 3], const bool (&usable)[G], const CellGeo *__restrict__ geo, int R, int roll_first,
                                           const short *__restrict__ ev16, int H, int W, float r_row, float r_col, int (&best)[G],
                                           int (&best_roll)[G], int (&best_cell)[G])
{
#pragma unroll
    for (unsigned k = 0; k < G; k++) { best[k] = haf_cell_math::kNoCellVote; best_roll[k] = -1; best_cell[k] = -1; }
    const size_t HW = (size_t)H * (size_t)W;
    for (int r = 0; r < R; r++) {
        const CellGeo &g = geo[r];                        // (r is wave-uniform: sixteen scalar registers)
        const global_ptr<const short> grid = as_global<const short>(ev16 + (size_t)r * HW);
        int ci[G], val[G];
#pragma unroll
        for (unsigned k = 0; k < G; k++) {
            const int c = haf_cell_math::point_cell(g.m, p[3 * k], p[3 * k + 1], p[3 * k + 2], r_row, r_col, H, W);
            ci[k] = usable[k] ? c : -1;
        }
#pragma unroll
        for (unsigned k = 0; k < G; k++) val[k] = ci[k] >= 0 ? (int)grid[ci[k]] : 0;      // (0 <= ci < H * W: inside roll r's grid)
#pragma unroll
        for (unsigned k = 0; k < G; k++)
            if (ci[k] >= 0 && (best_roll[k] < 0 || val[k] > best[k])) { best[k] = val[k]; best_roll[k] = roll_first + r; best_cell[k] = ci[k]; }
    }
}

template <int KIND>
__global__ __launch_bounds__(kFrameThreads) void k_grasp_map(const FrameDev f, const CellGeo *__restrict__ geo, int R, int roll_first,
                                                             const short *__restrict__ ev16, int H, int W, float r_row, float r_col,
                                                             short *__restrict__ vote, short *__restrict__ roll, int *__restrict__ cell)
{
    constexpr unsigned G = frame_group<KIND>();
    const unsigned n = (unsigned)f.n;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;      // (n < 2^31 and at most 2^11 points of slack: no wrap)
    if (i0 >= n) return;
    const bool whole = i0 + G <= n;
    float p[G * 3];
    group_points<KIND>(f, i0, n, p);

    bool usable[G];
    int best[G], best_roll[G], best_cell[G];
#pragma unroll
    for (unsigned k = 0; k < G; k++) usable[k] = i0 + k < n && haf_cell_math::point_usable(p + 3 * k);
    group_best<G>(p, usable, geo, R, roll_first, ev16, H, W, r_row, r_col, best, best_roll, best_cell);

    // a 16-bit image's group is 2 G bytes, the cells' 4 G: vector stores where the caller's base makes the group's address a multiple of that
    unsigned pv[G / 2], pr[G / 2];
#pragma unroll
    for (unsigned k = 0; k < G / 2; k++) {
        pv[k] = ((unsigned)best[2 * k] & 0xFFFFu) | ((unsigned)best[2 * k + 1] << 16);
        pr[k] = ((unsigned)best_roll[2 * k] & 0xFFFFu) | ((unsigned)best_roll[2 * k + 1] << 16);
    }
    auto store16 = [&](short *img, const unsigned (&w)[G / 2], const int (&e)[G]) {
        if (!img) return;
        short *at = img + i0;
        if (whole && (reinterpret_cast<uintptr_t>(at) & (2u * G - 1u)) == 0) {
            if constexpr (G == 8) *as_global<v4u>(at) = v4u{w[0], w[1], w[2], w[3]};
            else *as_global<v2u>(at) = v2u{w[0], w[1]};
        } else {
            const global_ptr<short> o = as_global<short>(at);
#pragma unroll
            for (unsigned k = 0; k < G; k++)
                if (i0 + k < n) o[k] = (short)e[k];
        }
    };
    store16(vote, pv, best);
    store16(roll, pr, best_roll);
    if (cell) {
        int *at = cell + i0;
        if (whole && (reinterpret_cast<uintptr_t>(at) & 15u) == 0) {
            const global_ptr<v4u> o = as_global<v4u>(at);
#pragma unroll
            for (unsigned j = 0; j < G / 4; j++)
                o[j] = v4u{(unsigned)best_cell[4 * j], (unsigned)best_cell[4 * j + 1], (unsigned)best_cell[4 * j + 2], (unsigned)best_cell[4 * j + 3]};
        } else {
            const global_ptr<int> o = as_global<int>(at);
#pragma unroll
            for (unsigned k = 0; k < G; k++)
                if (i0 + k < n) o[k] = best_cell[k];
        }
    }
}

void launch_grasp_map(const FrameDev &f, const CellGeo *geo, int R, int roll_first, const short *ev16, int H, int W, float r_row, float r_col,
                      short *vote, short *roll, int *cell, hipStream_t s)
{
    const unsigned G = f.kind == HAF_FRAME_DEPTH_U16 ? 8u : 4u;
    const unsigned groups = ((unsigned)f.n + G - 1) / G;
    if (!groups) return;
    const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads), block(kFrameThreads);
    with_frame_kind(f.kind, [&](auto K) {
        hipLaunchKernelGGL(k_grasp_map<decltype(K)::value>, grid, block, 0, s, f, geo, R, roll_first, ev16, H, W, r_row, r_col, vote, roll, cell);
    });
}

// ---- the masked best pixel ----
constexpr int kBestThreads = 256;

// mask: n packed bytes (the host's rows without their padding), or null for every pixel.  *best starts as 0, which no pixel's key is
__global__ __launch_bounds__(kBestThreads) void k_map_best(const short *__restrict__ vote, const short *__restrict__ roll,
                                                           const unsigned char *__restrict__ mask, unsigned n, int min_vote,
                                                           unsigned long long *__restrict__ best)
{
    unsigned long long key = 0ull;
    for (unsigned i = blockIdx.x * (unsigned)kBestThreads + threadIdx.x; i < n; i += gridDim.x * (unsigned)kBestThreads) {
        const int r = roll[i], v = vote[i];
        if (pick_qualifies(v, r, min_vote) && (!mask || mask[i] != 0)) {
            const unsigned long long k = pick_key(v, r, i);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best, key);
}

void launch_map_best(const short *vote, const short *roll, const unsigned char *mask, unsigned n, int min_vote, unsigned long long *best,
                     hipStream_t s)
{
    const unsigned blocks = std::max(1u, std::min(1024u, (n + kBestThreads - 1) / kBestThreads));
    hipLaunchKernelGGL(k_map_best, dim3(blocks), dim3(kBestThreads), 0, s, vote, roll, mask, n, min_vote, best);
}

// ---- the record of one cell ----
// rec[br] as k_top_grasps reads it (the roll's n_evals); out = cell_record (device_common.h) of cell (row, col) of (cloud, roll) br:
// {vote at the cell, row, col, its z window (pick_rules.h), n_evals}.  One wave.
__global__ __launch_bounds__(64) void k_cell_record(const short *__restrict__ ev16, const float *__restrict__ heights,
                                                    const RollRecordDev *__restrict__ rec, int br, int row, int col, int H, int W,
                                                    RollRecordDev *__restrict__ out)
{
    const size_t HW = (size_t)H * W;
    const RollRecordDev q = cell_record(ev16 + (size_t)br * HW, heights + (size_t)br * HW, rec[br].n_evals, row, col, H, W);
    if (threadIdx.x == 0) *out = q;
}

void launch_cell_record(const short *ev16, const float *heights, const RollRecordDev *rec, int br, int row, int col, int H, int W,
                        RollRecordDev *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_cell_record, dim3(1), dim3(64), 0, s, ev16, heights, rec, br, row, col, H, W, out);
}

// ---- the best pixel per instance label (haf_grasp_map_labels) ----
// k_map_labels<KIND, LABEL_BYTES>: a lane owns the group of G pixels k_grasp_map gives it and reads the group's labels FIRST: a group
// without a label in 1..n_labels is done before the deprojection and the R gathers (a background wave costs its label load).  A labelled
// pixel's (vote, roll, cell) is group_best's, the map's own; a qualifying one (pick_rules.h: pick_qualifies) sends pick_key(vote, roll, i) to
// its label's slot of the workgroup's table in dynamic LDS -- n_labels 64-bit keys, then n_labels 32-bit counts: 12 bytes per label, at
// most 48 KB -- with one LDS atomicMax and one atomicAdd.  At the end the workgroup walks its table and sends the non-zero slots on to
// the global table (zeroed by the caller): one 64-bit atomicMax and one atomicAdd each.  A label outside 1..n_labels indexes nothing.
template <int KIND, int LB>
__global__ __launch_bounds__(kFrameThreads) void k_map_labels(const FrameDev f, const CellGeo *__restrict__ geo, int R, int roll_first,
                                                              const short *__restrict__ ev16, int H, int W, float r_row, float r_col,
                                                              const void *__restrict__ labels, unsigned long long label_stride, int n_labels,
                                                              int min_vote, unsigned long long *__restrict__ g_key, unsigned *__restrict__ g_cnt)
{
    constexpr unsigned G = frame_group<KIND>();
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_key[];      // [n_labels] keys, then [n_labels] counts
    unsigned *s_cnt = reinterpret_cast<unsigned *>(s_key + n_labels);
    for (int l = threadIdx.x; l < n_labels; l += kFrameThreads) { s_key[l] = 0ull; s_cnt[l] = 0u; }
    __syncthreads();

    const unsigned n = (unsigned)f.n;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;
    if (i0 < n) {                                         // (no early return: every lane meets the barrier below)
        unsigned lab[G];
        group_labels<G, LB>(labels, label_stride, (unsigned)f.width, n, i0, n_labels, lab);      // (0, or 1..n_labels)
        bool any = false;
#pragma unroll
        for (unsigned k = 0; k < G; k++) any |= lab[k] != 0u;
        if (any) {
            float p[G * 3];
            group_points<KIND>(f, i0, n, p);
            bool usable[G];
            int best[G], best_roll[G], best_cell[G];
#pragma unroll
            for (unsigned k = 0; k < G; k++) usable[k] = lab[k] != 0u && i0 + k < n && haf_cell_math::point_usable(p + 3 * k);
            group_best<G>(p, usable, geo, R, roll_first, ev16, H, W, r_row, r_col, best, best_roll, best_cell);
#pragma unroll
            for (unsigned k = 0; k < G; k++)
                if (lab[k] != 0u && pick_qualifies(best[k], best_roll[k], min_vote)) {      // (1 <= lab <= n_labels: inside the table)
                    atomicMax(&s_key[lab[k] - 1u], pick_key(best[k], best_roll[k], i0 + k));
                    atomicAdd(&s_cnt[lab[k] - 1u], 1u);
                }
        }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n_labels; l += kFrameThreads) {
        const unsigned c = s_cnt[l];
        if (c) { atomicMax(&g_key[l], s_key[l]); atomicAdd(&g_cnt[l], c); }
    }
}

void launch_map_labels(const FrameDev &f, const CellGeo *geo, int R, int roll_first, const short *ev16, int H, int W, float r_row, float r_col,
                       const void *labels, size_t label_stride, int label_bytes, int n_labels, int min_vote, unsigned long long *g_key,
                       unsigned *g_cnt, hipStream_t s)
{
    with_frame_kind(f.kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        constexpr unsigned G = frame_group<KIND>();
        const unsigned groups = ((unsigned)f.n + G - 1) / G;
        if (!groups) return;
        const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads), block(kFrameThreads);
        const size_t lds = (size_t)n_labels * 12;
        if (label_bytes == 2)
            hipLaunchKernelGGL((k_map_labels<KIND, 2>), grid, block, lds, s, f, geo, R, roll_first, ev16, H, W, r_row, r_col, labels,
                               (unsigned long long)label_stride, n_labels, min_vote, g_key, g_cnt);
        else
            hipLaunchKernelGGL((k_map_labels<KIND, 1>), grid, block, lds, s, f, geo, R, roll_first, ev16, H, W, r_row, r_col, labels,
                               (unsigned long long)label_stride, n_labels, min_vote, g_key, g_cnt);
    });
}

// What a wave does once its table holds its key: k_label_records and k_object_records.  The key names the best pixel i and the roll; the
// pixel's point (point_of(i, u, v, p)) and its cell under that roll of the request's CellGeo (grasp_cells.h) are recomputed -- the
// arithmetic is deterministic: this is the cell the pass over the frame saw -- and the rest is cell_record at that cell.  *out = {the
// haf_label_pick image, the record}, written by lane 0: without a record for a key of 0 (nothing qualifies: label_out_none) and for a key
// that decodes to nothing, which cell = -2 marks (the host answers HAF_E_INTERNAL).  n: the frame's pixels, `width` to a row; geo / ev16 /
// heights / rec: the request's first roll of the last batch
__device__ __forceinline__ LabelOutDev label_out_none()
{
    LabelOutDev o;
    o.found = 0; o.u = o.v = o.roll = o.cell = -1; o.vote = haf_cell_math::kNoCellVote; o.n_pixels = 0;
    o.rec.vote = 0; o.rec.row = o.rec.col = 0; o.rec.h_locmax = 0.0f; o.rec.n_evals = 0;
    return o;
}
template <class PointOf>
__device__ __forceinline__ void finish_pick(unsigned long long key, unsigned count, unsigned n, unsigned width, const PointOf &point_of,
                                            const CellGeo *__restrict__ geo, int R, int roll_first, const short *__restrict__ ev16,
                                            const float *__restrict__ heights, const RollRecordDev *__restrict__ rec, int H, int W, float r_row,
                                            float r_col, LabelOutDev *__restrict__ out)
{
    LabelOutDev o = label_out_none();
    if (key == 0ull) {
        if (threadIdx.x == 0) *out = o;
        return;
    }
    const unsigned i = haf_pick_math::pick_key_pixel(key);
    const int roll = haf_pick_math::pick_key_roll(key), r = roll - roll_first;
    int ci = -2;
    unsigned u = 0, v = 0;
    if (i < n && r >= 0 && r < R) {
        v = i / width; u = i - v * width;
        float p[3];
        point_of(i, u, v, p);
        if (haf_cell_math::point_usable(p)) ci = haf_cell_math::point_cell(geo[r].m, p[0], p[1], p[2], r_row, r_col, H, W);
        if (ci < 0) ci = -2;
    }
    o.found = 1; o.u = (int)u; o.v = (int)v; o.vote = haf_pick_math::pick_key_vote(key); o.roll = roll; o.cell = ci; o.n_pixels = (int)count;
    if (ci >= 0) {                                        // (0 <= ci < H * W, 0 <= r < R)
        const size_t HW = (size_t)H * W;
        const int row = ci / W;
        o.rec = cell_record(ev16 + (size_t)r * HW, heights + (size_t)r * HW, rec[r].n_evals, row, ci - row * W, H, W);
    }
    if (threadIdx.x == 0) *out = o;
}

// k_label_records: one wave per label; the pixel's point is deprojected again from the frame (frame_points.h).  out[l]: label l + 1
__global__ __launch_bounds__(64) void k_label_records(const FrameDev f, const CellGeo *__restrict__ geo, int R, int roll_first,
                                                      const short *__restrict__ ev16, const float *__restrict__ heights,
                                                      const RollRecordDev *__restrict__ rec, int H, int W, float r_row, float r_col,
                                                      const unsigned long long *__restrict__ g_key, const unsigned *__restrict__ g_cnt,
                                                      LabelOutDev *__restrict__ out)
{
    const int l = blockIdx.x;
    const auto point_of = [&](unsigned, unsigned u, unsigned v, float *p) {
        const char *src = static_cast<const char *>(f.src) + (size_t)v * f.row_stride;
        if (f.kind == HAF_FRAME_DEPTH_U16) point_u16(f.m, u, v, *as_global<const uint16_t>(src + (size_t)u * 2), p);
        else if (f.kind == HAF_FRAME_DEPTH_F32) point_f32(f.m, u, v, *as_global<const float>(src + (size_t)u * 4), p);
        else {
            const global_ptr<const float> q = as_global<const float>(src + (size_t)u * f.point_stride);
            point_xyz(f.m, q[0], q[1], q[2], p);
        }
    };
    finish_pick(g_key[l], g_cnt[l], (unsigned)f.n, (unsigned)f.width, point_of, geo, R, roll_first, ev16, heights, rec, H, W, r_row, r_col, out + l);
}

void launch_label_records(const FrameDev &f, const CellGeo *geo, int R, int roll_first, const short *ev16, const float *heights,
                          const RollRecordDev *rec, int H, int W, float r_row, float r_col, int n_labels, const unsigned long long *g_key,
                          const unsigned *g_cnt, LabelOutDev *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_label_records, dim3(n_labels), dim3(64), 0, s, f, geo, R, roll_first, ev16, heights, rec, H, W, r_row, r_col, g_key,
                       g_cnt, out);
}

// ---- the best pixel per object ACROSS the requests of one frame (haf_score_objects) ----
// k_map_labels_objects<LABEL_BYTES>: what k_map_labels does for one request, for the B requests of a batch that share the frame and whose
// objects are instances of one label image.  A lane owns four pixels and reads their labels FIRST (object_group.h); a labelled pixel's
// request is the table's entry for its label (-1: no object of this call, or a request no roll ran for) and its point is read at its
// pixel index from the shared cloud -- the words k_frame_points wrote, whatever the frame's kind and residence: nothing is deprojected
// again.  The wave then takes its requests one after the other (next_request): CellGeo and the vote grids of the request in hand are
// wave-uniform, and (vote, roll, cell) of its pixels are group_best's -- k_map_labels' arithmetic and order.  A qualifying pixel
// (pick_qualifies) sends its pick_key to its REQUEST's slot of the workgroup's LDS table: B keys, then B counts, 12 bytes per request
// whatever n_labels is; the non-zero slots go on to the global table as in k_map_labels.  Bounds: 0 <= request < B by the host's table.
template <int LB>
__global__ __launch_bounds__(kFrameThreads) void k_map_labels_objects(const float *__restrict__ xyz, unsigned width, unsigned n,
                                                                      const CellGeo *__restrict__ geo, int B, int R, int roll_first,
                                                                      const short *__restrict__ ev16, int H, int W, float r_row, float r_col,
                                                                      const void *__restrict__ labels, unsigned long long label_stride,
                                                                      int n_labels, const int *__restrict__ req_of_label, int min_vote,
                                                                      unsigned long long *__restrict__ g_key, unsigned *__restrict__ g_cnt)
{
    constexpr unsigned G = kObjGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_okey[];      // [B] keys, then [B] counts
    unsigned *s_ocnt = reinterpret_cast<unsigned *>(s_okey + B);
    for (int b = threadIdx.x; b < B; b += kFrameThreads) { s_okey[b] = 0ull; s_ocnt[b] = 0u; }
    __syncthreads();

    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;      // (no early return: every lane meets the barrier below)
    int req[G];
    unsigned pending = group_requests<LB>(labels, label_stride, width, n, i0, req_of_label, n_labels, req);
    if (__ballot(pending != 0u) != 0ull) {                // (wave-uniform) a wave of background costs its label loads
        float p[G * 3];
        pending = group_cloud_points(xyz, i0, pending, p);
        const size_t HW = (size_t)H * (size_t)W;
        unsigned take;
        for (int b = next_request(req, pending, &take); b >= 0; b = next_request(req, pending, &take)) {
            bool usable[G];
            int best[G], best_roll[G], best_cell[G];
#pragma unroll
            for (unsigned k = 0; k < G; k++) usable[k] = (take & (1u << k)) != 0u;
            group_best<G>(p, usable, geo + (size_t)b * R, R, roll_first, ev16 + (size_t)b * R * HW, H, W, r_row, r_col, best, best_roll, best_cell);
#pragma unroll
            for (unsigned k = 0; k < G; k++)
                if (usable[k] && pick_qualifies(best[k], best_roll[k], min_vote)) {      // (0 <= b < B: inside the table)
                    atomicMax(&s_okey[b], pick_key(best[k], best_roll[k], i0 + k));
                    atomicAdd(&s_ocnt[b], 1u);
                }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += kFrameThreads) {
        const unsigned c = s_ocnt[b];
        if (c) { atomicMax(&g_key[b], s_okey[b]); atomicAdd(&g_cnt[b], c); }
    }
}

void launch_map_labels_objects(const float *xyz, int width, int n, const CellGeo *geo, int B, int R, int roll_first, const short *ev16, int H,
                               int W, float r_row, float r_col, const void *labels, size_t label_stride, int label_bytes, int n_labels,
                               const int *req_of_label, int min_vote, unsigned long long *g_key, unsigned *g_cnt, hipStream_t s)
{
    const unsigned groups = ((unsigned)std::max(0, n) + kObjGroup - 1) / kObjGroup;
    if (!groups || B < 1) return;
    const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads), block(kFrameThreads);
    const size_t lds = (size_t)B * 12;
    if (label_bytes == 2)
        hipLaunchKernelGGL(k_map_labels_objects<2>, grid, block, lds, s, xyz, (unsigned)width, (unsigned)n, geo, B, R, roll_first, ev16, H, W, r_row,
                           r_col, labels, (unsigned long long)label_stride, n_labels, req_of_label, min_vote, g_key, g_cnt);
    else
        hipLaunchKernelGGL(k_map_labels_objects<1>, grid, block, lds, s, xyz, (unsigned)width, (unsigned)n, geo, B, R, roll_first, ev16, H, W, r_row,
                           r_col, labels, (unsigned long long)label_stride, n_labels, req_of_label, min_vote, g_key, g_cnt);
}

// k_object_records: one wave per REQUEST; the pixel's point is read from the shared cloud, and finish_pick gets the request's own
// CellGeo, ev16, heights and rec.  out[b]: request b
__global__ __launch_bounds__(64) void k_object_records(const float *__restrict__ xyz, unsigned width, unsigned n, const CellGeo *__restrict__ geo,
                                                       int R, int roll_first, const short *__restrict__ ev16, const float *__restrict__ heights,
                                                       const RollRecordDev *__restrict__ rec, int H, int W, float r_row, float r_col,
                                                       const unsigned long long *__restrict__ g_key, const unsigned *__restrict__ g_cnt,
                                                       LabelOutDev *__restrict__ out)
{
    const int b = blockIdx.x;
    const auto point_of = [&](unsigned i, unsigned, unsigned, float *p) {
        const global_ptr<const float> q = as_global<const float>(xyz + (size_t)i * 3);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    };
    const size_t HW = (size_t)H * W, br0 = (size_t)b * R;
    finish_pick(g_key[b], g_cnt[b], n, width, point_of, geo + br0, R, roll_first, ev16 + br0 * HW, heights + br0 * HW, rec + br0, H, W, r_row, r_col,
                out + b);
}

void launch_object_records(const float *xyz, int width, int n, const CellGeo *geo, int B, int R, int roll_first, const short *ev16,
                           const float *heights, const RollRecordDev *rec, int H, int W, float r_row, float r_col,
                           const unsigned long long *g_key, const unsigned *g_cnt, LabelOutDev *out, hipStream_t s)
{
    if (B < 1) return;
    hipLaunchKernelGGL(k_object_records, dim3(B), dim3(64), 0, s, xyz, (unsigned)width, (unsigned)std::max(0, n), geo, R, roll_first, ev16, heights, rec,
                       H, W, r_row, r_col, g_key, g_cnt, out);
}

}  // namespace haf
