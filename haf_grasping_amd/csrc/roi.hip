// roi.hip -- k_roi_mark, k_roi_mark_view: the ROI cell sets S_r of a haf_score_frames_roi / haf_score_views_roi request (include/hafgrasp.h) -- for every roll the cells that
// the points of the request's MASKED pixels fall into.  The definition is haf_roi_cells' (roi_host.cpp), compiled from the same two
// headers: frame_points.h (pixel -> base-frame point) and grasp_cells.h (point -> cell of a roll).
//
// The kernel runs behind k_frame_points on the request's stream and reads the pixel's point where that kernel has just written it (the
// points area of the request's input block, point index = pixel index v * width + u): the words ARE frame_points.h's, whatever the kind
// and residence of the frame, and the masked pixels -- a few per cent of the frame -- are not deprojected twice.
//
// A streaming kernel with R scattered bit stores per MASKED pixel, one lane per pixel:
//   * the mask byte is loaded first (neighbouring lanes read neighbouring bytes); a lane whose byte is zero does nothing more;
//   * a masked lane loads its point (12 bytes), drops out unless all three words are finite (the rule of haf_view_points), and per
//     roll computes the cell and sets its bit with one vector atomicOr on a 64-bit word;
//   * the roll transforms are read by a wave-uniform index: scalar loads.
// S is a bit set per (request, roll): H rows of roi_row_words(W) 64-bit words, bit (col & 63) of word (col >> 6) of row `row`, zeroed by
// the caller's hipMemsetAsync.  The bit form makes the dilation of k_mask_count_roi (prestages.hip) a handful of shifts per 64 cells and
// the gate of the vote (vote.hip) one word per quad.  Bounds: point_cell returns -1 or a cell inside [0, H * W).
//
// k_roi_mark_view<KIND> (haf_score_views_roi): the same sets for the VIEWS of fused requests.  k_view_points compacts a request's points
// in the order its atomics arrive, so a masked pixel's point has no index to be read at: the kernel deprojects it once more from the
// view's raw pixels, which still lie where k_view_points read them (staged host views in raw areas of their own, a device view in the
// caller's memory).  The arithmetic is group_points' (frame_group.h) and deterministic: the words are the ones that were compacted.
//   * a lane owns the group of 8 / 4 pixels group_points gives it and loads the group's mask bytes FIRST -- one 8- or 4-byte load where
//     the group lies inside one row at an aligned address, byte by byte elsewhere -- and is done when all are zero: a background wave
//     costs that one load;
//   * a group with a masked pixel is deprojected, and for every roll (wave-uniform index: scalar loads of RollGeo) each masked,
//     all-finite point's cell gets its bit by one 64-bit atomicOr;
//   * one launch per frame kind present in the batch, grid.y over every view of the batch (frames.hip: launch_kind); a block whose view
//     is of another kind, has no mask or ends before it returns at once.  The per-view constants (RoiViewDev: mask, stride, the
//     request's S and RollGeo) are wave-uniform.
// Bounds: a lane past the view's end marks nothing; a mask byte is read only for a pixel inside the view; point_cell as above.
#include "frame_group.h"
#include "grasp_cells.h"

namespace haf {

constexpr int kRoiThreads = 256;

__global__ __launch_bounds__(kRoiThreads) void k_roi_mark(const unsigned char *__restrict__ mask, unsigned long long mask_stride, unsigned width,
                                                          unsigned n, const float *__restrict__ xyz, const RollGeo *__restrict__ geo, int R,
                                                          unsigned long long *__restrict__ S, int H, int W, float r_row, float r_col)
{
    const unsigned i = blockIdx.x * (unsigned)kRoiThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned v = i / width, u = i - v * width;
    if (mask[(size_t)v * mask_stride + u] == 0) return;
    const float p[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
    if (!haf_cell_math::point_usable(p)) return;
    const size_t grid_words = (size_t)H * roi_row_words(W);
    for (int r = 0; r < R; r++) {
        const int c = haf_cell_math::point_cell(geo[r].m, p[0], p[1], p[2], r_row, r_col, H, W);   // (r is wave-uniform)
        if (c < 0) continue;
        const int row = c / W, col = c - row * W;                                                  // (0 <= c < H * W)
        atomicOr(S + (size_t)r * grid_words + (size_t)row * roi_row_words(W) + (col >> 6), 1ull << (col & 63));
    }
}

void launch_roi_mark(const unsigned char *mask, size_t mask_stride, int width, int n, const float *xyz, const RollGeo *geo, int R,
                     unsigned long long *S, int H, int W, float r_row, float r_col, hipStream_t s)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_roi_mark, dim3(((unsigned)n + kRoiThreads - 1) / kRoiThreads), dim3(kRoiThreads), 0, s, mask,
                       (unsigned long long)mask_stride, (unsigned)width, (unsigned)n, xyz, geo, R, S, H, W, r_row, r_col);
}

template <int KIND>
__global__ __launch_bounds__(kFrameThreads) void k_roi_mark_view(const FrameDev *__restrict__ frames, const RoiViewDev *__restrict__ views, int R,
                                                                 int H, int W, float r_row, float r_col)
{
    constexpr unsigned G = frame_group<KIND>();
    const FrameDev &f = frames[blockIdx.y];
    const RoiViewDev &rv = views[blockIdx.y];
    if (f.kind != KIND || rv.mask == nullptr) return;
    const unsigned n = (unsigned)f.n;
    const unsigned i0 = (blockIdx.x * (unsigned)kFrameThreads + threadIdx.x) * G;      // (n < 2^31 and at most 2^11 points of slack: no wrap)
    if (i0 >= n) return;
    const unsigned Wf = (unsigned)f.width;
    const unsigned v0 = i0 / Wf, u0 = i0 - v0 * Wf;
    unsigned sel = 0;                                     // bit k: pixel i0 + k exists and its mask byte is not zero
    const unsigned char *a = rv.mask + (size_t)v0 * rv.stride + u0;
    if (i0 + G <= n && u0 + G <= Wf && (reinterpret_cast<uintptr_t>(a) & (G - 1u)) == 0) {
        unsigned long long w;                             // the group's mask bytes in one load of G bytes: inside one row
        if constexpr (G == 8) w = *as_global<const unsigned long long>(a);
        else w = *as_global<const unsigned>(a);
        if (w == 0) return;
#pragma unroll
        for (unsigned k = 0; k < G; k++) sel |= ((w >> (8 * k)) & 0xFFull) ? 1u << k : 0u;
    } else {
        unsigned u = u0, v = v0;
#pragma unroll
        for (unsigned k = 0; k < G; k++) {
            if (i0 + k < n && *as_global<const unsigned char>(rv.mask + (size_t)v * rv.stride + u) != 0) sel |= 1u << k;
            if (++u == Wf) { u = 0; v++; }
        }
        if (sel == 0) return;
    }
    float p[G * 3];
    group_points<KIND>(f, i0, n, p);
#pragma unroll
    for (unsigned k = 0; k < G; k++)
        if (!haf_cell_math::point_usable(p + 3 * k)) sel &= ~(1u << k);
    if (sel == 0) return;
    const size_t grid_words = (size_t)H * roi_row_words(W);
    for (int r = 0; r < R; r++) {
        const RollGeo &g = rv.geo[r];                     // (r and the view are wave-uniform)
        unsigned long long *const Sr = rv.S + (size_t)r * grid_words;
#pragma unroll
        for (unsigned k = 0; k < G; k++) {
            if (!(sel & (1u << k))) continue;
            const int c = haf_cell_math::point_cell(g.m, p[3 * k], p[3 * k + 1], p[3 * k + 2], r_row, r_col, H, W);
            if (c < 0) continue;
            const int row = c / W, col = c - row * W;     // (0 <= c < H * W)
            atomicOr(Sr + (size_t)row * roi_row_words(W) + (col >> 6), 1ull << (col & 63));
        }
    }
}

template <int KIND> static void launch_mark_kind(const FrameDev *views_dev, const FrameDev *views_host, const RoiViewDev *roi_dev,
                                                 const RoiViewDev *roi_host, int n_views, int R, int H, int W, float r_row, float r_col,
                                                 hipStream_t s)
{
    constexpr unsigned G = frame_group<KIND>();
    unsigned groups = 0;
    for (int k = 0; k < n_views; k++)
        if (views_host[k].kind == KIND && roi_host[k].mask) groups = std::max(groups, ((unsigned)views_host[k].n + G - 1) / G);
    if (!groups) return;
    for (int k0 = 0; k0 < n_views; k0 += 65535) {             // (grid.y holds 65535 views)
        const dim3 grid((groups + kFrameThreads - 1) / kFrameThreads, (unsigned)std::min(65535, n_views - k0));
        hipLaunchKernelGGL(k_roi_mark_view<KIND>, grid, dim3(kFrameThreads), 0, s, views_dev + k0, roi_dev + k0, R, H, W, r_row, r_col);
    }
}

void launch_roi_mark_views(const FrameDev *views_dev, const FrameDev *views_host, const RoiViewDev *roi_dev, const RoiViewDev *roi_host,
                           int n_views, int R, int H, int W, float r_row, float r_col, hipStream_t s)
{
    launch_mark_kind<HAF_FRAME_DEPTH_U16>(views_dev, views_host, roi_dev, roi_host, n_views, R, H, W, r_row, r_col, s);
    launch_mark_kind<HAF_FRAME_DEPTH_F32>(views_dev, views_host, roi_dev, roi_host, n_views, R, H, W, r_row, r_col, s);
    launch_mark_kind<HAF_FRAME_XYZ_F32>(views_dev, views_host, roi_dev, roi_host, n_views, R, H, W, r_row, r_col, s);
}

}  // namespace haf
