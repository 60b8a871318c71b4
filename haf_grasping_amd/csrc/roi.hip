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
//
// k_roi_mark_objects<LABEL_BYTES> (haf_score_objects): the cell sets of ALL requests of a batch whose requests share one frame and whose
// masks are the instances of one label image -- request b's mask is `labels == the label of its object` -- in ONE launch.
//   * a lane owns a group of four pixels and reads their labels FIRST (object_group.h: one 4- or 8-byte load where the group is
//     aligned inside a row); a group of background pixels costs that one load, a wave of them returns before anything else;
//   * a labelled pixel looks its request up in the label -> request table the host uploaded (n_labels small integers, -1: not an
//     object of this call; a label above n_labels indexes nothing) and reads its point at its pixel index from the shared cloud, as
//     k_roi_mark does, with the same finiteness rule;
//   * the wave then takes the requests its pixels belong to one after the other (next_request): the request in hand is wave-uniform,
//     so its R RollGeo are scalar loads, and each of its pixels sets its cell's bit in that request's grid of roll r by one 64-bit
//     atomicOr -- mark_cell below, the device function k_roi_mark sets its bits with.
// Bounded by the label loads (1 or 2 bytes per pixel) and R atomics per labelled, finite pixel.  Bounds: req is the host's table entry,
// inside [0, B) by construction (engine_objects.cpp); point_cell as above.  No workgroup waits for another.
#include "object_group.h"

namespace haf {

constexpr int kRoiThreads = 256;

// the bit of point p's cell under the transform g in the grid Sr (H rows of roi_row_words(W) words); nothing when p has no cell there
__device__ __forceinline__ void mark_cell(const RollGeo &g, const float *p, unsigned long long *__restrict__ Sr, int H, int W, float r_row, float r_col)
{
    const int c = haf_cell_math::point_cell(g.m, p[0], p[1], p[2], r_row, r_col, H, W);
    if (c < 0) return;
    const int row = c / W, col = c - row * W;             // (0 <= c < H * W)
    atomicOr(Sr + (size_t)row * roi_row_words(W) + (col >> 6), 1ull << (col & 63));
}

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
    for (int r = 0; r < R; r++) mark_cell(geo[r], p, S + (size_t)r * grid_words, H, W, r_row, r_col);   // (r is wave-uniform)
}

void launch_roi_mark(const unsigned char *mask, size_t mask_stride, int width, int n, const float *xyz, const RollGeo *geo, int R,
                     unsigned long long *S, int H, int W, float r_row, float r_col, hipStream_t s)
{
    if (n < 1) return;
    hipLaunchKernelGGL(k_roi_mark, dim3(((unsigned)n + kRoiThreads - 1) / kRoiThreads), dim3(kRoiThreads), 0, s, mask,
                       (unsigned long long)mask_stride, (unsigned)width, (unsigned)n, xyz, geo, R, S, H, W, r_row, r_col);
}

template <int LB>
__global__ __launch_bounds__(kRoiThreads) void k_roi_mark_objects(const void *__restrict__ labels, unsigned long long label_stride, unsigned width,
                                                                  unsigned n, const float *__restrict__ xyz, const int *__restrict__ req_of_label,
                                                                  int n_labels, const RollGeo *__restrict__ geo, int R,
                                                                  unsigned long long *__restrict__ S, int H, int W, float r_row, float r_col)
{
    const unsigned i0 = (blockIdx.x * (unsigned)kRoiThreads + threadIdx.x) * kObjGroup;      // (n < 2^31 and at most 2^10 points of slack: no wrap)
    int req[kObjGroup];
    unsigned pending = group_requests<LB>(labels, label_stride, width, n, i0, req_of_label, n_labels, req);
    if (__ballot(pending != 0u) == 0ull) return;          // a wave of background: its label loads were all it cost
    float p[kObjGroup * 3];
    pending = group_cloud_points(xyz, i0, pending, p);
    const size_t grid_words = (size_t)H * roi_row_words(W);
    unsigned take;
    for (int b = next_request(req, pending, &take); b >= 0; b = next_request(req, pending, &take)) {
        const RollGeo *const gb = geo + (size_t)b * R;    // (b is wave-uniform: scalar loads)
        unsigned long long *const Sb = S + (size_t)b * R * grid_words;
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (unsigned k = 0; k < kObjGroup; k++)
                if (take & (1u << k)) mark_cell(gb[r], p + 3 * k, Sb + (size_t)r * grid_words, H, W, r_row, r_col);
        }
    }
}

void launch_roi_mark_objects(const void *labels, size_t label_stride, int label_bytes, int width, int n, const float *xyz,
                             const int *req_of_label, int n_labels, const RollGeo *geo, int R, unsigned long long *S, int H, int W,
                             float r_row, float r_col, hipStream_t s)
{
    if (n < 1) return;
    const unsigned groups = ((unsigned)n + kObjGroup - 1) / kObjGroup;
    const dim3 grid((groups + kRoiThreads - 1) / kRoiThreads), block(kRoiThreads);
    if (label_bytes == 2)
        hipLaunchKernelGGL(k_roi_mark_objects<2>, grid, block, 0, s, labels, (unsigned long long)label_stride, (unsigned)width, (unsigned)n, xyz,
                           req_of_label, n_labels, geo, R, S, H, W, r_row, r_col);
    else
        hipLaunchKernelGGL(k_roi_mark_objects<1>, grid, block, 0, s, labels, (unsigned long long)label_stride, (unsigned)width, (unsigned)n, xyz,
                           req_of_label, n_labels, geo, R, S, H, W, r_row, r_col);
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
