// roi.hip -- k_roi_mark: the ROI cell sets S_r of a haf_score_frames_roi request (include/hafgrasp.h) -- for every roll the cells that
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
#include "device_common.h"
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

}  // namespace haf
