// object_group.h -- what the kernels of haf_score_objects share (roi.hip: k_roi_mark_objects, graspmap.hip: k_map_labels_objects): a lane's
// group of kObjGroup consecutive pixels of a label image, the request each of them belongs to, and the walk of a wave over the
// requests its pixels belong to.  The requests of an objects call share one frame and differ in everything a roll reads (RollGeo,
// CellGeo, vote grids, cell sets), so a wave handles them one after the other: the request in hand is wave-uniform and its transforms
// stay scalar loads, as in the single-request kernels.  A wave of background pixels takes no turn, most labelled waves one or two.
#pragma once
#include "label_group.h"
#include "grasp_cells.h"

namespace haf {

constexpr unsigned kObjGroup = 4;

// req[k] = the request of pixel i0 + k: req_of_label[label - 1] for a label in 1..n_labels, -1 for the background, a label above
// n_labels and a pixel past the frame's end.  The labels first (label_group.h: group_labels); a group without a label reads nothing of
// the table.  Returns the bits of the k with req[k] >= 0.  Bounds: the table is read at an index below n_labels only
template <int LB>
__device__ __forceinline__ unsigned group_requests(const void *__restrict__ labels, unsigned long long label_stride, unsigned width, unsigned n,
                                                   unsigned i0, const int *__restrict__ req_of_label, int n_labels, int (&req)[kObjGroup])
{
    unsigned lab[kObjGroup];
    group_labels<kObjGroup, LB>(labels, label_stride, width, n, i0, n_labels, lab);
    unsigned sel = 0;
#pragma unroll
    for (unsigned k = 0; k < kObjGroup; k++) {
        req[k] = lab[k] != 0u ? req_of_label[lab[k] - 1u] : -1;      // (1 <= lab <= n_labels)
        if (req[k] >= 0) sel |= 1u << k;
    }
    return sel;
}

// The points of the group's selected pixels from the shared cloud (packed xyz in pixel order: the words k_frame_points wrote); a pixel
// whose point is not finite in all three words (the rule of haf_view_points) leaves sel.  Returns what is left of sel
__device__ __forceinline__ unsigned group_cloud_points(const float *__restrict__ xyz, unsigned i0, unsigned sel, float (&p)[kObjGroup * 3])
{
#pragma unroll
    for (unsigned k = 0; k < kObjGroup; k++) {
        p[3 * k] = p[3 * k + 1] = p[3 * k + 2] = 0.0f;
        if (!(sel & (1u << k))) continue;                 // (a selected pixel lies inside the frame: i0 + k < n)
        const global_ptr<const float> q = as_global<const float>(xyz + (size_t)(i0 + k) * 3);
        p[3 * k] = q[0]; p[3 * k + 1] = q[1]; p[3 * k + 2] = q[2];
        if (!haf_cell_math::point_usable(p + 3 * k)) sel &= ~(1u << k);
    }
    return sel;
}

// One turn of the wave's walk: the request of the lowest pending pixel of the wave's first lane that has one, as a wave-uniform
// value; -1 when no lane has a pending pixel.  *take = this lane's pending pixels of that request, which leave `pending`.  Every lane
// that calls it in one turn calls it in all of them (the return value is the loop's condition), and no lane waits for another wave
__device__ __forceinline__ int next_request(const int (&req)[kObjGroup], unsigned &pending, unsigned *take)
{
    int mine = -1;
#pragma unroll
    for (unsigned k = 0; k < kObjGroup; k++)
        if (mine < 0 && (pending & (1u << k))) mine = req[k];
    *take = 0u;
    const unsigned long long lanes = __ballot(mine >= 0);
    if (lanes == 0ull) return -1;
    const int b = __builtin_amdgcn_readfirstlane(__shfl(mine, __ffsll((long long)lanes) - 1, 64));
#pragma unroll
    for (unsigned k = 0; k < kObjGroup; k++)
        if ((pending & (1u << k)) && req[k] == b) *take |= 1u << k;
    pending &= ~*take;
    return b;
}

}  // namespace haf
