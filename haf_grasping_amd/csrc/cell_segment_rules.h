// cell_segment_rules.h -- the per-point and per-cell rules of haf_segment_cells (include/hafgrasp.h), written once: which point is
// foreground, which cell of the top-down grid it falls into, and which two neighbouring occupied cells are linked.
//
// The same source is compiled for the device (cellsegment.hip) and for the host (cellsegment_host.cpp: haf_segment_cells_ref, the
// definition of record), as segment_rules.h is.  Nothing is restated: the points and the rounded fp32 operations are frame_points.h's,
// the height band is segment_rules.h's foreground(), the range rule plane_rules.h's point_usable(), the height and its ordered key
// label_shape.h's.  Everything else of the definition (counts, components, anchors, numbering) is integer work on these rules.
#pragma once
#include "segment_rules.h"
#include "label_shape.h"

namespace haf_cell_math {

using namespace haf_segment_math;
using namespace haf_shape_math;

// what the rules read of haf_cell_segment_params: inv_cell = 1.0f / cell is formed ONCE per call on the host (cell_rules of
// cellsegment_host.cpp); band.gap2 is not read
struct CellRules {
    SegmentRules band;
    float x0, y0, inv_cell, max_step;
    int nx, ny, connectivity;
};

// (plane_rules.h's range rule, said by name: grasp_cells.h has a point_usable of its own in THIS namespace, which would win unqualified)
HAF_FRAME_HD bool cell_foreground(const float *p, const CellRules &r) { return haf_plane_math::point_usable(p) && foreground(p, r.band); }

// f = (w - w0) * inv_cell; inside when 0 <= f < n.  A usable w, |w0| <= 64 and inv_cell <= 1000 keep f finite.  (int)f truncates,
// which is floorf for the f >= 0 that pass; -0.0f passes and gives 0; a w just below w0 gives f < 0 and is outside, never cell 0
HAF_FRAME_HD int cell_coord(float w, float w0, float inv_cell, int n)
{
    const float f = f_mul(f_sub(w, w0), inv_cell);
    return (f >= 0.0f && f < (float)n) ? (int)f : -1;
}
// the cell index iy * nx + ix of a foreground point, -1 when it lies outside the grid
HAF_FRAME_HD int cell_of(const float *p, const CellRules &r)
{
    const int ix = cell_coord(p[0], r.x0, r.inv_cell, r.nx), iy = cell_coord(p[1], r.y0, r.inv_cell, r.ny);
    return (ix >= 0 && iy >= 0) ? iy * r.nx + ix : -1;
}
// a foreground point's height key: foreground() has shown h to be no NaN, so the key is never kShapeNone
HAF_FRAME_HD int32_t cell_height_key(const float *p, const CellRules &r) { return height_key(shape_height(r.band.plane, p)); }

// A cell's top travels as shape_enc(key): an unsigned word whose zero is "no point yet" and whose unsigned order is the heights'.
// Two occupied cells with tops a, b: linked when max_step <= 0 or |a - b| <= max_step, the difference ONE subtraction -- a - b =
// -(b - a) exactly, so the rule is symmetric; inf - inf is a NaN and does not link
HAF_FRAME_HD bool cells_linked(uint32_t top_a, uint32_t top_b, float max_step)
{
    if (max_step <= 0.0f) return true;
    const float d = f_sub(key_height(shape_dec(top_a)), key_height(shape_dec(top_b)));
    return f_from_bits(f_bits(d) & 0x7FFFFFFFu) <= max_step;
}

}  // namespace haf_cell_math
