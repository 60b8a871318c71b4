// segment_rules.h -- the per-pixel rules of haf_segment_frame (include/hafgrasp.h), written once: which point is foreground and which
// two neighbouring foreground points are linked.
//
// The same source is compiled for the device (segment.hip: k_segment_tile) and for the host (segment_host.cpp: haf_segment_ref, the
// definition of record), as depth_filter.h is, on top of frame_points.h -- whose points and rounded fp32 operations these are: nothing
// of them is restated here.  Everything else of the definition (components, anchors, numbering) is integer work on these two predicates.
#pragma once
#include "frame_points.h"

namespace haf_segment_math {

using namespace haf_frame_math;

// what the predicates read of haf_segment_params: gap2 = max_gap * max_gap is formed ONCE per call on the host (segment_rules below)
struct SegmentRules {
    float plane[4];
    float min_height, max_height, gap2;
};

// h = ((plane[0] x + plane[1] y) + plane[2] z) + plane[3], left to right; p: the point's three words
HAF_FRAME_HD bool foreground(const float *p, const SegmentRules &r)
{
    const float h = f_add(f_add(f_add(f_mul(r.plane[0], p[0]), f_mul(r.plane[1], p[1])), f_mul(r.plane[2], p[2])), r.plane[3]);
    const bool finite = f_finite(p[0]) && f_finite(p[1]) && f_finite(p[2]);
    return finite && !f_nan(h) && h >= r.min_height && (r.max_height <= 0.0f || h <= r.max_height);
}

// two foreground points: d2 = ((dx dx + dy dy) + dz dz); a NaN or infinite d2 does not link.  linked(p, q) == linked(q, p): the
// differences only change their sign
HAF_FRAME_HD bool linked(const float *p, const float *q, float gap2)
{
    const float dx = f_sub(q[0], p[0]), dy = f_sub(q[1], p[1]), dz = f_sub(q[2], p[2]);
    const float d2 = f_add(f_add(f_mul(dx, dx), f_mul(dy, dy)), f_mul(dz, dz));
    return f_finite(d2) && d2 <= gap2;
}

}  // namespace haf_segment_math
