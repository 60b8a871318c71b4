// clearance_rules.h -- the per-point rules of haf_check_grasps (include/hafgrasp.h), written once: which scene point is NEAR a grasp,
// the three integer dot products that put it into the gripper's frame, and the region of the gripper it lies in.
//
// The same source is compiled for the device (clearance.hip) and for the host (clearance_host.cpp: haf_check_grasps_ref, the definition
// of record), on top of plane_rules.h -- whose usable-point rule and 1/4096 m coordinate word these are.  Everything here is int32
// arithmetic; the doubles of a grasp and of the gripper become integers ONCE per call on the host (clearance_host.cpp: grasp_frame,
// gripper_rules), and the derived metres come from the integer rows through ONE host function (clearance_finish).
//
// Units.  A scene point enters as q, its three coord_words (1/4096 m, |q| <= 2^16).  A grasp is twelve words: the origin o =
// lrint(4096 averaged_grasp_point) (|o| <= 2^16) and the axis words A, B, C = lrint(16384 axis): A along the approach vector, C the
// closing axis, B = A x C.  d = q - o; s = C . d, t = B . d, u = A . d are in units of 2^-12 x 2^-14 = 2^-26 m, the unit of every bound
// W(x) = llrint(x 2^26).
//
// The prefilter and why nothing after it overflows.  A point is NEAR when |d_j| <= reach_q for j = 0, 1, 2; only a near point is
// counted anywhere.  reach_q <= kClearMaxReachQ = 4099 (gripper_rules refuses a gripper of more than 1 m reach), an axis word is at most
// 16384 in magnitude, so |s|, |t|, |u| <= 3 x 4099 x 16384 < 2^28: three-term int32 sums, exact.  An unusable or masked-out pixel is
// the word kClearFarWord = 2^30 in x: |2^30 - o| >= 2^30 - 2^16 > reach_q, so it fails the prefilter by itself, and 2^30 + 2^16 does not
// overflow.  A void grasp carries reach_q = -1: no |d_j| is <= -1.
//
// No point inside a box fails the prefilter.  Let M be the integer matrix of rows C, B, A.  grasp_frame forms the axes in double as an
// orthonormal R (to ~1e-15) and rounds: M = 16384 R + E with |E_ij| <= 1/2, so ||E||_2 <= ||E||_F <= 3/2.  For any d,
//     |(s, t, u)| = |M d| >= 16384 |d| - |E d| >= (16384 - 3/2) |d|.
// A point in a box has |(s, t, u)| <= r 2^26 + 2, r = the circumscribed radius in metres of the boxes about the grasp point (the + 2:
// every bound is one rounded W or the sum of two).  So |d_j| <= |d| <= (r 2^26 + 2) / 16382.5 = 4096 r (1 + 9.2e-5) + 1.3e-4, which for
// r <= 1 is below 4096 r + 0.38.  reach_q = ceil(4096 r) + kClearReachMargin with a margin of 3 words covers that with room to spare
// (and the 1e-15 of R).  tests/test_clearance_cpu.py checks the same thing empirically: an independent definition WITHOUT the prefilter
// gives the same rows.
#pragma once
#include "plane_rules.h"

namespace haf_clear_math {

using namespace haf_plane_math;

constexpr int32_t kClearFarWord = 1 << 30;                // x word of a pixel that is unusable or masked out
constexpr int32_t kClearAxisOne = 16384;                  // an axis component of 1
constexpr int kClearBoundShift = 26;                      // bounds, s, t, u: units of 2^-26 m
constexpr int32_t kClearReachMargin = 3;                  // words (1/4096 m) added to ceil(4096 reach): see the proof above
constexpr int32_t kClearMaxReachQ = 4096 + kClearReachMargin;
constexpr int kClearGraspWords = 16;                      // a grasp on the device: A[3] B[3] C[3] o[3] reach_q and three words of padding
constexpr int kClearRowWords = 8;                         // a grasp's row, below

// a grasp's row: five counts, then the extremes of s and u over the BETWEEN points.  On the host they are plain int32 (0 where there is
// no between point); on the device the row is zeroed and the extremes travel as label_shape.h's words whose zero is the empty value
enum { CLEAR_NEAR = 0, CLEAR_FINGER0 = 1, CLEAR_FINGER1 = 2, CLEAR_PALM = 3, CLEAR_BETWEEN = 4, CLEAR_SMIN = 5, CLEAR_SMAX = 6, CLEAR_UMAX = 7 };
enum { CLEAR_REGION_NONE = 0, CLEAR_REGION_BETWEEN = 1, CLEAR_REGION_FINGER0 = 2, CLEAR_REGION_FINGER1 = 3, CLEAR_REGION_PALM = 4 };

// the gripper as the rules read it, formed ONCE per call on the host (gripper_rules of clearance_host.cpp); every word is a W()
struct ClearBounds {
    int32_t half_open;                                    // W(opening / 2)
    int32_t finger_out;                                   // W(opening / 2 + finger_thickness)
    int32_t half_breadth;                                 // W(finger_breadth / 2)
    int32_t u0, u1;                                       // -W(tip_depth), W(finger_length - tip_depth)
    int32_t palm_half_w, palm_half_b;                     // W(palm_width / 2), W(palm_breadth / 2)
    int32_t u2;                                           // u1 + W(palm_height)
    int32_t reach_q;                                      // 1/4096 m, of every grasp that is not void
};

struct GraspWords { int32_t a[3], b[3], c[3], o[3], reach_q, pad[3]; };
static_assert(sizeof(GraspWords) == kClearGraspWords * 4, "a grasp is sixteen words");

HAF_FRAME_HD int32_t i_abs(int32_t x) { return x < 0 ? -x : x; }

// |d_j| <= reach_q for all three j (d = q - o; |q| <= 2^30, |o| <= 2^16: no overflow)
HAF_FRAME_HD bool clear_near(int32_t dx, int32_t dy, int32_t dz, int32_t reach_q)
{
    return i_abs(dx) <= reach_q && i_abs(dy) <= reach_q && i_abs(dz) <= reach_q;
}

HAF_FRAME_HD int32_t clear_dot(const int32_t *w, int32_t dx, int32_t dy, int32_t dz) { return w[0] * dx + w[1] * dy + w[2] * dz; }

// the region of a NEAR point.  The intervals of s make between and the fingers disjoint, those of u the fingers and the palm (u < u1
// against u >= u1); the order of the tests settles the one degenerate case, an opening so small that W(opening / 2) = 0
HAF_FRAME_HD int clear_region(const ClearBounds &g, int32_t s, int32_t t, int32_t u)
{
    if (u >= g.u0 && u < g.u1 && i_abs(t) <= g.half_breadth) {
        if (s > -g.half_open && s < g.half_open) return CLEAR_REGION_BETWEEN;
        if (s >= -g.finger_out && s <= -g.half_open) return CLEAR_REGION_FINGER0;
        if (s >= g.half_open && s <= g.finger_out) return CLEAR_REGION_FINGER1;
        return CLEAR_REGION_NONE;
    }
    if (u >= g.u1 && u <= g.u2 && i_abs(s) <= g.palm_half_w && i_abs(t) <= g.palm_half_b) return CLEAR_REGION_PALM;
    return CLEAR_REGION_NONE;
}

// the x word of a pixel: its coord_word when the point is usable and admitted, else the far word (y and z are then 0)
HAF_FRAME_HD void clear_point_words(const float *p, bool admitted, int32_t *q)
{
    q[0] = kClearFarWord; q[1] = 0; q[2] = 0;
    if (admitted && point_usable(p)) { q[0] = coord_word(p[0]); q[1] = coord_word(p[1]); q[2] = coord_word(p[2]); }
}

}  // namespace haf_clear_math
