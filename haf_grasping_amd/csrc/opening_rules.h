// opening_rules.h -- the rules of haf_fit_openings (include/hafgrasp.h), written once on top of clearance_rules.h: the bin of a point along
// the closing axis, the slab it lies in, and the search for the first free placement over a grasp's two histograms.
//
// The same source is compiled for the device (opening.hip) and for the host (opening_host.cpp: haf_fit_openings_ref, the definition of
// record).  Scene points, the usable rule, a grasp's twelve words, void grasps, s / t / u and every W() are clearance_rules.h's and
// clearance_host.cpp's: nothing of them is restated here.  The doubles of the gripper and of the parameters become integers ONCE per
// call on the host (opening_host.cpp: opening_rules), and the derived metres come from the integer rows through ONE host function
// (opening_finish).
//
// For a fixed pose the question is one-dimensional.  The finger slab U0 <= u < U1, |t| <= W(finger_breadth / 2) and the palm slab
// U1 <= u <= U2, |t| <= W(palm_breadth / 2) do not depend on the opening; a point is in at most one of them (u < U1 against u >= U1).
// So ONE pass that histograms s over the two slabs answers every opening and every sideways shift.
//
// Bins.  B = 1 << shift words of 2^-26 m; bin(s) = s >= 0 ? s >> shift : ~((-s) >> shift): bin j >= 0 is [jB, (j + 1)B), bin -j - 1 is
// (-(j + 1)B, -jB] -- symmetric about 0, which makes the ownership of an edge clear_region's: a point at s = -jB belongs to finger 0,
// one at s = +jB to finger 1, neither to what lies between.  A histogram is kOpenBins = 128 words, word = bin + 64; only points with
// -half_bins <= bin < half_bins are counted.
//
// Every bin set of a placement lies inside [-63, 63).  With E = max(W(max_opening / 2) + W(finger_thickness), W(palm_width / 2)) +
// W(max_shift), shift the smallest with (E >> shift) + 2 <= 64, half_bins = (E >> shift) + 2, and floor(a) + floor(b) + floor(c) <=
// floor(a + b + c):
//     c_max + j_max + tb = (W(max_shift) >> shift) + (W(max_opening / 2) >> shift) + (W(finger_thickness) >> shift) + 1
//                       <= (E >> shift) + 1 = half_bins - 1 <= 63,
//     c_max + pb         = (W(max_shift) >> shift) + (W(palm_width / 2) >> shift) + 1 <= (E >> shift) + 1 = half_bins - 1 <= 63,
// and the lower ends are the negatives.  So a range [lo, hi) of a placement has -half_bins < lo <= hi < half_bins: every bin of it is
// counted, and lo + 64, hi + 64 index a prefix array of kOpenBins + 1 words.
//
// The prefilter.  A counted point has |s| <= half_bins B, and t and u inside one of the two slabs: it lies in the box es = half_bins B
// 2^-26 m, et, eu as gripper_rules forms them.  reach_q = ceil(4096 r) + kClearReachMargin with r that box's radius, refused above 1 m:
// the proof in clearance_rules.h -- no point inside the box fails the near test, nothing after it overflows -- carries over word for word
// (its r is this r; its "+ 2" covers a bound that is one rounded W or the sum of two, and half_bins B is an exact integer).
#pragma once
#include "clearance_rules.h"

namespace haf_open_math {

using namespace haf_clear_math;

constexpr int kOpenBins = 128;                            // words of one histogram
constexpr int kOpenZero = kOpenBins / 2;                  // the word of bin 0
constexpr int kOpenRowWords = 16;                         // a grasp's row as the search writes it, below

// a grasp's row: the placement found and the counts there.  OPEN_FOUND is 1, 0 or -1 (a void grasp, zeros elsewhere)
enum { OPEN_FOUND = 0, OPEN_J = 1, OPEN_C = 2, OPEN_SYM_J = 3, OPEN_BETWEEN = 4, OPEN_FINGER0 = 5, OPEN_FINGER1 = 6, OPEN_PALM = 7,
       OPEN_FINGER_SLAB = 8, OPEN_PALM_SLAB = 9 };
enum { OPEN_SLAB_NONE = 0, OPEN_SLAB_FINGER = 1, OPEN_SLAB_PALM = 2 };

// the gripper and the parameters as the rules read them, formed ONCE per call on the host (opening_rules of opening_host.cpp)
struct OpenRules {
    int32_t shift, half_bins;                             // B = 1 << shift; bins -half_bins .. half_bins - 1 are counted
    int32_t tb, pb;                                       // a finger's thickness and the palm's half width, in bins
    int32_t j_min, j_max, c_max;                          // half openings and shifts searched, in bins
    int32_t half_breadth, u0, u1;                         // the finger slab: W(finger_breadth / 2), -W(tip_depth), W(finger_length - tip_depth)
    int32_t palm_half_b, u2;                              // the palm slab: W(palm_breadth / 2), u1 + W(palm_height)
    int32_t reach_q;                                      // 1/4096 m, of every grasp that is not void
    int32_t max_hits, min_between;
};

HAF_FRAME_HD int32_t open_bin(int32_t s, int32_t shift) { return s >= 0 ? s >> shift : ~((-s) >> shift); }

// the slab of a NEAR point (|t|, |u| < 2^28)
HAF_FRAME_HD int open_slab(const OpenRules &r, int32_t t, int32_t u)
{
    if (u >= r.u0 && u < r.u1) return i_abs(t) <= r.half_breadth ? OPEN_SLAB_FINGER : OPEN_SLAB_NONE;
    if (u >= r.u1 && u <= r.u2) return i_abs(t) <= r.palm_half_b ? OPEN_SLAB_PALM : OPEN_SLAB_NONE;
    return OPEN_SLAB_NONE;
}

HAF_FRAME_HD bool open_bin_counted(const OpenRules &r, int32_t bin) { return bin >= -r.half_bins && bin < r.half_bins; }

// placements in the order of the search: p = 0, 1, .. runs over j ascending, then |c| ascending, then c ascending.  A half opening has
// 2 c_max + 1 shifts: 0, -1, +1, -2, +2, ..
HAF_FRAME_HD int32_t open_placements(const OpenRules &r) { return (r.j_max - r.j_min + 1) * (2 * r.c_max + 1); }
HAF_FRAME_HD void open_placement(const OpenRules &r, int32_t p, int32_t *j, int32_t *c)
{
    const int32_t nc = 2 * r.c_max + 1, q = p / nc, i = p - q * nc, m = (i + 1) >> 1;
    *j = r.j_min + q;
    *c = (i & 1) ? -m : m;
}

// the four counts of placement (j, c) from the prefix sums of a grasp's two histograms (pf[k], pp[k] = the sum of the words below k,
// k = 0 .. kOpenBins) into row[OPEN_BETWEEN .. OPEN_PALM]; true when the placement is FREE.  The ranges lie inside the arrays: see the
// header's proof
template <class PREFIX>
HAF_FRAME_HD bool open_counts(const OpenRules &r, const PREFIX &pf, const PREFIX &pp, int32_t j, int32_t c, int32_t *row)
{
    const int32_t z = kOpenZero + c;
    const uint32_t between = pf[z + j] - pf[z - j], f0 = pf[z - j] - pf[z - j - r.tb], f1 = pf[z + j + r.tb] - pf[z + j];
    const uint32_t palm = pp[z + r.pb] - pp[z - r.pb];
    row[OPEN_BETWEEN] = (int32_t)between; row[OPEN_FINGER0] = (int32_t)f0; row[OPEN_FINGER1] = (int32_t)f1; row[OPEN_PALM] = (int32_t)palm;
    // (every count is at most the frame's 2^28 pixels: the sum of three fits)
    return f0 + f1 + palm <= (uint32_t)r.max_hits && between >= (uint32_t)r.min_between;
}

}  // namespace haf_open_math
