// space_rules.h -- the per-sample rules of haf_check_space (include/hafgrasp.h), written once: the lattice of sample points inside the
// gripper's four boxes, a sample's point in the base frame, a depth pixel's observed word, and the state of a sample in one view.
//
// The same source is compiled for the device (space.hip) and for the host (space_host.cpp: haf_check_space_ref, the definition of
// record), on top of clearance_rules.h -- whose grasp words and gripper bounds these are -- and of transfer_rules.h -- whose projection
// into a pinhole image (transfer_project) is used unchanged -- and frame_points.h's depth rule.  Only transfer_project's transform into
// the camera's frame is floating point, twelve rounded fp32 operations; everything else here is integer arithmetic, so no result depends
// on an order of evaluation, and the counts are integer sums, which do not depend on the order in which atomics arrive.
//
// Units.  A lattice coordinate s, t, u is in units of 2^-26 m, the unit of every bound W(x) of clearance_rules.h.  A sample's point is
//     P_j = o_j 2^28 + s C_j + t B_j + u A_j,   int64, units of 2^-40 m
// (o: 1/4096 m, so o 2^28 is 2^-40 m; an axis word is 2^-14, so s C is 2^-26 x 2^-14 = 2^-40 m).
// Why nothing overflows.  |o_j| <= 2^16, so |o_j 2^28| <= 2^44.  gripper_rules refuses a reach above 1 m, so every bound is at most
// 2^26 + 2 in magnitude (one rounded W or the sum of two) and so is every lattice coordinate, which lies between two bounds; an axis word
// is at most 16384: |s C_j + t B_j + u A_j| <= 3 (2^26 + 2) 2^14 < 2^42.  |P_j| < 2^44 + 2^42 < 2^45.  Pq_j = (P_j + 2^23) >> 24 is a
// word of 1/65536 m with |Pq_j| < 2^21, exact as a float, and p_j = (float)Pq_j * (1 / 65536) is exact too.
// A lattice coordinate: (2k + 1)(hi - lo) <= 2 x 65536 x (2^27 + 4) < 2^45, int64.
#pragma once
#include "clearance_rules.h"
#include "transfer_rules.h"

namespace haf_space_math {

using namespace haf_clear_math;
using namespace haf_transfer_math;

enum { SPACE_BETWEEN = 0, SPACE_FINGER0 = 1, SPACE_FINGER1 = 2, SPACE_PALM = 3, SPACE_REGIONS = 4 };
// a sample's state, and its rank when the views are merged: the maximum wins
enum { SPACE_UNSEEN = 0, SPACE_HIDDEN = 1, SPACE_FREE = 2, SPACE_HIT = 3, SPACE_STATES = 4 };
enum { SPACE_AXIS_S = 0, SPACE_AXIS_T = 1, SPACE_AXIS_U = 2 };

constexpr int kSpaceRowWords = SPACE_REGIONS * SPACE_STATES;     // a grasp's row: n[region][state]
constexpr int32_t kSpaceFarWord = 1 << 20;                // the observed word of a valid depth above 16 m
constexpr int kSpaceMaxViews = 8;                         // HAF_MAX_SPACE_VIEWS
constexpr int32_t kSpaceMaxSamples = 65536;               // HAF_MAX_SPACE_SAMPLES

// the call's lattice, the same for every grasp, formed ONCE per call on the host (space_lattice of space_host.cpp): per region and axis
// (s, t, u) the box [lo, hi] and the number of samples n; first[r] = the index of region r's first sample, first[4] = N
struct SpaceLattice {
    int32_t S;                                            // W(sample_step)
    int32_t lo[SPACE_REGIONS][3], hi[SPACE_REGIONS][3], n[SPACE_REGIONS][3];
    int32_t first[SPACE_REGIONS + 1];
};

// one view as the rules read it: the projection's constants (transfer_rules of transfer_host.cpp, for the camera the view is), the
// constants of its depth rule (frame_math of frames_host.cpp) and its kind
struct SpaceViewRules {
    TransferRules r;
    haf_frame_math::FrameMath m;
    int32_t kind, pad;
};

// sample k of n on [lo, hi]: both divisions truncate on non-negative operands
HAF_FRAME_HD int32_t space_coord(int32_t lo, int32_t hi, int32_t n, int32_t k)
{
    return (int32_t)((int64_t)lo + ((int64_t)(2 * k + 1) * ((int64_t)hi - (int64_t)lo)) / (int64_t)(2 * n));
}

// sample j < N: its region and its three coordinates.  Region-major, then u, then t, with s fastest
HAF_FRAME_HD int space_sample(const SpaceLattice &l, int32_t j, int32_t *stu)
{
    int r = 0;
    while (r + 1 < SPACE_REGIONS && j >= l.first[r + 1]) r++;
    const uint32_t local = (uint32_t)(j - l.first[r]), ns = (uint32_t)l.n[r][SPACE_AXIS_S], nt = (uint32_t)l.n[r][SPACE_AXIS_T];
    const uint32_t row = local / ns, ks = local - row * ns, ku = row / nt, kt = row - ku * nt;
    stu[0] = space_coord(l.lo[r][0], l.hi[r][0], (int32_t)ns, (int32_t)ks);
    stu[1] = space_coord(l.lo[r][1], l.hi[r][1], (int32_t)nt, (int32_t)kt);
    stu[2] = space_coord(l.lo[r][2], l.hi[r][2], l.n[r][SPACE_AXIS_U], (int32_t)ku);
    return r;
}

// the sample's point in the base frame: Pq, words of 1/65536 m, and p, the same as floats (exact)
HAF_FRAME_HD void space_point(const GraspWords &g, const int32_t *stu, int32_t *Pq, float *p)
{
    for (int j = 0; j < 3; j++) {
        const int64_t P = (int64_t)g.o[j] * ((int64_t)1 << 28) + (int64_t)stu[0] * g.c[j] + (int64_t)stu[1] * g.b[j] + (int64_t)stu[2] * g.a[j];
        Pq[j] = (int32_t)((P + ((int64_t)1 << 23)) >> 24);      // (an arithmetic shift)
        p[j] = f_mul((float)Pq[j], 1.0f / kTransferQuantum);
    }
}

// a depth pixel's observed word by frame_points.h's depth rule; raw: the 2 or 4 bytes of the sample.  false: the pixel is invalid
HAF_FRAME_HD bool space_observed(const SpaceViewRules &v, uint32_t raw, int32_t &Zobs)
{
    float z;
    bool ok;
    if (v.kind == HAF_FRAME_DEPTH_U16) {
        const uint32_t d = raw & 0xFFFFu;
        z = f_mul((float)d, v.m.depth_scale);
        ok = d != 0 && haf_frame_math::depth_in_range(z, v.m);
    } else {
        const float d = f_from_bits(raw);
        z = f_mul(d, v.m.depth_scale);
        ok = f_finite(d) && d > 0.0f && haf_frame_math::depth_in_range(z, v.m);
    }
    Zobs = !ok ? 0 : (z > 16.0f ? kSpaceFarWord : metre_word(z));
    return ok;
}

// a sample of depth word Qz at a valid pixel whose observed word is Zobs
HAF_FRAME_HD int space_state(const TransferRules &r, int32_t Qz, int32_t Zobs)
{
    const int64_t tol = (int64_t)r.TA + (((int64_t)r.TR * (int64_t)Zobs) >> 16), D = (int64_t)Qz - (int64_t)Zobs;
    return D > tol ? SPACE_HIDDEN : (D < -tol ? SPACE_FREE : SPACE_HIT);
}

}  // namespace haf_space_math
