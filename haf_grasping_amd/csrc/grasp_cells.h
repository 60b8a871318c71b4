// grasp_cells.h -- the cell of a roll's 1 cm grid that a base-frame point falls into, and the best vote over a request's rolls: THE
// arithmetic of haf_point_cells / haf_grasp_map_ref (include/hafgrasp.h), written once.
//
// Compiled for the host (graspmap_host.cpp: the definition of record) and for the device (graspmap.hip: k_grasp_map), as frame_points.h
// is.  The cell arithmetic is k_bin's (prestages.hip; server.cpp:488, 510-514): rows 0..2 of the roll's fp32 transform, each
// ((m0 x + m1 y) + m2 z) + m3 left to right, every step ONE correctly rounded fp32 operation and never a fused multiply-add; the strict
// range tests on the transformed x and y and "z is not a NaN"; floorf(100 (p + r)) and the index range test.
#pragma once
#include "frame_points.h"

#include <math.h>

namespace haf_cell_math {

using haf_frame_math::f_add;
using haf_frame_math::f_finite;
using haf_frame_math::f_mul;

constexpr int kNoCellVote = -32768;          // HAF_MAP_NO_CELL

// what the cell arithmetic reads of one roll: rows 0..2 of RollGeo::m, padded to 64 bytes (sixteen scalar registers per roll)
struct CellGeo {
    float m[12];
    float pad[4];
};

// row * W + col of point (x, y, z) under the roll whose transform is m, or -1.  r_row, r_col: pick_rules.h's cell_reach(H, W)
HAF_FRAME_HD int32_t point_cell(const float *m, float x, float y, float z, float r_row, float r_col, int H, int W)
{
    const float px = f_add(f_add(f_add(f_mul(m[0], x), f_mul(m[1], y)), f_mul(m[2], z)), m[3]);
    const float py = f_add(f_add(f_add(f_mul(m[4], x), f_mul(m[5], y)), f_mul(m[6], z)), m[7]);
    const float pz = f_add(f_add(f_add(f_mul(m[8], x), f_mul(m[9], y)), f_mul(m[10], z)), m[11]);
    if (!((px > -r_row) && (px < r_row) && (py > -r_col) && (py < r_col) && (pz == pz))) return -1;
    const int ix = (int)floorf(f_mul(100.0f, f_add(px, r_row)));
    const int iy = (int)floorf(f_mul(100.0f, f_add(py, r_col)));
    if (!(ix >= 0 && ix < H && iy >= 0 && iy < W)) return -1;
    return ix * W + iy;
}

// a pixel of a grasp map takes part when its point is finite in every component (the rule of haf_view_points)
HAF_FRAME_HD bool point_usable(const float *p) { return f_finite(p[0]) && f_finite(p[1]) && f_finite(p[2]); }

}  // namespace haf_cell_math
