// pick_rules.h -- the rules of the pick path, written once: the key a pixel competes with, which pixels compete, how far a grid reaches
// from its centre, and the z window of a cell.  Every call that answers from the vote grids of the last scored batch uses them:
// haf_grasp_map_best, haf_grasp_map_labels, haf_score_objects, haf_cell_pose, haf_top_grasps and the roll record of the vote itself.
//
// Compiled for the host (graspmap_host.cpp: the definitions of record; the engine_*.cpp units) and for the device (vote.hip,
// graspmap.hip, topgrasps.hip), as grasp_cells.h is.  Integer work but for one fp32 comparison and cell_reach, whose double
// intermediate is part of its definition.
#pragma once
#include "grasp_cells.h"
#include "label_shape.h"

namespace haf_pick_math {

using haf_cell_math::kNoCellVote;
using haf_shape_math::height_key;          // the ordered key of a height, for host and device (label_shape.h)
using haf_shape_math::key_height;

// THE pick key.  Most significant first: vote + 32768 (16 bits), 65535 - roll (16 bits), 2^32 - 1 - pixel index (32 bits).  The
// maximum over a set of pixels is therefore the one with the largest vote, then the lowest roll, then the lowest pixel index v * width
// + u (v, then u ascending).  0 is no pixel's key: a pixel that qualifies has a vote above kNoCellVote, so its top 16 bits are not zero
HAF_FRAME_HD unsigned long long pick_key(int vote, int roll, unsigned pixel)
{
    return ((unsigned long long)(unsigned)(vote + 32768) << 48) | ((unsigned long long)(unsigned)(65535 - roll) << 32) |
           (unsigned long long)(0xFFFFFFFFu - pixel);
}
HAF_FRAME_HD int pick_key_vote(unsigned long long key) { return (int)(key >> 48) - 32768; }
HAF_FRAME_HD int pick_key_roll(unsigned long long key) { return 65535 - (int)((key >> 32) & 0xFFFFull); }
HAF_FRAME_HD unsigned pick_key_pixel(unsigned long long key) { return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull); }

// a pixel of a grasp map competes for a pick when it has a roll and its vote reaches min_vote (and is a vote at all)
HAF_FRAME_HD bool pick_qualifies(int vote, int roll, int min_vote) { return roll >= 0 && vote >= min_vote && vote > kNoCellVote; }

// how far an H x W grid of 1 cm cells reaches from its centre, in metres (server.cpp:410-411): formed in double, then rounded once
HAF_FRAME_HD void cell_reach(int H, int W, float *r_row, float *r_col)
{
    *r_row = (float)((0.5 * (float)H) / 100.0);
    *r_col = (float)((0.5 * (float)W) / 100.0);
}

// The z window of cell (row, col): rows row-4..row+4, cols col-4..col+3, clipped to the grid -- kZWindowSlots slots in row-major order
// (server.cpp:1342-1351).  z_window_slot: the cell (rr, cc) of slot q, false when it lies outside the grid.  The window's value is the
// maximum above -10 under the ordered key: start from z_window_start(), fold every slot's height in, take key_height of the result
constexpr int kZWindowSlots = 72;
HAF_FRAME_HD bool z_window_slot(int q, int row, int col, int H, int W, int *rr, int *cc)
{
    *rr = row + q / 8 - 4;
    *cc = col + q % 8 - 4;
    return *rr >= 0 && *cc >= 0 && *rr < H && *cc < W;
}
HAF_FRAME_HD int32_t z_window_start() { return height_key(-10.0f); }
HAF_FRAME_HD int32_t z_window_fold(int32_t zk, float h)
{
    if (!(-10.0f < h)) return zk;
    const int32_t k = height_key(h);
    return k > zk ? k : zk;
}

}  // namespace haf_pick_math
