"""Shared by tests/test_grasp_map_cpu.py and tests/test_grasp_map_gpu.py: an independent numpy-fp32 mirror of the per-pixel grasp map
(include/hafgrasp.h: haf_point_cells, haf_grasp_map_ref) built on the CPU oracle's own roll transforms `M` and vote grids `graspseval`,
and the frames both suites run it on.  numpy float32 arithmetic rounds every operation, so the mirror, the host definition and the
device kernel must agree in every pixel."""
import numpy as np

import frame_cases as fc
from haf_grasping_amd import capi

F = np.float32
NO_CELL = -32768


def half_extent(cells):
    return F((0.5 * float(F(cells))) / 100.0)


def mirror_transform(m16, pts):
    """rows 0..2 of the oracle's 4x4 `m16` applied to float32 [N, 3] points: ((m0 x + m1 y) + m2 z) + m3, every step rounded to fp32"""
    m = np.asarray(m16, dtype=F).reshape(-1)
    x, y, z = (np.ascontiguousarray(pts[:, k], dtype=F) for k in range(3))
    with np.errstate(all="ignore"):
        out = [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)]
    assert all(o.dtype == F for o in out)
    return out


def mirror_cells(m16, pts, H, W):
    """-> (int64 [N] cell row * W + col or -1, float32 [N] transformed z)"""
    px, py, pz = mirror_transform(m16, pts)
    r_row, r_col = half_extent(H), half_extent(W)
    with np.errstate(all="ignore"):
        ok = (px > -r_row) & (px < r_row) & (py > -r_col) & (py < r_col) & (pz == pz)
        ix = np.floor(F(100.0) * (px + r_row))
        iy = np.floor(F(100.0) * (py + r_col))
    ix = np.where(ok, ix, -1).astype(np.int64)
    iy = np.where(ok, iy, -1).astype(np.int64)
    ok &= (ix >= 0) & (ix < H) & (iy >= 0) & (iy < W)
    return np.where(ok, ix * W + iy, -1), pz


def mirror_map(Ms, grids, roll_first, words, H, W):
    """The expectation: Ms [R, 16] and grids [R, H, W] of the rolls roll_first .., words uint32 [N, 3] of the pixels' points
    (frame_cases.mirror_points) -> (vote int16 [N], roll int16 [N], cell int32 [N])"""
    pts = np.ascontiguousarray(words, dtype=np.uint32).view(F).reshape(-1, 3)
    usable = np.isfinite(pts).all(axis=1)
    n = pts.shape[0]
    vote, roll, cell = np.full(n, NO_CELL, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for r in range(len(Ms)):
        c, _ = mirror_cells(Ms[r], pts, H, W)
        c = np.where(usable, c, -1)
        has = c >= 0
        val = np.full(n, NO_CELL, np.int64)
        val[has] = np.asarray(grids[r], dtype=F).reshape(-1)[c[has]].astype(np.int64)
        take = has & ((roll < 0) | (val > vote))
        vote[take], roll[take], cell[take] = val[take], roll_first + r, c[take]
    return vote.astype(np.int16), roll.astype(np.int16), cell.astype(np.int32)


def assert_map_equal(got, want, name):
    """got: dict of [height, width] images, want: the (vote, roll, cell) tuple of mirror_map"""
    for k, w in zip(("vote", "roll", "cell"), want):
        g = got[k].reshape(-1)
        bad = np.flatnonzero(g != w)
        assert g.shape == w.shape and bad.size == 0, (name, k, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


def organised(xyz, width=640, floats=3):
    """a cloud as an organised float32 [height, width, floats] image, the tail padded with NaN points"""
    n = len(xyz)
    h = (n + width - 1) // width
    img = np.full((h, width, floats), np.nan, F)
    img.reshape(-1, floats)[:n, :3] = xyz[:, :3]
    return img


def key_argmax(vote, roll, mask, min_vote):
    """The best pixel in key order -- vote descending, roll ascending, v ascending, u ascending -- among the pixels the mask selects
    (None: all) that have a cell and a vote >= min_vote -> (u, v) or None"""
    v, r = vote.astype(np.int64), roll.astype(np.int64)
    ok = (r >= 0) & (v >= min_vote)
    if mask is not None:
        ok &= mask != 0
    idx = np.flatnonzero(ok.reshape(-1))
    if idx.size == 0:
        return None
    order = np.lexsort((idx, r.reshape(-1)[idx], -v.reshape(-1)[idx]))
    i = int(idx[order[0]])
    return i % vote.shape[1], i // vote.shape[1]
