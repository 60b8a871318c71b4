"""Shared by tests/test_prestage_cpu.py and tests/test_prestage_gpu.py: the pre-stage kernels of csrc/prestages.hip against the oracle's
stage functions (hafo_transform, hafo_height_grid, hafo_integral, hafo_mask) on grids up to 1100 x 1100 and on clouds made to hurt.

reference()      heights, integral image and mask per roll from the four stage functions
eval_list()      the evaluation list by its definition (the comment above k_scan, k_compact), in plain numpy
mirror_*()       an independent numpy restatement of the binning and of the integral image: it pins the oracle on the hostile clouds
                 (test_prestage_cpu.py), the GPU tests never use it
expected_forms() a Python mirror of the shape thresholds in launch_small_pre, launch_bin and launch_integral
cases(H)         the seeded cases of a grid size, each (name, H, cfg_kw, in_kw, clouds, rolls): clouds is a list (one request of len(clouds)
                 clouds sharing in_kw), rolls = (first, count)

Every case keeps z + z_shift away from exact +-0: the device's ordered key ranks +0 above -0, the reference keeps the first of two
equal values; reference() asserts that no point of a case lands on a height of +-0 under any of its rolls.
No device is touched here."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from oracle_inputs import oracle_input

F = np.float32
U32 = np.uint32
SIZES = [56, 63, 64, 70, 71, 128, 129, 192, 576, 601, 1100]
STRIP_SIZES = (601, 1100)            # a strip search area: one side the grid's size, the other 200
# 37 does not divide 90, so no two rolls are mirror images of each other; roll 90 of that step is 3330 = 9 * 360 + 90 degrees, the
# 90-degree partner of roll 0 (row_counts)
ROLL_STEP, N_ROLLS, ROLL_90 = 37, 91, 90
Z_SHIFT = 0.15

# launch_small_pre, launch_bin, launch_integral (csrc/prestages.hip)
K_SMALL_PRE_MAX_POINTS = 16384
K_BIN_LDS_CELLS = 16384
K_BIN_CHUNK = 2048
K_BKT_MIN_POINTS = 32768
K_BKT_MAX_BUCKETS = 9216
K_I_SMALL_CELLS = 8192
LDS_LIMIT = 64 * 1024
BIN_GLOBAL, BIN_LDS, BIN_TILES, BIN_FUSED, BIN_LDS_FUSED = range(5)
INTEGRAL_SMALL, INTEGRAL_BAND, INTEGRAL_FUSED = range(3)


def cfg_of(H):
    return dict(grid_h=H, grid_w=H, n_rolls=N_ROLLS, roll_step_deg=ROLL_STEP)


def area_of(H):
    return dict(grasp_area_length_x=H, grasp_area_length_y=200 if H in STRIP_SIZES else H)


def half(H):
    """r_row = r_col of a square grid in metres, as the server computes it (410-411)"""
    return F((0.5 * float(F(H))) / 100.0)


# ---- the thresholds ----------------------------------------------------------------------------------------------------------------

def _pitch(W):
    return (W + 15) // 16 * 16 + 1


def small_pre_lds(H, W):
    return H * _pitch(W) * 8 + H * W * 4 + (H + 1) * (W + 1) * 4 + H * 4


def integral_small_lds(H, W):
    return H * _pitch(W) * 8 + H * W * 4


def bucket_grid(H):
    """bin_bucket_grid -> (buckets per side, bucket edge in cells)"""
    bc = max(H // 64, 8)
    r, bs = 0.005 * H, 0.01 * bc
    rb = r * 1.41422 + bs
    return int(2.0 * rb / bs) + 1, bc


def expected_forms(H, n_points_per_cloud):
    """which kernels serve a request of clouds of these sizes on a square H x H grid (an engine whose max_points holds them) ->
    dict(bin, integral, bucket_refused) as Engine.prestage_forms() reports them"""
    max_n, total_n = max(n_points_per_cloud), sum(n_points_per_cloud)
    if small_pre_lds(H, H) <= LDS_LIMIT:
        return dict(bin=BIN_FUSED if max_n <= K_SMALL_PRE_MAX_POINTS else BIN_LDS_FUSED, integral=INTEGRAL_FUSED, bucket_refused=False)
    nb, _ = bucket_grid(H)
    wanted = H * H > K_BIN_LDS_CELLS and total_n >= K_BKT_MIN_POINTS
    fits = nb * nb + 1 <= K_BKT_MAX_BUCKETS
    if wanted and fits:
        form = BIN_TILES
    elif H * H <= K_BIN_LDS_CELLS and max_n >= 4 * K_BIN_CHUNK:
        form = BIN_LDS
    else:
        form = BIN_GLOBAL
    small = H * H <= K_I_SMALL_CELLS and integral_small_lds(H, H) <= LDS_LIMIT
    return dict(bin=form, integral=INTEGRAL_SMALL if small else INTEGRAL_BAND, bucket_refused=wanted and not fits)


# ---- the oracle's stages -----------------------------------------------------------------------------------------------------------

def _ocfg(cfg_kw):
    return O.make_cfg(H=cfg_kw["grid_h"], W=cfg_kw["grid_w"], n_rolls=cfg_kw["n_rolls"], roll_step_deg=cfg_kw["roll_step_deg"], z_shift=Z_SHIFT)


def transform(cfg_kw, in_kw, roll):
    """hafo_transform -> float32 [16]"""
    M = np.zeros(16, F)
    ocfg, oin = _ocfg(cfg_kw), oracle_input(in_kw)
    O.lib().hafo_transform(C.byref(ocfg), C.byref(oin), roll, 0, M.ctypes.data)
    return M


def reference(cloud, H, cfg_kw, in_kw, rolls):
    """the four stage functions over rolls = (first, count) -> dict(M [R, 16], heights [R, H, H], integral [R, H + 1, H + 1], mask [R, H, H])"""
    cloud = np.ascontiguousarray(cloud, F)
    first, count = rolls
    ocfg, oin = _ocfg(cfg_kw), oracle_input(in_kw)
    out = dict(M=np.zeros((count, 16), F), heights=np.zeros((count, H, H), F), integral=np.zeros((count, H + 1, H + 1), F),
               mask=np.zeros((count, H, H), np.uint8))
    L = O.lib()
    for k in range(count):
        M, h, ii, m = out["M"][k], out["heights"][k], out["integral"][k], out["mask"][k]
        L.hafo_transform(C.byref(ocfg), C.byref(oin), first + k, 0, M.ctypes.data)
        L.hafo_height_grid(C.byref(ocfg), cloud.ctypes.data, cloud.shape[0], cloud.shape[1], M.ctypes.data, h.ctypes.data)
        L.hafo_integral(C.byref(ocfg), h.ctypes.data, ii.ctypes.data)
        L.hafo_mask(C.byref(ocfg), C.byref(oin), first + k, ii.ctypes.data, m.ctypes.data)
        pz = mirror_points(cloud, M)[2]
        assert not (pz == 0).any(), "a height of exactly +-0: the oracle's answer would depend on the order of the points"
    return out


def eval_list(masks):
    """masks [B, R, H, W] -> the evaluation list (cell ids (grid * H + row) * W + col) by its definition: per grid in (cloud, roll) order the
    masked cells of a row from left to right; the row's first cnt % 64 cells go to region B, the rest to region A as whole chunks of 64;
    region A of all rows of all grids comes first, then region B"""
    masks = np.asarray(masks)
    B, R, H, W = masks.shape
    rows = masks.reshape(B * R * H, W)
    a, b = [], []
    for k in np.flatnonzero(rows.any(axis=1)):
        ids = (k * W + np.flatnonzero(rows[k])).astype(np.int32)
        rem = ids.size % 64
        b.append(ids[:rem])
        a.append(ids[rem:])
    return np.concatenate(a + b) if a else np.zeros(0, np.int32)


def row_major_list(mask):
    """one grid's masked cells in row-major order (cell ids inside the grid)"""
    return np.flatnonzero(np.asarray(mask).reshape(-1)).astype(np.int32)


# ---- the independent mirror --------------------------------------------------------------------------------------------------------

def mirror_points(cloud, M):
    """pcl::transformPointCloud as the server uses it: fp32, left to right, unfused -> (px, py, pz)"""
    x, y, z = (np.ascontiguousarray(cloud[:, k], F) for k in range(3))
    M = np.asarray(M, F)
    with np.errstate(all="ignore"):
        p = [((M[4 * k] * x + M[4 * k + 1] * y) + M[4 * k + 2] * z) + M[4 * k + 3] for k in range(3)]
    assert all(q.dtype == F for q in p)
    return p


def mirror_cells(cloud, M, H):
    """-> (index of every point that lands in the grid, its row, its column, its height)"""
    px, py, pz = mirror_points(cloud, M)
    r = half(H)
    with np.errstate(all="ignore"):
        inside = (px > -r) & (px < r) & (py > -r) & (py < r)
        idx = np.flatnonzero(inside)
        ix = np.floor(F(100) * (px[idx] + r)).astype(np.int64)
        iy = np.floor(F(100) * (py[idx] + r)).astype(np.int64)
    ok = (ix >= 0) & (ix < H) & (iy >= 0) & (iy < H)
    return idx[ok], ix[ok], iy[ok], pz[idx[ok]]


def mirror_heights(cloud, M, H, raw=False):
    """max per cell over -1 and the points' heights (a NaN never wins), then every cell below -0.99 becomes 0; raw: before that rule"""
    _, ix, iy, pz = mirror_cells(cloud, M, H)
    keep = ~np.isnan(pz)
    h = np.full(H * H, -1.0, F)
    np.maximum.at(h, ix[keep] * H + iy[keep], pz[keep])
    h = h.reshape(H, H)
    if raw:
        return h
    h = h.copy()
    h[h.astype(np.float64) < -0.99] = 0
    return h


def mirror_integral(h):
    """float64 running row sum plus the row above, narrowed to float32; first row and column zero"""
    H, W = h.shape
    s = np.cumsum(np.cumsum(h.astype(np.float64), axis=1), axis=0)
    ii = np.zeros((H + 1, W + 1), F)
    ii[1:, 1:] = s.astype(F)
    return ii


def mirror_bucket(cloud, H, m0):
    """point_bucket of csrc/prestages.hip in float32: the bucket of every point (or -1); m0 = the transform of roll 0 without x-scale"""
    nb, bc = bucket_grid(H)
    bs = F(0.01) * F(bc)
    rb = F(0.005) * F(H) * F(1.41422) + bs
    inv = F(1.0) / bs
    x, y, z = (np.ascontiguousarray(cloud[:, k], F) for k in range(3))
    m0 = np.asarray(m0, F)
    with np.errstate(all="ignore"):
        x0 = ((m0[0] * x + m0[1] * y) + m0[2] * z) + m0[3]
        y0 = ((m0[4] * x + m0[5] * y) + m0[6] * z) + m0[7]
        fx, fy = (x0 + rb) * inv, (y0 + rb) * inv
        ok = (fx >= 0) & (fx < F(nb)) & (fy >= 0) & (fy < F(nb))
    q = np.full(x.shape, -1, np.int64)
    q[ok] = fy[ok].astype(np.int64) * nb + fx[ok].astype(np.int64)
    return q


def bucket_corner(H, x, y):
    """the lower corner (metres, roll-0 frame without x-scale) and the edge of the bucket that holds (x, y)"""
    nb, bc = bucket_grid(H)
    bs = 0.01 * bc
    rb = 0.005 * H * 1.41422 + bs
    return -rb + np.floor((x + rb) / bs) * bs, -rb + np.floor((y + rb) / bs) * bs, bs


# ---- the clouds --------------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([20250607] + [int(k) for k in key])


def scene(H, n, seed=0, spread=0.98):
    """a friendly cloud: n points uniform over the grid's area, z a smooth surface of 0.03..0.13 m plus noise"""
    rng = _rng(1, H, seed)
    r = float(half(H)) * spread
    x, y = rng.uniform(-r, r, n), rng.uniform(-r, r, n)
    z = 0.08 + 0.04 * np.sin(9.0 * x / max(r, 0.3) + seed) * np.cos(7.0 * y / max(r, 0.3)) + rng.uniform(0.0, 0.01, n)
    return np.stack([x, y, z], axis=1).astype(F)


def _inverse(M):
    return np.linalg.inv(np.asarray(M, np.float64).reshape(4, 4))


def _carry_back(M, px, py, pz):
    """points given in a roll's frame -> float32 points of the input frame, through the float64 inverse of that roll's matrix"""
    p = np.stack([px, py, pz, np.ones_like(px)], axis=0).astype(np.float64)
    return (_inverse(M) @ p)[:3].T.astype(F)


def _case(name, H, clouds, rolls=(0, 3), in_kw=None):
    kw = area_of(H)
    kw.update(in_kw or {})
    return (name, H, cfg_of(H), kw, [np.ascontiguousarray(c, F) for c in clouds], rolls)


def friendly(H, n, rolls=(0, 3)):
    return _case("friendly_%d" % n, H, [scene(H, n)], rolls)


def one_cell(H, rolls=(0, 3)):
    """40 000 points inside a single 1 cm cell, distinct z: one bucket, one address for every atomic"""
    rng = _rng(2, H)
    n = 40000
    bx, by, _ = bucket_corner(H, 0.031, 0.022)
    r = float(half(H))
    # the first grid cell that lies wholly inside that bucket
    cx = (np.ceil((bx + r) * 100 + 0.2) + 0.0) / 100 - r
    cy = (np.ceil((by + r) * 100 + 0.2) + 0.0) / 100 - r
    x, y = cx + rng.uniform(0.001, 0.009, n), cy + rng.uniform(0.001, 0.009, n)
    z = 0.05 + rng.permutation(n) * 1e-6
    pts = np.stack([x, y, z], axis=1).astype(F)
    assert np.unique(pts[:, 2]).size == n
    return _case("one_cell", H, [pts], rolls)


def one_bucket(H, rolls=(0, 3)):
    """40 000 points inside a patch of 8 x 8 cells' size that lies in ONE bucket, plus 2 000 spread points (the first 40 000 rows are the patch)"""
    rng = _rng(3, H)
    n = 40000
    bx, by, _ = bucket_corner(H, 0.031, 0.022)
    x, y = bx + rng.uniform(0.0005, 0.0795, n), by + rng.uniform(0.0005, 0.0795, n)
    z = 0.04 + rng.uniform(0.0, 0.1, n)
    return _case("one_bucket", H, [np.concatenate([np.stack([x, y, z], axis=1).astype(F), scene(H, 2000, seed=3)])], rolls)


def borders(H, rolls=(0, 3), n_back=20000, per_roll=1500):
    """for each roll of the case, lattice points (i / 100 - r, j / 100 - r) of the ROLLED frame, the outermost +-r included, each at
    -2 .. +2 fp32 ulps, carried back through the float64 inverse of that roll's matrix and rounded to float32; behind them a friendly
    background (the first rows are the lattice points)"""
    rng = _rng(4, H)
    cfg_kw, in_kw = cfg_of(H), area_of(H)
    r = half(H)
    parts = []
    for roll in range(rolls[0], rolls[0] + rolls[1]):
        M = transform(cfg_kw, in_kw, roll)
        # the upper part of the grid mostly: there one fp32 ulp of 100 * (p + r) is larger than what the trip through the input frame costs
        i = np.concatenate([rng.integers(H // 3, H + 1, per_roll - 200), rng.integers(0, H + 1, 120), np.zeros(40, np.int64), np.full(40, H)])
        j = np.concatenate([rng.integers(H // 3, H + 1, per_roll - 200), np.zeros(40, np.int64), np.full(40, H), rng.integers(0, H + 1, 120)])
        for ulps in (-2, -1, 0, 1, 2):
            px = (i.astype(np.float64) / 100.0 - float(r)).astype(F)
            py = (j.astype(np.float64) / 100.0 - float(r)).astype(F)
            for _ in range(abs(ulps)):
                px = np.nextafter(px, F(np.inf if ulps > 0 else -np.inf))
                py = np.nextafter(py, F(np.inf if ulps > 0 else -np.inf))
            parts.append(_carry_back(M, px, py, rng.uniform(0.17, 0.3, px.size)))
    return _case("borders", H, [np.concatenate(parts + [scene(H, n_back, seed=4)])], rolls)


def negatives(H, n=40000, rolls=(0, 3)):
    """cells whose maximum lies in (-0.99, 0), cells below -0.99, z of -inf and -1e30, exact duplicates that set a cell's maximum"""
    rng = _rng(5, H)
    pts = scene(H, n, seed=5).astype(np.float64)
    r = float(half(H))
    left, low = pts[:, 0] < -0.45 * r, (pts[:, 0] > 0.45 * r) & (pts[:, 1] < 0)
    pts[left, 2] = -Z_SHIFT - rng.uniform(0.01, 0.8, left.sum())             # heights in (-0.81, -0.01)
    # heights below -0.99: the cell is cleared -- half of them in (-0.999, -0.991), above the -1 of an empty cell, the rest below it
    pts[low, 2] = -Z_SHIFT - np.where(rng.uniform(0, 1, low.sum()) < 0.5, rng.uniform(0.991, 0.999, low.sum()), 1.0 + rng.uniform(0.0, 2.0, low.sum()))
    k = rng.choice(n, 400, replace=False)
    pts[k[:200], 2] = -np.inf
    pts[k[200:], 2] = -1e30
    dup = pts[rng.choice(np.flatnonzero(~left & ~low), 300, replace=False)].copy()
    dup[:, 2] = 0.5                                                          # the same xyz three times, the highest of its cell
    return _case("negatives", H, [np.concatenate([pts, dup, dup, dup])], rolls)


FAR = dict(grasp_area_center=(40.0, -25.0, 1.5), approach_vector=(-0.3, 0.2, 0.9), gripper_opening_width=3)


def far_centre(H, n=40000, rolls=(0, 3)):
    """a search centre tens of metres from the origin, a tilted approach vector and an x-scale of 3; the cloud is generated around that
    centre: a disc of radius 0.31 r in the unscaled frame of roll 0, which every roll keeps inside the grid"""
    rng = _rng(6, H)
    in_kw = dict(area_of(H), **FAR)
    M = transform(cfg_of(H), in_kw, 0)
    rad, ang = 0.31 * float(half(H)) * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    x0, y0 = rad * np.cos(ang), rad * np.sin(ang)
    pz = 0.2 + 0.05 * np.sin(40 * x0) * np.cos(30 * y0) + rng.uniform(0, 0.01, n)
    return _case("far_centre", H, [_carry_back(M, 3.0 * x0, y0, pz)], rolls, FAR)


def bad_values(H, stride, n=40000, rolls=(0, 3)):
    """NaN in each coordinate, +-inf in x and y; rows of `stride` floats, the padding filled with NaN"""
    rng = _rng(7, H)
    pts = scene(H, n, seed=7)
    k = rng.choice(n, 500, replace=False)
    for c in range(3):
        pts[k[100 * c:100 * c + 100], c] = np.nan
    pts[k[300:350], 0], pts[k[350:400], 0] = np.inf, -np.inf
    pts[k[400:450], 1], pts[k[450:500], 1] = np.inf, -np.inf
    wide = np.full((n, stride), np.nan, F)
    wide[:, :3] = pts
    return _case("bad_values_s%d" % stride, H, [wide], rolls)


ROW_TARGETS = (1, 63, 64, 65, 127, 128, 129)
STRIP_H = 0.00175        # 18 cells of a 9 x 9 window sum to 0.0315 > 0.03, the 16 of a window one column short to 0.028, one strip's 9 to 0.016


def row_count_targets(H):
    """the target counts a grid of H cells has room for: a pair of strips takes 17 rows, a row of n masked cells n + 8 columns"""
    fit = [t for t in ROW_TARGETS if t + 8 <= H - 16]
    return fit[:max(1, (H - 14 - 14) // 17)]


def row_counts(H, rolls=(0, 2)):
    """height strips laid out so that the mask of roll 0 has rows of exactly 0, 1, 63, 64, 65, 127, 128 and 129 cells (as many of them
    as the grid has room for: row_count_targets) with empty rows in between.  A target of n cells is a PAIR of strips eight rows apart, each
    n + 8 cells long and 1.75 mm high: only the windows of the row midway hold both strips, and only the n of them that hold nine columns
    of each exceed the mask's 0.03.  Below the last pair a block of tall points keeps the mask of the other rolls from being empty."""
    r = float(half(H))
    targets = row_count_targets(H)
    # in the middle of the grid, where the search rectangle of every roll reaches
    cells, row, col = [], max(7, (H - 17 * len(targets) - 14) // 2), max(8, (H - max(targets) - 8) // 2)
    for t in targets:
        for c in range(col, col + t + 8):
            cells += [(row, c, STRIP_H), (row + 8, c, STRIP_H)]
        row += 17
    if row + 13 <= H - 8:
        cells += [(i, j, 0.1) for i in range(row + 1, row + 13) for j in range(col + 2, col + 14)]
    i, j, h = (np.array(v, np.float64) for v in zip(*cells))
    pts = np.stack([(i + 0.5) / 100 - r, (j + 0.5) / 100 - r, h - Z_SHIFT], axis=1)
    return _case("row_counts" if rolls[0] == 0 else "row_counts_roll%d" % rolls[0], H, [pts], rolls)


def thresholds(H, counts, rolls=(0, 3)):
    """the same scene cut to the point counts at which the form of the binning changes"""
    base = scene(H, max(counts), seed=8)
    return [_case("threshold_%d" % n, H, [base[:n]], rolls) for n in counts]


def uneven_batch(H, rolls=(0, 3)):
    """three clouds in one request: 40 000 points, none, 100"""
    return _case("uneven_batch", H, [scene(H, 40000, seed=9), np.zeros((0, 3), F), scene(H, 100, seed=10, spread=0.6)], rolls)


def empty(H, rolls=(0, 3)):
    return _case("empty", H, [np.zeros((0, 3), F)], rolls)


ALL_COUNTS = (8191, 8192, 16384, 16385, 32767, 32768)


def _all_clouds(H):
    return ([friendly(H, 6000 if small_pre_lds(H, H) <= LDS_LIMIT else 40000), one_cell(H), one_bucket(H), borders(H), negatives(H), far_centre(H),
             bad_values(H, 4), bad_values(H, 8), row_counts(H), row_counts(H, (ROLL_90, 1)), uneven_batch(H)] + thresholds(H, ALL_COUNTS))


_BUILT = {}


def cases(H):
    """the cases of a grid size.  Every cloud runs on a fused grid (56), on 128 (k_bin_lds at exactly 64 KiB of LDS), on 192 (tiles) and
    on 576; a boundary size has one friendly and one hostile cloud; 601 and 1100 have a strip search area, two rolls and 300 000 points"""
    if H not in _BUILT:
        two = (1, 2)
        _BUILT[H] = {
            56: lambda: _all_clouds(56),
            63: lambda: [friendly(63, 6000), borders(63)],                    # the largest fused grid; borders: 42 500 points, k_bin_lds in front
            64: lambda: [friendly(64, 10000), negatives(64, 4000)],           # k_integral_small behind k_bin_lds / k_bin
            70: lambda: [friendly(70, 10000), borders(70)],                   # the largest k_integral_small grid
            71: lambda: [friendly(71, 10000), one_cell(71)],                  # the band form on the smallest grid it serves
            128: lambda: _all_clouds(128),
            129: lambda: [friendly(129, 40000), borders(129)],                # 3 x 3 tiles, the last row and column one cell wide
            192: lambda: _all_clouds(192),
            576: lambda: [friendly(576, 100000, two), one_cell(576, two), one_bucket(576, two), borders(576, two), negatives(576, rolls=two),
                          far_centre(576, rolls=two), bad_values(576, 4, rolls=two), bad_values(576, 8, rolls=two), row_counts(576),
                          row_counts(576, (ROLL_90, 1)), uneven_batch(576, two)] + thresholds(576, (32767, 32768), two),
            601: lambda: [friendly(601, 300000, (0, 2)), one_bucket(601, (0, 2))],
            1100: lambda: [friendly(1100, 300000, (0, 2)), one_cell(1100, (0, 2))],
        }[H]()
    return _BUILT[H]


_REFS = {}


def case_reference(case):
    """reference() of every cloud of the case, computed once -> dict(per_cloud: [reference dict], masks [B, R, H, H], list: eval_list)"""
    name, H, cfg_kw, in_kw, clouds, rolls = case
    if (name, H) not in _REFS:
        per = [reference(c, H, cfg_kw, in_kw, rolls) for c in clouds]
        masks = np.stack([p["mask"] for p in per])
        _REFS[name, H] = dict(per_cloud=per, masks=masks, list=eval_list(masks))
    return _REFS[name, H]


def engine_kw(H):
    """the haf_config fields an engine needs to serve every case of the size, and no more"""
    cs = cases(H)
    return dict(cfg_of(H), max_clouds=max(len(c[4]) for c in cs), max_points=max(sum(len(x) for x in c[4]) for c in cs),
                max_rolls_per_call=max(c[5][1] for c in cs))
