"""Shared by tests/test_cell_segment_cpu.py and tests/test_cell_segment_gpu.py: an independent numpy mirror of haf_segment_cells_ref
(include/hafgrasp.h) and the clouds and frames both suites run it on.  The points are frame_cases.mirror_points'; every floating-point
step is numpy float32 arithmetic, one rounded operation each; the components come from a flood fill over a dictionary of occupied
cells, the numbering and the infos from recounting -- nothing here shares code or method with csrc/cellsegment_host.cpp (a sequential
union-find over the whole grid) or csrc/cellsegment.hip."""
import numpy as np

import frame_cases as fc
from haf_grasping_amd import capi

F = np.float32
# (nx, ny): one cell; one short of a 64 x 16 tile; the tile exactly; one over each way; more than two tiles each way; one row; one column
GRIDS = [(1, 1), (63, 15), (64, 16), (65, 17), (130, 33), (4096, 1), (1, 4096)]
CELL = 0.01
LOW, HIGH = 0.050, 0.120                                 # two object heights above the plane z = 0 (a 7 cm step)
PATTERNS = ["random", "serpentine", "checker", "diag_dr", "diag_dl", "full"]


def height_key(h):
    """float32 array -> int64 keys ordered as the floats, -0 below +0"""
    b = h.astype(F).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, b ^ 0x7FFFFFFF)


def key_height(k):
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k, k ^ 0x7FFFFFFF).astype(np.int32).view(F)


def point_cells(frame, image, p):
    """-> (fg [n], cell [n] (-1: none), key [n]): the definition's per-point rules in numpy float32"""
    w = fc.mirror_points(frame, image)
    pts = w.view(F)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    usable = ((w & np.uint32(0x7FFFFFFF)) <= np.uint32(0x41800000)).all(axis=1)
    a, b, c, d = (F(v) for v in p.plane)
    with np.errstate(all="ignore"):
        h = ((a * x + b * y) + c * z) + d
        assert h.dtype == F
        fg = usable & ~np.isnan(h) & (h >= F(p.min_height))
        if F(p.max_height) > 0:
            fg &= h <= F(p.max_height)
        inv = F(1) / F(p.cell)
        assert type(inv) is F
        fx, fy = (x - F(p.x0)) * inv, (y - F(p.y0)) * inv
        assert fx.dtype == F
        inside = fg & (fx >= 0) & (fx < F(p.nx)) & (fy >= 0) & (fy < F(p.ny))
        ix, iy = np.floor(np.where(inside, fx, 0)).astype(np.int64), np.floor(np.where(inside, fy, 0)).astype(np.int64)
    return fg, np.where(inside, iy * p.nx + ix, -1), height_key(h)


def mirror_cells(frame, image, p, dtype=np.uint8):
    """haf_segment_cells_ref in numpy -> (labels [H, W] of dtype, infos, stats, cell_labels [ny, nx] uint16)"""
    H, W = image.shape[:2]
    nx, ny = p.nx, p.ny
    fg, cell, key = point_cells(frame, image, p)
    count, top = {}, {}
    for c, k in zip(cell[cell >= 0].tolist(), key[cell >= 0].tolist()):
        count[c] = count.get(c, 0) + 1
        top[c] = max(top.get(c, k), k)
    step = F(p.max_step)

    def linked(a, b):
        if not step > 0:
            return True
        with np.errstate(all="ignore"):
            return bool(np.abs(key_height(top[a]) - key_height(top[b])) <= step)
    offs = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (-1, 1), (1, -1), (-1, -1)] if p.connectivity == 8 else [])
    comp = {}
    members = []                                          # per component in ascending order of anchor: its cells
    for c in sorted(count):
        if c in comp:
            continue
        comp[c] = len(members)
        todo, mine = [c], []
        while todo:
            a = todo.pop()
            mine.append(a)
            ax, ay = a % nx, a // nx
            for dx, dy in offs:
                bx, by = ax + dx, ay + dy
                if 0 <= bx < nx and 0 <= by < ny:
                    b = by * nx + bx
                    if b in count and b not in comp and linked(a, b):
                        comp[b] = comp[c]
                        todo.append(b)
        members.append(mine)
    infos, label_of, kept = [], {}, 0
    for mine in members:
        pts = sum(count[a] for a in mine)
        if pts < p.min_points:
            continue
        kept += 1
        if kept > p.max_labels:
            continue
        xs, ys = [a % nx for a in mine], [a // nx for a in mine]
        anchor = min(mine)
        infos.append((pts, len(mine), anchor % nx, anchor // nx, min(xs), min(ys), max(xs), max(ys), key_height(max(top[a] for a in mine))))
        for a in mine:
            label_of[a] = kept
    grid = np.zeros(nx * ny, np.uint16)
    for a, l in label_of.items():
        grid[a] = l
    labels = np.array([label_of.get(c, 0) for c in cell.tolist()], np.int64).reshape(H, W)
    stats = [H * W, int(fg.sum()), int((fg & (cell < 0)).sum()), len(count), len(members), kept]
    return labels.astype(dtype), np.array(infos, capi.CELL_SEGMENT_INFO_DTYPE), stats, grid.reshape(ny, nx)


def same(a, b):
    """two results agree in every label word, info field, stat and (when both carry one) cell_labels word"""
    ok = a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes() and list(a[2]) == list(b[2])
    if len(a) > 3 and len(b) > 3:
        ok = ok and a[3].dtype == b[3].dtype and a[3].shape == b[3].shape and (a[3] == b[3]).all()
    return bool(ok)


# ---- clouds planted on a grid ------------------------------------------------------------------------------------------------------

def grid_kw(nx, ny, **over):
    kw = dict(plane=[0, 0, 1, 0], min_height=0.01, max_height=0.0, cell=CELL, x0=0.0, y0=0.0, nx=nx, ny=ny, connectivity=8, max_step=0.0,
              min_points=1, max_labels=255)
    kw.update(over)
    return kw


def cloud_of(cells, rng=None, cell=CELL, x0=0.0, y0=0.0):
    """cells: [(ix, iy, height, points)] -> float32 [N, 3]: every point well inside its cell, one of them at the cell's height and the
    others up to 5 mm below; shuffled when an rng is given"""
    out = []
    for k, (ix, iy, h, n) in enumerate(cells):
        for j in range(n):
            fx, fy = (0.25 + 0.5 * ((k * 7 + j * 3) % 11) / 10.0), (0.25 + 0.5 * ((k * 5 + j) % 7) / 6.0)
            out.append((x0 + (ix + fx) * cell, y0 + (iy + fy) * cell, h - 0.001 * (j % 5)))
    xyz = np.array(out, F).reshape(-1, 3)
    if rng is not None:
        xyz = xyz[rng.permutation(len(xyz))]
    return np.ascontiguousarray(xyz)


def occupancy(pattern, nx, ny, rng):
    """-> (occupied [ny, nx] bool, height [ny, nx]) or None when the pattern does not apply to the grid"""
    u, v = np.meshgrid(np.arange(nx), np.arange(ny))
    occ = np.zeros((ny, nx), bool)
    hm = np.full((ny, nx), LOW)
    if pattern == "random":                               # ~55 % occupied, 9 x 7 blocks of two heights
        occ = rng.random((ny, nx)) < 0.55
        hm = np.where((u // 9 + v // 7) % 2 == 0, LOW, HIGH)
    elif pattern == "serpentine":                         # one cell wide through every row
        if ny == 1 or nx == 1:
            occ[:] = True
        else:
            occ[0::2, :] = True
            occ[1::4, nx - 1] = True
            occ[3::4, 0] = True
    elif pattern == "checker":
        occ = (u + v) % 2 == 0
    elif pattern in ("diag_dr", "diag_dl"):               # a staircase of corner links through the corner of tile (0, 0): (63, 15) -> (64, 16)
        if nx < 2 or ny < 2:
            return None
        k = np.arange(ny)
        xs = (48 + k) if pattern == "diag_dr" else (79 - k)
        if nx < 80:
            xs = k if pattern == "diag_dr" else nx - 1 - k
        ok = (xs >= 0) & (xs < nx)
        occ[k[ok], xs[ok]] = True
    elif pattern == "full":
        occ[:] = True
    else:
        raise KeyError(pattern)
    return occ, hm


def grid_case(pattern, nx, ny, seed=0, **over):
    """-> (name, frame, image [1, N, 3], params kw) or None: a shuffled N x 1 cloud planted on the pattern's cells, 1..3 points each"""
    rng = np.random.default_rng([seed, PATTERNS.index(pattern), nx, ny])
    got = occupancy(pattern, nx, ny, rng)
    if got is None:
        return None
    occ, hm = got
    ys, xs = np.nonzero(occ)
    cells = [(int(x), int(y), float(hm[y, x]), 1 + (int(x) * 3 + int(y)) % 3) for x, y in zip(xs, ys)]
    kw = grid_kw(nx, ny, **over)
    if max(nx, ny) == 4096:                               # 4096 cells of 5 mm about the origin: every point within the usable 16 m
        kw.update(cell=0.005, x0=-10.24 if nx == 4096 else 0.0, y0=-10.24 if ny == 4096 else 0.0)
    xyz = cloud_of(cells, rng, kw["cell"], kw["x0"], kw["y0"])
    if len(xyz) == 0:
        xyz = np.zeros((1, 3), F)
    if pattern == "random":
        kw.update(max_step=0.03, min_points=3)
        kw.update(over)
    image = xyz.reshape(1, -1, 3)
    return ("%s_%dx%d" % (pattern, nx, ny), capi.xyz_frame(image), image, kw)


def grid_cases(grids=None):
    """every pattern on every grid it applies to, with 8-connectivity; the checkerboard and the staircases with 4-connectivity too"""
    out = []
    for nx, ny in grids or GRIDS:
        for pattern in PATTERNS:
            for conn in (8, 4) if pattern in ("checker", "diag_dr", "diag_dl", "random") else (8,):
                c = grid_case(pattern, nx, ny, connectivity=conn, max_labels=capi.MAX_LABELS)
                if c is not None:
                    out.append((c[0] + "_c%d" % conn,) + c[1:])
    return out


def rule_cases():
    """the rules one at a time -> [(name, frame, image, params kw, expected (n_labels, stats[4], stats[5]))]"""
    out = []

    def add(name, cells, want, **kw):
        xyz = cloud_of(cells)
        image = xyz.reshape(1, -1, 3)
        out.append((name, capi.xyz_frame(image), image, grid_kw(16, 8, **kw), want))
    plateaus = [(x, y, LOW if x < 4 else HIGH, 2) for x in range(8) for y in range(3)]
    add("plateaus_split_by_max_step", plateaus, (2, 2, 2), max_step=0.03)
    add("plateaus_joined_without_max_step", plateaus, (1, 1, 1), max_step=0.0)
    add("plateaus_joined_by_a_wide_max_step", plateaus, (1, 1, 1), max_step=0.08)
    # the size rule counts points: one cell of 50 points is kept, 49 linked cells of one point each are dropped
    sizes = [(15, 7, LOW, 50)] + [(x, y, LOW, 1) for y in range(4) for x in range(13)][:49]
    add("min_points_counts_points", sizes, (1, 2, 1), min_points=50)
    singles = [(x, y, LOW, 1) for y in range(0, 8, 2) for x in range(0, 16, 2)]
    add("max_labels_cap", singles, (5, 32, 32), max_labels=5)
    add("all_points_in_one_cell", [(3, 2, HIGH, 40)], (1, 1, 1))
    add("below_min_height_is_empty", [(3, 2, 0.005, 4)], (0, 0, 0))
    nan = np.full((1, 1, 3), np.nan, F)
    out.append(("empty_cloud", capi.xyz_frame(nan), nan, grid_kw(16, 8), (0, 0, 0)))
    return out


def frame_cases():
    """frames of other shapes and kinds on the default 1024 x 1024 grid: the patterns of segment_cases under both poses -> [(name,
    frame, image, params kw)]"""
    import segment_cases as sc
    out = []
    for shape in ((13, 7), (61, 5)):
        for kind in sc.KINDS:
            for tilted in (False, True):
                frame, image, kw = sc.make_case("random", kind, shape, tilted)
                out.append(("random_%s_%dx%d_%s" % (kind, shape[0], shape[1], "tilted" if tilted else "identity"), frame, image,
                            dict(plane=kw["plane"], min_height=0.01, max_height=0.2, min_points=2, max_step=0.03)))
    return out


def line_cases():
    """N x 1 clouds, N = 1, 63, 65, 1000: points scattered over a 40 x 25 cm patch of the default grid at three heights"""
    out = []
    for n in (1, 63, 65, 1000):
        rng = np.random.default_rng([7, n])
        xyz = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(0.0, 0.25, n), rng.choice([0.0, LOW, HIGH], n)], axis=1).astype(F)
        image = np.ascontiguousarray(xyz).reshape(1, n, 3)
        out.append(("line_%d" % n, capi.xyz_frame(image), image, dict(min_points=1, max_step=0.03, cell=0.02, max_labels=capi.MAX_LABELS)))
    return out
