"""Shared by tests/test_vote_cpu.py and tests/test_vote_gpu.py: an independent numpy mirror of the vote and of the record rule on top of
it (server.cpp:865-932, 1342-1351) -- the 29-tap sum of an int8 label grid, the same sum of a float32 grid in fp32 and source order,
the int record (first-wins argmax, longest run, smaller row, end - len/2), the float record with its truncating running maximum, the
form gated by a cell set S -- and the named synthetic grids both suites run it on.  No GPU and no engine.

Every builder returns Case objects: a name, the grid, and `claim`, the properties the case is there for (read back from the mirror by
test_vote_cpu.py, so a case that stops exercising its edge fails on the CPU).  Label values stay in [-9, 99]; -1 is "unlabelled"."""
import numpy as np

import roi_cases as rc

F = np.float32
# (weight, dr, dc) in the order the source adds them (server.cpp:873-878)
WEIGHTS = ([(w, -2, dc) for w, dc in zip((1, 2, 3, 2, 1), range(-2, 3))] + [(w, -1, dc) for w, dc in zip((2, 3, 4, 3, 2), range(-2, 3))] +
           [(w, 0, dc) for w, dc in zip((2, 2, 3, 4, 55, 4, 3, 2, 2), range(-4, 5))] +
           [(w, 1, dc) for w, dc in zip((2, 3, 4, 3, 2), range(-2, 3))] + [(w, 2, dc) for w, dc in zip((1, 2, 3, 2, 1), range(-2, 3))])
assert len(WEIGHTS) == 29 and sum(w for w, _, _ in WEIGHTS) == 123 and {(dr, dc) for _, dr, dc in WEIGHTS} == set(rc.TAPS)
SIZES = (15, 56, 61, 128, 131, 132, 136)      # tests/test_vote_gpu.py says which kernel path each one is the smallest grid of
FLOAT_SIZES = (56, 136)
BLOCK = 2048                                  # cells per workgroup of the large-grid vote kernel


class Case:
    def __init__(self, name, grid, heights=None, **claim):
        self.name, self.grid, self.heights, self.claim = name, grid, heights, claim

    def __repr__(self):
        return "Case(%s %s)" % (self.name, "x".join(map(str, self.grid.shape)))


# ---------------------------------------------------------------- the mirror ----------------------------------------------------------------

def vote_int(g, S=None):
    """int8 [H, W] labels -> int64 [H, W] votes: 0 on the border (rows 0, 1, H-2, H-1, cols 0..3, W-4..W-1), 0 where the label is
    negative, 0 outside the cell set S (bool [H, W]) if one is given, else the 29-tap sum"""
    g = np.asarray(g).astype(np.int64)
    H, W = g.shape
    ev = np.zeros((H, W), np.int64)
    acc = np.zeros((H - 4, W - 8), np.int64)
    for w, dr, dc in WEIGHTS:
        acc += w * g[2 + dr:H - 2 + dr, 4 + dc:W - 4 + dc]
    ev[2:H - 2, 4:W - 4] = np.where(g[2:H - 2, 4:W - 4] < 0, 0, acc)
    if S is not None:
        ev[~np.asarray(S, bool)] = 0
    return ev


def vote_f32(g):
    """float32 [H, W] -> float32 [H, W]: the 29 products and their sum in fp32, left to right as the source spells them"""
    g = np.ascontiguousarray(g, dtype=F)
    H, W = g.shape
    ev = np.zeros((H, W), F)
    acc = None
    with np.errstate(all="ignore"):
        for w, dr, dc in WEIGHTS:
            term = F(w) * g[2 + dr:H - 2 + dr, 4 + dc:W - 4 + dc]
            acc = term if acc is None else acc + term
    assert acc.dtype == F
    ev[2:H - 2, 4:W - 4] = np.where(g[2:H - 2, 4:W - 4] < 0, F(0), acc)
    return ev


def runs_of(ev, value):
    """the maximal horizontal runs of cells equal to `value` -> (row, first col, length) arrays in row-major order"""
    eq = np.asarray(ev) == value
    H, W = eq.shape
    pad = np.zeros((H, W + 2), bool)
    pad[:, 1:-1] = eq
    start = np.flatnonzero((pad[:, 1:-1] & ~pad[:, :-2]).ravel())
    end = np.flatnonzero((pad[:, 1:-1] & ~pad[:, 2:]).ravel())
    return start // W, start % W, end - start + 1


def pick_run(ev, value):
    """the first longest run of `value` in row-major order -> (row, end - len // 2, len), or None without any"""
    row, c0, ln = runs_of(ev, value)
    if ln.size == 0:
        return None
    i = int(np.flatnonzero(ln == ln.max())[0])
    return int(row[i]), int(c0[i] + ln[i] - 1 - ln[i] // 2), int(ln[i])


def record_int(ev):
    """(top, row, col) of an integer vote grid: roi_cases.mirror_record without its Python loop over the rows"""
    top = int(np.asarray(ev).max())
    row, col, _ = pick_run(ev, top)
    return top, row, col


def record_f32(evf):
    """hafo_vote_f's rule on a float32 vote grid.  topval is an int that starts at -1000; a cell replaces it where v > topval, and
    topval = (int)v truncates.  So before cell k it is the running maximum of the truncated votes of the cells before k, and the first
    loop ends on the LAST cell that exceeded it.  Then the first longest run of cells EQUAL to the final topval moves the result, if
    there is one.  -> (top, row, col, branch): branch "run", or "first" / "later" when no cell equals top -- the first cell whose
    truncation reaches top, or a later cell a fraction above it"""
    v = np.ascontiguousarray(evf, dtype=F)
    H, W = v.shape
    t = np.trunc(v.ravel().astype(np.float64)).astype(np.int64)
    before = np.maximum.accumulate(np.concatenate([[-1000], t]))[:-1]
    hits = np.flatnonzero(v.ravel().astype(np.float64) > before)
    top = int(max(-1000, t.max()))
    last = int(hits[-1])
    run = pick_run(v, F(top))
    if run is not None:
        return top, run[0], run[1], "run"
    first = int(np.flatnonzero(t == top)[0])
    return top, last // W, last % W, "first" if last == first else "later"


def z_window(h, row, col):
    """rows row-4..row+4, cols col-4..col+3 of the height grid, clipped to it, row-major"""
    H, W = h.shape
    return np.asarray(h, F)[max(0, row - 4):min(H, row + 5), max(0, col - 4):min(W, col + 4)].ravel()


def z_key(h, row, col):
    """h_locmax as the int kernels take it: the maximum above -10 under the ordered-int key (-0.0 below +0.0)"""
    w = z_window(h, row, col)
    return rc.key_max(w[w > -10.0])


def z_seq(h, row, col):
    """h_locmax as the reference and the probability kernel take it: `if (h_locmax < h) h_locmax = h` in row-major order from -10 (of
    -0.0 and +0.0 the one that comes first stays)"""
    m = F(-10.0)
    for x in z_window(h, row, col):
        if m < x:
            m = x
    return m


def stats(ev):
    """what the claims are read from: an integer vote grid -> dict"""
    top, row, col = record_int(ev)
    r, c0, ln = runs_of(ev, top)
    return dict(top=top, row=row, col=col, run=int(ln.max()), runs=int(ln.size), rows_tied=int(np.unique(r[ln == ln.max()]).size),
                runs_tied=int((ln == ln.max()).sum()), cells=int((np.asarray(ev) == top).sum()), vmin=int(np.asarray(ev).min()))


def roi_words(S):
    """bool [..., H, W] -> uint64 [..., H, (W + 63) // 64]: bit (col & 63) of word (col >> 6) of a row (the layout of haf_roi_cells)"""
    S = np.asarray(S, bool)
    W = S.shape[-1]
    nw = (W + 63) // 64
    pad = np.zeros(S.shape[:-1] + (nw * 64,), np.uint64)
    pad[..., :W] = S
    return (pad.reshape(S.shape[:-1] + (nw, 64)) << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


# ---------------------------------------------------------------- building blocks ----------------------------------------------------------------

def _bg(N, v=-1):
    return np.full((N, N), v, np.int8)


def _band(g, row, c0, L, v=1):
    """labels v on rows row-2..row+2, cols c0-4..c0+L+3: on a background of -1 exactly the cells (row, c0..c0+L-1) have all 29 taps
    inside it and vote 123 v -- one run of length L; every other cell of the band votes less"""
    N = g.shape[0]
    assert 2 <= row <= N - 3 and 4 <= c0 and c0 + L - 1 <= N - 5 and L >= 1, (N, row, c0, L)
    g[row - 2:row + 3, c0 - 4:c0 + L + 4] = v
    return g


def _centre(c0, L):
    return c0 + L - 1 - L // 2


# ---------------------------------------------------------------- the case families ----------------------------------------------------------------

def constant(N):
    mid = N - 1 - N // 2
    return [Case("all -1", _bg(N, -1), top=0, row=0, col=mid, run=N, vmin=0),
            Case("all 0", _bg(N, 0), top=0, row=0, col=mid, run=N, vmin=0),
            Case("all 1", _bg(N, 1), top=123, row=2, col=_centre(4, N - 8), run=N - 8, rows_tied=N - 4, cells=(N - 4) * (N - 8)),
            Case("all 99", _bg(N, 99), top=12177, row=2, col=_centre(4, N - 8), run=N - 8, rows_tied=N - 4),
            Case("all -9", _bg(N, -9), top=0, row=0, col=mid, run=N, vmin=0)]


def border_walk(N):
    """every cell of rows 0, 1, N-2, N-1 and of cols 0..3, N-4..N-1, corners included, each exactly once"""
    cells = [(r, c) for r in (0, 1, N - 2, N - 1) for c in range(N)]
    cells += [(r, c) for r in range(2, N - 2) for c in (0, 1, 2, 3, N - 4, N - 3, N - 2, N - 1)]
    assert len(set(cells)) == len(cells) == N * N - (N - 4) * (N - 8)
    return cells


BORDER_VALUES = (7, 0, 99, -9)


def border(N, bg):
    """one label at every position of the border walk: 1 on a background of -1 (no vote anywhere: the only label >= 0 lies on the
    border, which scores 0), and 7, 0, 99, -9 in turn on a background of +1 (the border cell still scores 0; the interior cells
    whose footprint reaches it move by weight x (value - 1))"""
    out = []
    for i, (r, c) in enumerate(border_walk(N)):
        g = _bg(N, bg)
        g[r, c] = 1 if bg < 0 else BORDER_VALUES[i % 4]
        out.append(Case("border %d,%d on %+d" % (r, c, bg), g, at=(r, c), **(dict(top=0, row=0, col=N - 1 - N // 2, cells=N * N) if bg < 0 else {})))
    return out


RUN_LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 129)


def run_lengths(N):
    """one run of 123 of every length that fits, started before and ended after a column that is a multiple of 4 only (12, 20, 68,
    132), of 8 (8, 16, 72) and of 64 (64, 128) -- a run of 1 lies on the column itself -- and in rows 2, N // 2 and N - 3"""
    out = []
    for L in RUN_LENGTHS:
        if L > N - 8:
            continue
        seen = set()
        for m in (8, 12, 16, 20, 64, 68, 72, 128, 132):
            c0 = max(4, min(m - max(1, L // 2), N - 4 - L)) if L > 1 else m
            if c0 + L - 1 > N - 5 or (L > 1 and not c0 < m <= c0 + L - 1) or c0 in seen:
                continue
            seen.add(c0)
            row = (2, N // 2, N - 3)[len(seen) % 3]
            out.append(Case("run %d over col %d" % (L, m), _band(_bg(N), row, c0, L), top=123, row=row, col=_centre(c0, L), run=L, runs=1, over=m))
    return out


def ties(N):
    """bands need 5 rows and L + 8 columns each and a free row or column between them; isolated cells are single labels 1 on a
    background of 0 (vote 55, their neighbours at most 4 + 4)"""
    out = []
    L = 3 if N >= 23 else 1
    lo, hi = 2, 8                                                     # two bands' rows: 0..4 and 6..10
    # equal runs in different rows, the upper one further right: the smaller row wins
    if N >= 2 * L + 17:
        g = _band(_band(_bg(N), hi, 4, L), lo, L + 13, L)
        out.append(Case("equal runs, rows %d and %d" % (lo, hi), g, top=123, row=lo, col=_centre(L + 13, L), run=L, runs=2, rows_tied=2))
        # equal runs in one row: the first wins
        g = _band(_band(_bg(N), hi, 4, L), hi, L + 13, L)
        out.append(Case("equal runs in row %d" % hi, g, top=123, row=hi, col=_centre(4, L), run=L, runs=2, rows_tied=1, runs_tied=2))
    # a longer run in the lower row against a shorter one above: the longer wins
    g = _band(_band(_bg(N), lo, 4, 3), hi, 4, 5)
    out.append(Case("longer run below", g, top=123, row=hi, col=_centre(4, 5), run=5, runs=2, runs_tied=1))
    g = _band(_band(_bg(N), lo, 4, 5), hi, 4, 3)
    out.append(Case("longer run above", g, top=123, row=lo, col=_centre(4, 5), run=5, runs=2, runs_tied=1))
    # isolated equal top cells: the first in row-major order wins
    g = _bg(N, 0)
    g[3, N - 5] = g[9, 4] = 1
    out.append(Case("isolated cells, rows 3 and 9", g, top=55, row=3, col=N - 5, run=1, runs=2, rows_tied=2, cells=2))
    g = _bg(N, 0)
    cols = [4, N - 5] + ([4 + (N - 9) // 2] if N >= 19 else [])      # (five columns apart at least: outside each other's footprint)
    g[N - 3, cols] = 1
    out.append(Case("isolated cells in the last interior row", g, top=55, row=N - 3, col=4, run=1, runs=len(cols), rows_tied=1, cells=len(cols)))
    # an even run against an odd one of the next length, and two adjacent rows that tie
    g = _band(_band(_bg(N), lo, 4, 2), hi, 4, 2)
    out.append(Case("runs of 2", g, top=123, row=lo, col=4, run=2, runs=2, rows_tied=2))
    g = _bg(N)
    g[2:8, 0:4 + 4 + 4] = 1                                          # 6 rows: rows 4 and 5 have all taps inside, cols 4..7
    out.append(Case("adjacent rows tie", g, top=123, row=4, col=_centre(4, 4), run=4, runs=2, rows_tied=2))
    return out


def block_seams(N):
    """N >= 129: the top run and its tie partner on either side of linear cell k x 2048, where two workgroups of the large-grid kernel
    share a grid row, and in the rows on either side of it"""
    out = []
    if N < 129:
        return out
    for k in (1, 2, 5, 7):
        r, c = divmod(k * BLOCK, N)
        if not (3 <= r <= N - 10):
            continue
        cs = min(max(c, 6), N - 7)                                    # a run of 4 over the seam column where the interior allows it
        out.append(Case("seam %d: run over it" % k, _band(_bg(N), r, cs - 2, 4), top=123, row=r, col=_centre(cs - 2, 4), run=4, seam=(r, c)))
        if 16 <= c <= N - 17:
            g = _band(_band(_bg(N), r, c - 12, 1), r, c + 8, 1)
            out.append(Case("seam %d: equal runs either side, one row" % k, g, top=123, row=r, col=c - 12, run=1, runs=2, runs_tied=2, seam=(r, c)))
            g = _band(_band(_bg(N), r, c - 12, 1), r, c + 8, 2)
            out.append(Case("seam %d: the longer run behind it" % k, g, top=123, row=r, col=c + 9 - 1, run=2, runs=2, seam=(r, c)))
            g = _band(_bg(N), r, c + 8, 3)
            out.append(Case("seam %d: top only behind it" % k, g, top=123, row=r, col=_centre(c + 8, 3), run=3, runs=1, seam=(r, c)))
            g = _band(_bg(N), r, c - 12, 3)
            out.append(Case("seam %d: top only before it" % k, g, top=123, row=r, col=_centre(c - 12, 3), run=3, runs=1, seam=(r, c)))
        # rows 2048 k // N and the next: 6 rows of labels make rows r and r + 1 tie
        g = _bg(N)
        g[r - 2:r + 4, 8:8 + 8 + 5] = 1
        out.append(Case("seam %d: rows %d and %d tie" % (k, r, r + 1), g, top=123, row=r, col=_centre(12, 5), run=5, runs=2, rows_tied=2, seam=(r, c)))
        g = _band(_band(_bg(N), r + 6, 4, 3), r - 5 if r >= 7 else r, 24, 3)
        if r >= 7:
            out.append(Case("seam %d: equal runs in the blocks before and behind" % k, g, top=123, row=r - 5, col=_centre(24, 3), run=3, runs=2, rows_tied=2, seam=(r, c)))
    assert out
    return out


def _rand(N, seed, density, values):
    rng = np.random.RandomState(seed)
    on = rng.uniform(size=(N, N)) < density
    if values == "pm1":
        g = np.where(on, 1, -1)
    elif values == "pm01":
        g = np.where(on, rng.randint(0, 2, size=(N, N)), -1)
    else:
        g = np.where(on, rng.randint(0, 100, size=(N, N)), rng.randint(-9, 0, size=(N, N)))
    return g.astype(np.int8)


def negative(N):
    g = _bg(N, -9)
    g[N // 2, N // 2] = 0
    out = [Case("a 0 among -9s", g, top=0, row=0, col=N - 1 - N // 2, run=N, vmin=-612)]
    out.append(Case("sparse +1", _rand(N, 77, 0.1, "pm1"), negative=True))
    # no vote can be positive: 0 and -9 as a checkerboard (a 0 cell sums its -9 neighbours, a -9 cell scores 0); top 0, row 0 wins
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    g = np.where((ii + jj) % 2 == 0, 0, -9).astype(np.int8)
    out.append(Case("checkerboard 0 / -9", g, top=0, row=0, col=N - 1 - N // 2, run=N, negative=True, vmin=-9 * 36))
    g = _bg(N, 0)
    g[N // 2, :] = -9                                               # a row of -9 under zeros: negative votes in the four rows around it
    out.append(Case("a row of -9 in zeros", g, top=0, row=0, col=N - 1 - N // 2, run=N, negative=True))
    return out


def random_grids(N):
    return [Case("random %s %.2f" % (values, dens), _rand(N, 1000 + 10 * i + j, dens, values), random=True)
            for i, dens in enumerate((0.05, 0.5, 0.95)) for j, values in enumerate(("pm1", "pm01", "wide"))]


def ranking(N):
    """for k_top_grasps: grids of 99s with holes (votes from 12 177 down: more than two 8-bit digits of sort key), many equal runs"""
    rng = np.random.RandomState(5)
    g = _bg(N, 99)
    g[rng.uniform(size=(N, N)) < 0.03] = -9
    out = [Case("99 with -9 holes", g, wide=True)]
    g = _bg(N, 99)
    g[rng.uniform(size=(N, N)) < 0.2] = 0
    out.append(Case("99 with 0 holes", g, wide=True))
    out.append(Case("all 99", _bg(N, 99), top=12177, wide=True))
    g = _bg(N)
    for r in range(2, N - 2, 6):                                      # a band per 6 rows, lengths falling: every run a candidate of its own length
        _band(g, r, 4, max(1, N - 8 - r))
    out.append(Case("bands of falling length", g, top=123, row=2, run=N - 10))
    return out


# ---- float grids (the probability form) ----

def float_cases(N):
    out = []
    for c in (constant(N)[2], ties(N)[0], negative(N)[0], _rand_case(N, 31, 0.5, "pm01"), _rand_case(N, 32, 0.9, "wide")):
        out.append(Case("integer-valued: " + c.name, c.grid.astype(F), integer=True))
    # +-p with p in [0.5, 1): what res * prob gives for labels +-1; -1 where unmasked
    for seed in (1, 2):
        rng = np.random.RandomState(seed)
        p = rng.uniform(0.5, 1.0, size=(N, N)).astype(F)
        p = np.minimum(p, np.nextafter(F(1), F(0)))
        g = np.where(rng.uniform(size=(N, N)) < 0.5, p, -p)
        g[rng.uniform(size=(N, N)) < 0.3] = -1.0
        out.append(Case("+-p seed %d" % seed, g.astype(F), branch=("first", "later")))
    # quarters: sums are exact multiples of 0.25, so cells EQUAL to the truncated top occur (run) or do not (later)
    for seed, dens, branch in QUARTER_SEEDS[N]:
        rng = np.random.RandomState(seed)
        g = (rng.randint(0, 5, size=(N, N)) * 0.25).astype(F)
        g[rng.uniform(size=(N, N)) < dens] = -1.0
        out.append(Case("quarters seed %d" % seed, g, branch=(branch,)))
    # the first cell reaching the top's truncation, then later cells a fraction above it; the last of those wins
    g = np.zeros((N, N), F)
    g[5, N - 6], g[9, 6], g[9, N - 7], g[N - 4, 5] = 1.01, 1.015, 1.005, 0.99
    out.append(Case("a later cell a fraction above", g, top=55, row=9, col=N - 7, branch=("later",)))
    g = g.copy()
    g[N - 3, N // 2] = 1.0                                            # ... and a cell that IS 55: the run rule takes over
    out.append(Case("... and an exact cell behind them", g, top=55, row=N - 3, col=N // 2, branch=("run",)))
    g = np.zeros((N, N), F)
    g[7, 7] = 1.01
    g[4, 9] = 0.999
    out.append(Case("the first cell alone", g, top=55, row=7, col=7, branch=("first",)))
    g = np.full((N, N), -0.5, F)
    g[N // 2, N // 2] = 0.0                                           # -34: truncates to -34, below the border's 0
    out.append(Case("negative float votes", g, top=0, row=0, col=N - 1 - N // 2, branch=("run",)))
    return out


def _rand_case(N, seed, density, values):
    return Case("random %s %.2f seed %d" % (values, density, seed), _rand(N, seed, density, values))


# (seed, share of -1 cells, branch the mirror takes): found by running the mirror, pinned by test_vote_cpu.py
QUARTER_SEEDS = {56: ((1, 0.3, "run"), (2, 0.3, "later"), (3, 0.3, "first")), 136: ((3, 0.3, "run"), (13, 0.3, "later"), (1, 0.3, "first"))}


# ---- height grids for the z window ----

def height_cases(N):
    """label grids whose winner lies in each corner of the interior (the window is clipped above or below; left and right it reaches
    cols 0 and N-1 but never leaves the grid, as col >= 4 and col + 3 <= N - 2 for every winner of a positive vote), on the top row (a
    vote of 0), with heights that put larger values just outside the window"""
    rng = np.random.RandomState(9)
    out = []
    for row, c0 in ((2, 4), (2, N - 5), (N - 3, 4), (N - 3, N - 5)):
        h = rng.uniform(-12.0, 1.0, size=(N, N)).astype(F)
        r0, r1, q0, q1 = max(0, row - 4), min(N, row + 5), max(0, c0 - 4), min(N, c0 + 4)
        h[r0:r1, q0:q1] = np.minimum(h[r0:r1, q0:q1], F(0.5))
        h[r0, q0], h[r1 - 1, q1 - 1] = 0.25, 0.75                     # the window's own corners hold its maximum
        for rr, cc in ((r0 - 1, q0), (r1, q0), (r0, q0 - 1), (r0, q1), (r1 - 1, q1)):
            if 0 <= rr < N and 0 <= cc < N:
                h[rr, cc] = 5.0                                       # just outside
        out.append(Case("window at %d,%d" % (row, c0), _band(_bg(N), row, c0, 1), heights=h, top=123, row=row, col=c0, z=F(0.75)))
    h = rng.uniform(-12.0, 1.0, size=(N, N)).astype(F)
    out.append(Case("window on row 0", _bg(N), heights=h, top=0, row=0, col=N - 1 - N // 2))
    h = np.full((N, N), 3.0, F)
    h[0:N // 2 + 5, :] = -11.0
    out.append(Case("nothing above -10", _band(_bg(N), N // 2 - 4, 4, 1), heights=h, top=123, row=N // 2 - 4, col=4, z=F(-10.0)))
    h = np.full((N, N), -10.0, F)                                     # -10 itself is not above -10
    out.append(Case("all at -10", _band(_bg(N), 6, 6, 1), heights=h, top=123, row=6, col=6, z=F(-10.0)))
    for name, a, b in (("-0.0 then +0.0", -0.0, 0.0), ("+0.0 then -0.0", 0.0, -0.0)):
        h = np.full((N, N), -5.0, F)
        h[6, 5], h[6, 6] = a, b
        out.append(Case(name, _band(_bg(N), 6, 6, 1), heights=h, top=123, row=6, col=6, z=F(0.0), zero_signs=True))
    return out


FAMILIES = dict(constant=constant, run_lengths=run_lengths, ties=ties, block_seams=block_seams, negative=negative, random=random_grids,
                ranking=ranking, heights=height_cases)


def int_cases(N):
    """every int8 family but the border walks (they are two families of their own: border(N, -1), border(N, +1))"""
    return [(fam, c) for fam, build in FAMILIES.items() for c in build(N)]


def roi_sets(N):
    """the cell sets of the ROI form: empty, full, a checkerboard, single cells at columns 63, 64 and N-5, one whole row"""
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    out = [("empty", np.zeros((N, N), bool)), ("full", np.ones((N, N), bool)), ("checkerboard", (ii + jj) % 2 == 0)]
    for c in (63, 64, N - 5):
        if 4 <= c <= N - 5:
            S = np.zeros((N, N), bool)
            S[N // 2, c] = True
            out.append(("cell at col %d" % c, S))
    S = np.zeros((N, N), bool)
    S[N // 2, :] = True
    out.append(("row %d" % (N // 2), S))
    return out


# ---- the oracle's vote on one grid ----

def oracle_vote(grid):
    """hafo_vote (int8 grid) / hafo_vote_f (float32 grid) -> (float32 [H, W] votes, (top, row, col))"""
    import ctypes as C
    from oracle import oracle as O
    g = np.ascontiguousarray(grid)
    assert g.dtype in (np.int8, F) and g.ndim == 2
    H, W = g.shape
    cfg = O.make_cfg(H=H, W=W)
    ev, best = np.zeros((H, W), F), np.zeros(3, np.int32)
    (O.lib().hafo_vote if g.dtype == np.int8 else O.lib().hafo_vote_f)(C.byref(cfg), g.ctypes.data, ev.ctypes.data, best.ctypes.data)
    return ev, (int(best[2]), int(best[0]), int(best[1]))


# ---- models whose labels are not +-1 ----
# (label a, label b) -> the grid values of the two classes: atoi of the first two characters of the "%g" text (server.cpp:843), so
# -10 reads as -1, the value of an unlabelled cell
LABEL_PAIRS = {(1, 0): (1, 0), (0, 1): (0, 1), (2, 1): (2, 1), (7, -7): (7, -7), (99, -9): (99, -9), (10, -10): (10, -1), (-1, 1): (-1, 1)}
LABEL_NSV = 200
# seed of models.write_random_model(balanced=True) per request: the oracle's label grids hold more than 50 cells of each class
LABEL_REQUESTS = {
    56: dict(seed=4, cfg=dict(n_rolls=4), inp=dict(grasp_area_length_x=32, grasp_area_length_y=44)),
    136: dict(seed=9, cfg=dict(n_rolls=1, grid_h=136, grid_w=136), inp=dict(grasp_area_length_x=120, grasp_area_length_y=50)),
}
