"""Clouds whose HEIGHTS are hostile to the code between the integral image and the label (device-free; data and oracle calls only).

Every other scene of the suite keeps its heights between 0 and about 0.4 m: every Haar feature stays below about 26, nearly every
attribute inside the range file, every scaled attribute within a few units.  The cases here take the same base cloud
(models.synthetic_cloud(grid, k=2, seed=21), approach vector (0, 0, 1), centre 0) and rewrite the points' z so that the GRID's height
h follows a rule (z' = h - 0.15, chosen so that the reference's fp32 z' + 0.15f gives h back exactly where h is a short binary
fraction; cx, cy: the point's cell row / column, z: the base cloud's z, 0.05 .. 0.26):

  natural   h = z + 0.15                           the control: what the rest of the suite looks like
  scale8    h = 8 z                                attributes leave the range file, nothing leaves any tier's number format
  half64    h = 64 z where y < 0, else z           scaled attributes beyond the exact-integer tier's fixed point (|x| > 15.874) and
                                                   kernel exponents beyond the screening band's a_x < 30, beside natural cells
  block1e6  h = 1e6 z where cy >= grid - 20, else z  features beyond decq4_float_scr's 1e4, scaled attributes beyond fp16's 65504
  ramp6     h = (z + 0.15) 2^(cy / 6)              every threshold above is crossed inside each row of the search area
  spikes    h = 3e4 at every 211th cell            features beyond 1e4 next to untouched cells
  pits      h = -0.9 at every 53rd cell            negative heights: the integral image is not monotone
  dyadic    h = round(64 (z + 0.15)) / 64          exact "%.4g" ties everywhere
  flat      h = 0.25                               features that are exactly 0; fv.cpp:187-191's `else returnval = -1` dominates

  leftblock h = 1e6 z where cy < 20, else z         the mask rule itself: behind the block every corner of the integral image carries
                                                   sums of 1e8 and more, the fp32 box sums of the rule (box > 0.03) drown in their
                                                   rounding, and the mask of roll 0 loses 371 of its cells (rows down to 58 cells)

block1e6 has its block at the grid's LAST 20 columns so that every masked row keeps its 82 cells (one whole 64-chunk of the feature
kernels and a left-over), as every case but leftblock does; leftblock is the same block at the first 20 columns, where the reference's
mask breaks down, and is there for that: its mask, like everything behind it, must still be the oracle's.

The request: 96 x 96 grid, search area 46 x 96, 2 rolls of 25 degrees: 5305 evaluations (leftblock: 4934).  Two models: the committed surrogate (rho = -1.75: an evaluation
whose kernel values all underflow has dec = +1.75) and write_random_model(300, seed=3, balanced=True) (gamma = 0.0031, rho = +0.01:
dec = -0.01, the other side of zero).

What regimes() measures from the ORACLE ALONE on 200 seeded masked cells of roll 0 (`outside`, `big`, `zero`: shares of the attribute
values svm-scale keeps -- outside the range file, |feature| >= 1e4 or 0 < |feature| < 1e-9, feature == 0; `f16`, `i8`, `ax30`: shares of
the cells with a scaled attribute beyond 65504, one beyond the exact-integer tier's 15.874, gamma |x|^2 / (2 ln 2) >= 30; `ties`: exact "%.4g" ties among the
200 x 324 feature values; `neg`: negative heights in the two grids; S = sum |coef| K over all evaluations; sur / rnd: the two models):

  case      outside  big     zero     f16    i8     ax30 (sur/rnd)  ties   neg  S == 0 (sur/rnd)  labels +/- (sur)  labels +/- (rnd)
  natural   0.081    0.000   0.0000   0.000  0.000  0.000 / 0.000      13     0     0 /    0          0 / 5305       5225 /   80
  scale8    0.343    0.000   0.0000   0.000  0.000  0.000 / 0.000      26     0     0 /    0          0 / 5305       4214 / 1091
  half64    0.572    0.000   0.0001   0.000  0.615  0.615 / 0.615     294     0   209 /  242          0 / 5305       2166 / 3139
  block1e6  0.229    0.170   0.0000   0.195  0.195  0.195 / 0.195     136     0  1306 / 1306         11 / 5294       3914 / 1391
  ramp6     0.937    0.130   0.0000   0.010  0.885  0.845 / 0.845     216     0  3641 / 3647          0 / 5305        313 / 4992
  spikes    0.430    0.363   0.0031   0.075  0.725  0.725 / 0.725    3031     0  4032 / 4032          0 / 5305       1248 / 4057
  pits      0.090    0.000   0.0000   0.000  0.000  0.000 / 0.000      12   241     0 /    0          3 / 5302       5061 /  244
  dyadic    0.083    0.000   0.0034   0.000  0.000  0.000 / 0.000    4278     0     0 /    0          0 / 5305       5209 /   96
  flat      0.084    0.000   0.4241   0.000  0.000  0.000 / 0.000       0     0     0 /    0          0 / 5305       5292 /   13
  leftblock 0.840    0.204   0.0816   0.235  0.970  0.520 / 0.515      93     0  1331 / 1331         44 / 4890        931 / 4003

No feature value is non-finite in any case (a non-finite float prints as text the reference parses differently: out of scope)."""
import atexit
import os
import re
import shutil
import tempfile
from fractions import Fraction

import numpy as np

import models
from oracle import oracle as O
from oracle_inputs import oracle_input

GRID = 96
CASES = ("natural", "scale8", "half64", "block1e6", "ramp6", "spikes", "pits", "dyadic", "flat", "leftblock")
MODELS = ("surrogate", "random")
Z_SHIFT = np.float32(0.15)
F16_MAX, DECQ_MAX, DECQ_MIN = 65504.0, 1e4, 1e-9
I8_Q, I8_MAX_INT = 23, 63 * (2 ** 21 + 2 ** 14 + 2 ** 7 + 1)      # csrc/kernels.h, kI8Q / kI8Max: four balanced base-128 digits, |x| <= 15.874


def beyond_fixed_point(scaled):
    """bool [...]: the scaled attribute does not fit the exact-integer tier's fixed point (i8_digits: rint(x 2^23) beyond kI8Max)."""
    return np.abs(np.rint(np.asarray(scaled, np.float64) * 2.0 ** I8_Q)) > I8_MAX_INT


def _z_for_height(h):
    """fp32 z' with fp32(z' + 0.15f) == fp32(h) wherever one exists among fp32(h - 0.15f) and its neighbours (the reference's
    pz = ... + M[10] * z + M[11] with M[10] = 1, M[11] = 0.15f)."""
    h = np.asarray(h, np.float32)
    z = (h - Z_SHIFT).astype(np.float32)
    for cand in (np.nextafter(z, np.float32(np.inf)), np.nextafter(z, np.float32(-np.inf))):
        bad = (z + Z_SHIFT).astype(np.float32) != h
        z = np.where(bad & ((cand + Z_SHIFT).astype(np.float32) == h), cand, z)
    return z


def base_cloud(grid=GRID):
    return models.synthetic_cloud(grid=grid, k=2, seed=21)


def hostile_cloud(name, grid=GRID):
    """The base cloud with its z rewritten by rule `name` (see the module's docstring)."""
    xyz = base_cloud(grid)
    z = xyz[:, 2].astype(np.float64)
    cell = np.arange(len(xyz)) // 2                           # (the cloud holds the cells' points pairwise, row-major)
    cy = cell % grid
    if name == "natural":
        return xyz
    if name == "scale8":
        h = 8.0 * z
    elif name == "half64":
        h = np.where(xyz[:, 1] < 0, 64.0 * z, z)
    elif name == "block1e6":
        h = np.where(cy >= grid - 20, 1.0e6 * z, z)
    elif name == "leftblock":
        h = np.where(cy < 20, 1.0e6 * z, z)
    elif name == "ramp6":
        h = (z + 0.15) * 2.0 ** (cy / 6.0)
    elif name == "spikes":
        h = np.where(cell % 211 == 0, 3.0e4, z + 0.15)
    elif name == "pits":
        h = np.where(cell % 53 == 0, -0.9, z + 0.15)
    elif name == "dyadic":
        h = np.round((z + 0.15) * 64.0) / 64.0
    elif name == "flat":
        h = np.full_like(z, 0.25)
    else:
        raise KeyError(name)
    out = xyz.copy()
    out[:, 2] = _z_for_height(h)
    return out


def request(grid=GRID, length_x=46):
    """(cfg_kw, in_kw): 2 rolls of 25 degrees on a grid x grid grid, a strip of length_x rows over the whole width."""
    return (dict(n_rolls=2, roll_step_deg=25, grid_h=grid, grid_w=grid, max_points=2 * grid * grid),
            dict(grasp_area_length_x=length_x, grasp_area_length_y=grid))


def cases(grid=GRID, length_x=46, names=CASES):
    """-> [(name, cloud, cfg_kw, in_kw)]"""
    cfg_kw, in_kw = request(grid, length_x)
    return [(n, hostile_cloud(n, grid), dict(cfg_kw), dict(in_kw)) for n in names]


# ---- models and the oracle, once per process -----------------------------------------------------------------------------------------

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DATA = os.path.join(_GOLDEN, "data")
_TMP = None
_MODEL_PATHS, _ORACLES, _RUNS, _CLOUDS, _REGIMES = {}, {}, {}, {}, {}


def _tmp():
    global _TMP
    if _TMP is None:
        _TMP = tempfile.mkdtemp(prefix="haf_hostile_")
        atexit.register(shutil.rmtree, _TMP, ignore_errors=True)
    return _TMP


def model_path(model):
    """"surrogate": the committed model; "random": write_random_model(300, seed=3, balanced=True); "clustered":
    write_clustered_model(260, seed=5); "surrogate_prob": the surrogate with the committed probA / probB."""
    if model not in _MODEL_PATHS:
        if model == "surrogate":
            p = os.path.join(_GOLDEN, "surrogate.model")
        elif model == "random":
            p = models.write_random_model(os.path.join(_tmp(), "rand300.model"), 300, seed=3, balanced=True)
        elif model == "clustered":
            p = models.write_clustered_model(os.path.join(_tmp(), "clustered260.model"), 260, seed=5)
        elif model == "surrogate_prob":
            import json
            with open(os.path.join(_GOLDEN, "surrogate_prob.json")) as f:
                pj = json.load(f)
            p = models.write_probability_model(os.path.join(_tmp(), "surrogate_prob.model"), model_path("surrogate"), pj["probA"], pj["probB"])
        else:
            raise KeyError(model)
        _MODEL_PATHS[model] = p
    return _MODEL_PATHS[model]


def oracle(model):
    if model not in _ORACLES:
        _ORACLES[model] = O.Oracle(os.path.join(_DATA, "Features.txt"), os.path.join(_DATA, "range21062012_allfeatures"), model_path(model))
    return _ORACLES[model]


def cloud(name, grid=GRID):
    if (name, grid) not in _CLOUDS:
        _CLOUDS[(name, grid)] = hostile_cloud(name, grid)
    return _CLOUDS[(name, grid)]


def oracle_run(name, model, grid=GRID, length_x=46, probability=0):
    """orc.run of (case, model), computed once per process.  The arrays are shared: nobody writes to them."""
    key = (name, model, grid, length_x, probability)
    if key not in _RUNS:
        cfg_kw, in_kw = request(grid, length_x)
        ocfg = O.make_cfg(n_rolls=cfg_kw["n_rolls"], roll_step_deg=cfg_kw["roll_step_deg"], H=grid, W=grid, probability=probability)
        want = oracle(model).run(cloud(name, grid), ocfg, oracle_input(in_kw))
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[key] = want
    return _RUNS[key]


# ---- the regimes of a case, from the oracle alone -------------------------------------------------------------------------------------

_VALUE = re.compile(r":(\S+)")


def q4_row(orc, f):
    """hafo_q4 of every value of one feature row: the doubles strtod reads from the row's "%.4g" text (the oracle prints the line, as
    the reference's feature file holds it; float() is strtod)."""
    tok = _VALUE.findall(orc.feature_line(f))
    assert len(tok) == len(f)
    return np.array([float(t) for t in tok])


def oracle_attr_rows(orc, ii, cells):
    """(features fp32 [n, 324], q4 [n, 324], scaled [n, 323]) of the oracle for the given cells of one integral image."""
    skip = np.zeros(325, np.uint8)
    skip[324] = 1               # phantom attribute: constant -1 in every row -> dropped by svm-scale.c:336-337
    F, Q, S = [], [], []
    for i, j in cells:
        f = orc.feature_values(ii[i - 7:i + 8, j - 7:j + 8])
        q = q4_row(orc, f)
        F.append(f)
        Q.append(q)
        S.append(orc.scale_row(q, 323, skip))
    return np.array(F), np.array(Q), np.array(S)


def beyond_fixed_point_cells(name, grid=GRID, length_x=46):
    """Linear indices (roll * H * W + row * W + col, sorted) of EVERY evaluation of the case with a scaled attribute beyond the
    exact-integer tier's fixed point, from the oracle's own attribute rows (the attributes do not depend on the model).  Once per
    process."""
    key = ("ovf", name, grid, length_x)
    if key not in _REGIMES:
        orc, want = oracle("surrogate"), oracle_run(name, "surrogate", grid, length_x)
        out = []
        for roll in range(want["rolls_done"]):
            cells = np.stack(np.nonzero(want["mask"][roll]), 1)
            S = oracle_attr_rows(orc, want["integral"][roll], cells)[2]
            hit = cells[beyond_fixed_point(S).any(axis=1)]
            out.append(roll * grid * grid + hit[:, 0] * grid + hit[:, 1])
        _REGIMES[key] = np.sort(np.concatenate(out))
    return _REGIMES[key]


def is_tie(v):
    """The fp32 value v lies exactly half way between two "%.4g" neighbours: |v| 10^k, 1000 <= |v| 10^k < 10000, has the
    fractional part 1/2 (exact rational arithmetic)."""
    v = float(v)
    if v == 0.0 or not np.isfinite(v):
        return False
    x = abs(Fraction(v))
    while x >= 10000:
        x /= 10
    while x < 1000:
        x *= 10
    return x - (x.numerator // x.denominator) == Fraction(1, 2)


def count_ties(F):
    """Number of exact "%.4g" ties among the fp32 values F: a float64 estimate of the fractional part picks the candidates, is_tie()
    decides them exactly."""
    v = np.abs(np.asarray(F, np.float32).reshape(-1).astype(np.float64))
    v = v[(v > 0) & np.isfinite(v)]
    y = v * 10.0 ** (3 - np.floor(np.log10(v)))
    cand = v[np.abs(y - np.floor(y) - 0.5) < 1e-6]
    return int(sum(is_tie(x) for x in cand))


def sample_cells(mask, n_sample, seed=5):
    """n_sample seeded masked cells of one roll's mask, row-major."""
    cells = np.stack(np.nonzero(mask), 1)
    if len(cells) > n_sample:
        cells = cells[np.sort(np.random.RandomState(seed).choice(len(cells), n_sample, replace=False))]
    return cells


def kept_attributes(orc):
    """bool [324]: the attributes svm-scale writes (not the phantom 324th, not one whose range is a single value)."""
    _, _, fmin, fmax, present = orc.range_table()
    kept = np.zeros(324, bool)
    kept[:323] = (present[1:324] != 0) & (fmin[1:324] != fmax[1:324])
    return kept


def regimes(orc, want, model=None, n_sample=200, roll=0):
    """What the oracle alone says about the regimes a case reaches, over n_sample seeded masked cells of `roll`:
    cells [n, 2], F / Q / S (oracle_attr_rows), per-cell predicates big / f16 / i8 / ax30 (bool [n]; ax30 needs `model`, the dict of
    Oracle.model_arrays()), and the shares and counts of the docstring's table."""
    key = (id(want), n_sample, roll)
    if key in _REGIMES:
        return _REGIMES[key]
    _, _, fmin, fmax, _ = orc.range_table()
    kept = kept_attributes(orc)
    cells = sample_cells(want["mask"][roll], n_sample)
    F, Q, S = oracle_attr_rows(orc, want["integral"][roll], cells)
    Fk, Qk = F[:, kept].astype(np.float64), Q[:, kept]
    lo, hi = fmin[1:324][kept[:323]], fmax[1:324][kept[:323]]
    big_v = (np.abs(Fk) >= DECQ_MAX) | ((Fk != 0) & (np.abs(Fk) < DECQ_MIN))
    out = dict(cells=cells, F=F, Q=Q, S=S,
               big=big_v.any(axis=1), f16=(np.abs(S) > F16_MAX).any(axis=1), i8=beyond_fixed_point(S).any(axis=1),
               share_outside=float(((Qk < lo) | (Qk > hi)).mean()), share_big=float(big_v.mean()), share_zero=float((Fk == 0).mean()),
               n_ties=count_ties(F), finite=bool(np.isfinite(F).all()),
               n_negative_heights=int((want["heights"] < 0).sum()), n_masked=int((want["mask"] == 1).sum()),
               min_row=int(min(c for c in (want["mask"][0] == 1).sum(axis=1) if c)) if (want["mask"][0] == 1).any() else 0)
    m = want["mask"] == 1
    out["n_s_zero"] = int((want["sabs"][m] == 0).sum())
    out["n_pos"], out["n_neg"] = int((want["labels"][m] > 0).sum()), int((want["labels"][m] < 0).sum())
    if model is not None:
        out["ax30"] = model["gamma"] * (S * S).sum(axis=1) / (2.0 * np.log(2.0)) >= 30.0
        out["share_ax30"] = float(out["ax30"].mean())
    for k in ("big", "f16", "i8"):
        out["share_" + k + "_cells"] = float(out[k].mean())
    _REGIMES[key] = out
    _REGIMES[("keep", key)] = want                 # (the key holds id(want): keep the object alive)
    return out
