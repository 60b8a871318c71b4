"""What the screening feature kernels must write, from a definition (no csrc/ arithmetic; data, the oracle and numpy only).

The kernels of the screening feature pass (csrc/features.hip: k_features_small<2>, k_features<2, 16 | 8>, k_features_serial<2, false | true>)
write per evaluation 320 fp16 operands, the fp32 sums the guard band is made of, and a_x.  This module restates all of it:

  v      the fp32 feature value of the slot's representative attribute, in the reference's order: Oracle.feature_values (hafo_feature_values)
  q4f    fl32 of the "%.4g" round trip of v as the screening pass takes it (haf_test_decq4_scr_n; NaN outside [1e-9, 1e4) and 0)
  u'     fmaf(q4f, scr_mul, scr_add) in fp32, formed EXACTLY: fl32(fl64(q4f mul) + add) is right unless the fp64 sum rounded AND landed on
         an fp32 tie; those cases are settled with fractions.Fraction (exact_fma32)
  u^     RN_fp16(u'), subnormals kept (numpy's float16)
  su2 = sum u'^2, sd2 = sum (u^ - u')^2, cr = sum (u^ - u') g + u' hd, ub = sum u' ubar, sx2 = su2 + sum extra u'^2: fp64, with the
         sum of the terms' magnitudes beside each (the band allows an fp32 accumulation kF32Acc of that)
  v_exact  the weighted sum of the window's region sums without any rounding, from the fp32 corners' exact binary values (Python
         integers in units of 2^-298), for the HAF slots; u_lin = scr_mul v_exact + scr_add; nu2 >= sum (u' - u_lin)^2
  the operand image's byte layout (20 480 bytes per 32 evaluations), the evaluation order of a masked grid (whole chunks
  of 64 of all rows, then the rows' remainders, which are taken from the rows' STARTS), the wave kind of every 64 evaluations, and for
  a low-rank request the path (A, B, C) of every wave from the three conditions above k_features_serial.

The slot table (which attribute a slot stands for, its two scaling floats, extra, pad, the correction constants) comes from the
device-free table build behind haf_test_host_slot_table; derive_scaling() forms scr_mul and scr_add again from the range file and
c = sqrt(2 gamma log2 e), and check_table() holds the hook's floats to them, so that a wrong table cannot be its own reference.  The
centred forms fold a centre mu into scr_add; the build is free in its choice (any centre gives the same decision function, which the
label comparison behind every GPU case checks), so the hook hands mu out, scr_add is held to the derived add - mu, |mu| to the norms the
band counts, and tests/test_screen_operands_cpu.py holds u' + mu of the centred table to the oracle's c x as it does u' of the plain one."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

import hostile_cases as hc
import models
from haf_grasping_amd import capi

K = 320                                    # slots
TILE_EVALS, TILE_BYTES, BAND_FLOATS = 32, 20480, 8
BLOCK_EVALS = 256                          # the screening sweep's workgroup: the evaluation list is padded to whole blocks
KF32ACC = 326.0 * 2.0 ** -24 * 1.01        # the band's fp32-accumulation constant (csrc/screen_band.h, features.hip: kF32Acc)
ETA_REL = 5.0e-6 * (1.0 + 1e-6) + 1.8e-7   # |u' - u| <= ETA_REL |u'| + eta_abs (csrc/feature_device.h: kScreenEtaRel)
FORMS = ("screen", "screen_cr", "screen_lrp")
KAPPA = 12.0                               # the matrix-core rounding constant handed to the table build (not read by anything compared here)
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
FEATURES, RANGE = os.path.join(_DATA, "Features.txt"), os.path.join(_DATA, "range21062012_allfeatures")


# ---- the operand image ------------------------------------------------------------------------------------------------

def image_offset(r, k):
    """Byte offset of (row r of 32, slot k of 320) in one 20 KiB operand image: per k-step of 32 slots and row block of 16 rows the 64
    lanes of a wave hold 8 consecutive slots each, lane = ((k % 32) / 8) 16 + r % 16."""
    return ((((k >> 5) * 2 + (r >> 4)) * 64 + ((k >> 3) & 3) * 16 + (r & 15)) * 16) + (k & 7) * 2


_HALF_INDEX = np.array([[image_offset(r, k) // 2 for k in range(K)] for r in range(TILE_EVALS)])


def image_rows(X, evals):
    """uint16 [len(evals), 320]: the fp16 bit patterns of the given evaluations out of the operand images X (uint8, whole tiles)."""
    tiles = np.ascontiguousarray(X[:len(X) // TILE_BYTES * TILE_BYTES]).view(np.uint16).reshape(-1, TILE_BYTES // 2)
    evals = np.asarray(evals)
    return tiles[(evals // TILE_EVALS)[:, None], _HALF_INDEX[evals % TILE_EVALS]]


# ---- the slot table ----------------------------------------------------------------------------------------------------------------

def slot_table(model_file, grid, form, feature_file=None, nshaf=302):
    """haf_test_host_slot_table for the given model on a grid x grid engine, under the current environment (HAF_NO_FAST_GROUPS, ...):
    dict(attr, skip, shaf [320] int; mul, add, extra, pad [320] f32; g, hd, ub [320] f32; mu [320] f64: the centre of the centred forms;
    c, lr_rho, ubar2, eta_abs, cr, mu_norm, mu_norm_t, fast_groups, extra_groups) or None when the model did not get that form's tables."""
    cfg = capi.default_config(feature_file=feature_file or FEATURES, range_file=RANGE, model_file=model_file, grid_h=grid, grid_w=grid,
                              nr_features_without_shaf=nshaf)
    attr, skip, shaf = (np.zeros(K, np.int32) for _ in range(3))
    desc, corr = np.zeros((K, 4), np.float32), np.zeros((K, 3), np.float32)
    mu, scal, groups, avail, msg = np.zeros(K), np.zeros(7), np.zeros(2, np.uint64), C.c_int(), C.create_string_buffer(512)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.testlib().haf_test_host_slot_table(C.byref(cfg), KAPPA, KAPPA, FORMS.index(form), p(attr), p(skip), p(shaf), p(desc), p(corr),
                                                 p(mu), p(scal), p(groups), C.byref(avail), msg, len(msg))
    assert rc == 0, (rc, msg.value.decode())
    if not avail.value:
        return None
    return dict(attr=attr, skip=skip, shaf=shaf, mul=desc[:, 0].copy(), add=desc[:, 1].copy(), extra=desc[:, 2].copy(), pad=desc[:, 3].copy(),
                g=corr[:, 0].copy(), hd=corr[:, 1].copy(), ub=corr[:, 2].copy(), c=scal[0], lr_rho=scal[1], ubar2=scal[2], eta_abs=scal[3],
                cr=int(scal[4]), mu=mu, mu_norm=scal[5], mu_norm_t=scal[6], nshaf=nshaf, fast_groups=int(groups[0]), extra_groups=int(groups[1]), form=form)


def derive_scaling(orc, gamma, attr):
    """(c, mul, add) in fp64 for the plain form: c = sqrt(2 gamma log2 e); for the slot of attribute a (row a of Features.txt, index a + 1
    of the range file) mul = c (upper - lower) / (fmax - fmin), add = c lower - fmin mul.  Unused slots: 0."""
    lower, upper, fmin, fmax, present = orc.range_table()
    c = math.sqrt(2.0 * gamma * math.log2(math.e))
    mul, add = np.zeros(K), np.zeros(K)
    for s, a in enumerate(attr):
        if a < 0:
            continue
        lo, hi = float(fmin[a + 1]), float(fmax[a + 1])
        assert present[a + 1] and hi != lo, ("a slot for an attribute svm-scale drops", s, a)
        mul[s] = float(Fraction(c) * Fraction(upper - lower) / (Fraction(hi) - Fraction(lo)))
        add[s] = float(Fraction(c) * Fraction(lower) - Fraction(lo) * Fraction(mul[s]))
    return c, mul, add, lower


def check_table(orc, gamma, tab):
    """The hook's table against the range file: c, every slot's scr_mul (and scr_add in the plain form) to fp32 rounding -- relative
    2^-23 plus, for scr_add, absolute 2^-23 |c lower| --, pad = |scr_mul| rounded up (0 for SHAF and unused slots), every attribute
    svm-scale keeps in exactly one slot, extra = the attributes that share the slot beyond the first, the group masks."""
    lower, upper, fmin, fmax, present = orc.range_table()
    reg, w = orc.feature_table()
    c, mul, add, lower = derive_scaling(orc, gamma, tab["attr"])
    assert abs(tab["c"] - c) <= 4e-16 * c
    used = tab["attr"] >= 0
    assert (tab["skip"][used] == 0).all() and (tab["skip"][~used] == 1).all()
    assert used[:used.sum()].all(), "used slots are the first ones"
    u23 = 2.0 ** -23
    assert (np.abs(tab["mul"].astype(np.float64) - mul) <= u23 * np.abs(mul)).all(), "scr_mul"
    assert (tab["mul"][~used] == 0).all() and (tab["add"][~used] == 0).all() and (tab["extra"][~used] == 0).all() and (tab["pad"][~used] == 0).all()
    # scr_add: the plain form's, and in the centred forms with the centre folded in -- add - mu, mu as the build chose it (any centre
    # gives the same decision function; the label comparison behind every GPU case holds the choice) and as the band counts it
    mu = tab["mu"]
    if not tab["cr"]:
        assert (mu == 0).all()
    assert (mu[~used] == 0).all() and (mu[tab["mul"] == 0] == 0).all()
    assert (np.abs(tab["add"].astype(np.float64) - (add - mu)) <= u23 * np.abs(add - mu) + u23 * abs(c * lower)).all(), "scr_add"
    if tab["cr"]:
        n_s, n_t = math.sqrt((mu * mu).sum()), math.sqrt(((1.0 + tab["extra"]) * mu * mu).sum())
        assert n_s > 0 and abs(tab["mu_norm"] - n_s) <= 1e-9 * n_s and abs(tab["mu_norm_t"] - n_t) <= 1e-9 * n_t, "|mu| as the band counts it"
    # every kept attribute (present in the range file with fmax != fmin, a row of the feature file) sits in exactly one slot
    nf = len(w)
    kept = [a for a in range(min(nf, 323)) if present[a + 1] and fmin[a + 1] != fmax[a + 1]]
    def key(a):                 # the same function of the window (active regions, their weights, the rule) with the same range
        act = region_active(reg[a], w[a])
        return (tuple((k, region_corners(reg[a], k), float(w[a, k])) for k in range(3) if act[k]), float(fmin[a + 1]), float(fmax[a + 1]), a >= tab["nshaf"])
    rep_of = {}
    for a in kept:
        rep_of.setdefault(key(a), a)
    reps = sorted(set(rep_of.values()))
    assert list(tab["attr"][used]) == reps, "one slot per distinct kept attribute, in the feature file's order"
    sharers = {r: 0 for r in reps}
    for a in kept:
        sharers[rep_of[key(a)]] += 1
    assert [int(x) for x in tab["extra"][used]] == [sharers[r] - 1 for r in reps], "extra counts the sharers"
    assert sum(sharers.values()) == len(kept)
    shaf = tab["attr"] >= tab["nshaf"]
    assert (tab["shaf"][used] == shaf[used]).all()
    want_pad = np.where(used & ~shaf, np.nextafter(np.abs(tab["mul"]), np.float32(np.inf)), np.float32(0))
    assert (tab["pad"] == want_pad).all(), "pad = |scr_mul| rounded up for HAF slots"
    eg = sum(1 << g for g in range(K // 8) if (tab["extra"][8 * g:8 * g + 8] != 0).any())
    assert tab["extra_groups"] == eg
    if "HAF_NO_FAST_GROUPS" in os.environ:
        assert tab["fast_groups"] == 0
    else:
        fg = 0
        for g in range(K // 8):
            ok = True
            for s in range(8 * g, 8 * g + 8):
                a = tab["attr"][s]
                if a >= 0 and (a >= tab["nshaf"] or region_active(reg[a], w[a])[2]):
                    ok = False
            fg |= int(ok) << g
        assert tab["fast_groups"] == fg
    return c


def region_active(reg, w):
    """[4] bool: region k of a feature row takes part (fv.cpp:155-159: weight != 0, x2 >= x1, y2 >= y1, not x2 == y2 == 0)."""
    return [bool(w[k] != 0 and reg[4 * k + 1] >= reg[4 * k] and reg[4 * k + 3] >= reg[4 * k + 2] and not (reg[4 * k + 1] == 0 and reg[4 * k + 3] == 0))
            for k in range(4)]


def region_corners(reg, k):
    """Indices (a, b, c, d) into the 15 x 15 window of the corners of region k, in the reference's order ((a - b) - c) + d."""
    x1, x2, y1, y2 = (int(v) for v in reg[4 * k:4 * k + 4])
    return (x2 + 1) * 15 + (y2 + 1), x1 * 15 + (y2 + 1), (x2 + 1) * 15 + y1, x1 * 15 + y1


# ---- exact fp32 arithmetic ------------------------------------------------------------------------------------------------------------

def decq4_scr(v):
    """fl64 of the screening pass's "%.4g" round trip of every fp32 value (NaN outside its range): haf_test_decq4_scr_n."""
    v = np.ascontiguousarray(v, np.float32)
    out = np.empty(v.shape, np.float64)
    rc = capi.testlib().haf_test_decq4_scr_n(v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), v.size)
    assert rc == 0
    return out


def _rn32(x):
    """RN to fp32 of an exact rational (ties to even), as a Python float; for finite results inside fp32's normal range or 0."""
    if x == 0:
        return 0.0
    lo = np.float32(float(x))                                       # (float(Fraction) is correctly rounded to fp64, then fp32: a candidate)
    cands = sorted({float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - x), int(np.float32(c).view(np.uint32)) & 1))
    return best


def exact_fma32(q, m, a):
    """fmaf(q, m, a) for fp32 arrays, formed exactly -> (fp32 array, number of entries settled with Fractions).  NaN in, NaN out."""
    q64, m64, a64 = (np.asarray(x, np.float32).astype(np.float64) for x in (q, m, a))
    q64, m64, a64 = np.broadcast_arrays(q64, m64, a64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = q64 * m64                                               # exact: 24 + 24 bits
        s = p + a64
        bb = s - p
        err = (p - (s - bb)) + (a64 - bb)                           # TwoSum: p + a = s + err exactly
        f = s.astype(np.float32)
        lo = np.where(f.astype(np.float64) <= s, f, np.nextafter(f, np.float32(-np.inf)))
        hi = np.where(f.astype(np.float64) >= s, f, np.nextafter(f, np.float32(np.inf)))
        tie = (err != 0) & np.isfinite(s) & (lo != hi) & (s == 0.5 * (lo.astype(np.float64) + hi.astype(np.float64)))
        tiny = np.isfinite(s) & (s != 0) & (np.abs(s) < 2.0 ** -120)
    out = f.copy()
    hard = np.argwhere(tie | tiny)
    for idx in hard:
        idx = tuple(idx)
        out[idx] = np.float32(_rn32(Fraction(float(q64[idx])) * Fraction(float(m64[idx])) + Fraction(float(a64[idx]))))
    return out, len(hard)


# ---- the evaluation list ----------------------------------------------------------------------------------------------------------------

def evaluation_order(mask):
    """Cell ids (roll H + row) W + col of a request's evaluations in the order of the general pre-stages (prestages.hip, "Evaluation
    order"): the masked cells of a row from left to right; its count modulo 64 -- the remainder -- is taken from the row's START; the
    whole chunks of 64 of all rows come first, row by row, then the remainders of all rows."""
    R, H, W = mask.shape
    a, b = [], []
    for r in range(R):
        for i in range(H):
            cols = np.flatnonzero(mask[r, i])
            rem = len(cols) % 64
            ids = (r * H + i) * W + cols
            b.append(ids[:rem])
            a.append(ids[rem:])
    return np.concatenate(a + b).astype(np.int32)


def wave_kinds(cells):
    """bool per wave of 64 consecutive evaluations: "fast" = its 64 cells are consecutive ids (a partly filled last wave is not)."""
    n = len(cells)
    nw = (n + 63) // 64
    fast = np.zeros(nw, bool)
    for w in range(n // 64):
        c = cells[64 * w:64 * w + 64]
        fast[w] = bool((c == c[0] + np.arange(64)).all())
    return fast


def predict_paths(cells, ii, H, W, negflags):
    """'A' / 'B' / 'C' per wave of a low-rank request, from the comment above k_features_serial: a wave that is not fast is C; a fast
    wave is A when its (cloud, roll)'s negative-height flag (bit 1) is clear, the band's bottom row is <= 2 x its top row in each of
    every lane's 15 columns, and every lane's window total -- rounded up as the kernel does, in fp32 -- is below its first corner (its
    second for the window that starts in column 0 of the integral image); else B.
    The window total and its rounding-up COPY the kernel's own fp32 steps (2.0e-7, 1.0001, the column-0 case) instead of restating the
    comment's condition, so an error shared with the kernel there would go unseen.  That is tolerable only because the prediction feeds
    nothing but the coverage assertions, the per-path split of the nu2 statistics and the "+inf on path A" check: every bound on nu2
    itself is asserted on every evaluation whatever its predicted path."""
    f32 = np.float32
    fast = wave_kinds(cells)
    out = []
    for w, fw in enumerate(fast):
        if not fw:
            out.append("C")
            continue
        c0 = int(cells[64 * w])
        br, rem = divmod(c0, H * W)
        i, j = divmod(rem, W)
        band = ii[br][i - 7:i + 8, j - 7:j - 7 + 78].astype(f32)      # 15 rows x 78 columns
        ok = not (int(negflags[br]) & 2)
        colok = band[14] <= f32(2.0) * band[0]
        lane = np.arange(64)
        ok = ok and all(colok[l:l + 15].all() for l in lane)
        tl, bl, tr, brc = band[0, lane], band[14, lane], band[0, lane + 14], band[14, lane + 14]
        tA, tB = (brc - tr).astype(f32), (bl - tl).astype(f32)
        T = (((tA - tB).astype(f32) + (f32(2.0e-7) * (np.abs(tA) + np.abs(tB)).astype(f32)).astype(f32)).astype(f32) * f32(1.0001)).astype(f32)
        dmin = tl.copy()
        if j - 7 == 0:
            dmin[0] = band[0, 1]
        ok = ok and bool((T < dmin).all())
        out.append("A" if ok else "B")
    return np.array(out)


# ---- the reference of a set of evaluations -----------------------------------------------------------------------------------------------

def windows(ii, cells, H, W):
    """fp32 [n, 15, 15]: the integral-image window of every cell id."""
    cells = np.asarray(cells)
    br, rem = np.divmod(cells, H * W)
    i, j = np.divmod(rem, W)
    return np.stack([ii[b][r - 7:r + 8, c - 7:c + 8] for b, r, c in zip(br, i, j)]).astype(np.float32)


def slot_values(orc, win, tab):
    """fp32 [n, 320]: the feature value of every slot's representative attribute (0 for an unused slot), from the oracle."""
    F = np.stack([orc.feature_values(w, tab["nshaf"]) for w in win]) if len(win) else np.zeros((0, orc.n_features), np.float32)
    V = np.zeros((len(win), K), np.float32)
    used = tab["attr"] >= 0
    V[:, used] = F[:, tab["attr"][used]]
    return V, F


def operands(V, tab):
    """u' (fp32 [n, 320], exact fma) and u^ (fp16) of slot values V; -> (u1, uh, number of fma ties settled exactly)."""
    q4f = decq4_scr(V).astype(np.float32)
    u1, hard = exact_fma32(q4f, tab["mul"][None, :], tab["add"][None, :])
    with np.errstate(over="ignore", invalid="ignore"):
        uh = u1.astype(np.float16)
    return q4f, u1, uh, hard


def sums(u1, uh, tab):
    """The five sums in fp64 with the sum of their terms' magnitudes: dict name -> (value [n], magnitude [n])."""
    f = u1.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        du = uh.astype(np.float64) - f
        g, hd, ub, ex = (tab[k].astype(np.float64)[None, :] for k in ("g", "hd", "ub", "extra"))
        t_cr = np.stack([du * g, f * hd])
        su2 = (f * f).sum(axis=1)
        out = dict(su2=(su2, su2), sd2=((du * du).sum(axis=1),) * 2,
                   cr=(t_cr.sum(axis=(0, 2)), np.abs(t_cr).sum(axis=(0, 2))),
                   ub=((f * ub).sum(axis=1), np.abs(f * ub).sum(axis=1)))
        sx2 = su2 + (ex * f * f).sum(axis=1)
        out["sx2"] = (sx2, sx2)
    return out


def _exact_ints(x32):
    """Python integers (object array, same shape): the fp32 values in units of 2^-149 (every finite fp32 is a multiple of it)."""
    m, e = np.frexp(np.asarray(x32, np.float32).astype(np.float64))
    M = np.round(m * 2.0 ** 24).astype(np.int64)                    # exact: 24-bit significands
    sh = (e.astype(np.int64) - 24 + 149)
    assert (sh[M != 0] >= 0).all()
    return M.astype(object) << np.where(M != 0, sh, 0).astype(object)


def v_exact(win, tab, orc):
    """fp64 [n, 320] (correctly rounded; NaN for SHAF and unused slots): sum_k w_k R_k of every HAF slot without rounding, and the
    smallest region sum of the evaluation as the REFERENCE's fp32 arithmetic computes it (min over the HAF slots' active regions, 0
    included) [n]."""
    reg, w = orc.feature_table()
    n = len(win)
    flat = win.reshape(n, 225)
    I = _exact_ints(flat)
    out = np.full((n, K), np.nan)
    rmin = np.zeros(n, np.float32)
    den = 1 << 298
    for s in range(K):
        a = int(tab["attr"][s])
        if a < 0 or tab["shaf"][s]:
            continue
        acc = np.zeros(n, object)
        act = region_active(reg[a], w[a])
        assert not act[3]
        for k in range(3):
            if not act[k]:
                continue
            ca, cb, cc, cd = region_corners(reg[a], k)
            wi = int(Fraction(float(w[a, k])) * (1 << 149))
            acc = acc + wi * (I[:, ca] - I[:, cb] - I[:, cc] + I[:, cd])
            R = (((flat[:, ca] - flat[:, cb]).astype(np.float32) - flat[:, cc]).astype(np.float32) + flat[:, cd]).astype(np.float32)
            rmin = np.minimum(rmin, R)
        out[:, s] = np.array([int(x) / den for x in acc])
    return out, rmin


def v_exact_fsum(win1, tab, orc):
    """The second route for ONE window: math.fsum over the (up to) twelve corner terms w_k x corner, each product exact in fp64."""
    reg, w = orc.feature_table()
    flat = win1.reshape(225).astype(np.float64)
    out = np.full(K, np.nan)
    for s in range(K):
        a = int(tab["attr"][s])
        if a < 0 or tab["shaf"][s]:
            continue
        terms = []
        act = region_active(reg[a], w[a])
        for k in range(3):
            if act[k]:
                ca, cb, cc, cd = region_corners(reg[a], k)
                wk = float(w[a, k])
                terms += [wk * flat[ca], -wk * flat[cb], -wk * flat[cc], wk * flat[cd]]
        out[s] = math.fsum(terms)
    return out


def noise_sum(u1, vex, tab):
    """sum over the HAF slots of (u' - u_lin)^2, u_lin = scr_mul v_exact + scr_add [n] (NaN where an operand is NaN)."""
    haf = tab["pad"] != 0
    with np.errstate(invalid="ignore"):
        ulin = tab["mul"].astype(np.float64)[None, haf] * vex[:, haf] + tab["add"].astype(np.float64)[None, haf]
        d = u1[:, haf].astype(np.float64) - ulin
        return (d * d).sum(axis=1)


def sample(cells, H, W, n_random=500, seed=7):
    """Indices into the evaluation list: every evaluation of three whole grid rows per roll (first, middle, last masked row) plus
    n_random seeded ones, sorted."""
    cells = np.asarray(cells)
    row = cells // W                                                # roll * H + row
    pick = []
    for r in np.unique(cells // (H * W)):
        rows = np.unique(row[cells // (H * W) == r])
        for q in {rows[0], rows[len(rows) // 2], rows[-1]}:
            pick.append(np.flatnonzero(row == q))
    rng = np.random.RandomState(seed)
    pick.append(rng.choice(len(cells), min(n_random, len(cells)), replace=False))
    return np.unique(np.concatenate(pick))


# ---- the cases (tests/test_screen_operands_gpu.py runs them; tests/test_screen_operands_cpu.py proves their coverage on the reference) --

HEIGHTS = ("natural", "block1e6", "pits", "dyadic")
HOLES_GRID = 160


def holes_cloud():
    """The 160-grid cloud with seven 13 x 13 holes of test_screening_feature_paths_agree_with_the_oracle: rows whose chunks of 64 are
    not all runs of neighbours, so fast and per-lane waves share a workgroup."""
    grid = HOLES_GRID
    xyz = models.synthetic_cloud(grid=grid, k=2, seed=12)
    cx = np.floor((xyz[:, 0] + grid * 0.005) / 0.01).astype(int)
    cy = np.floor((xyz[:, 1] + grid * 0.005) / 0.01).astype(int)
    keep = np.ones(len(xyz), bool)
    rng = np.random.RandomState(5)
    for _ in range(7):
        a, b = rng.randint(20, grid - 33, size=2)
        keep &= ~((cx >= a) & (cx < a + 13) & (cy >= b) & (cy < b + 13))
    return np.ascontiguousarray(xyz[keep])


# The launcher's rule (features.hip: launch_features_mode<XMODE_SCREEN>; engine_request.cpp: the request's estimate and `large`),
# restated so that the cases sit on its thresholds, which come from the code (csrc/kernels.h: kSmallEvals, kWaves16Evals, kLargeEvals,
# through haf_test_feature_thresholds); the GPU test asserts the kernel that actually ran through haf_test_feature_form.
def _thresholds():
    out = (C.c_longlong * 3)()
    assert capi.testlib().haf_test_feature_thresholds(out) == 0
    return tuple(int(x) for x in out)


K_SMALL_EVALS, K_WAVES16_EVALS, LARGE_EVALS = _thresholds()
FEAT_SMALL, FEAT_WAVES16, FEAT_WAVES8, FEAT_SERIAL, FEAT_SERIAL_LR = range(5)


def estimated_evals(grid, length_x, length_y, rolls):
    """The host's estimate of a request's evaluations: per roll at most (a + 2)(b + 2) lattice points of the search area's half sizes."""
    a2 = max(0, 2 * (int(length_x) // 2 - 7)) + 2
    b2 = max(0, 2 * (int(length_y) // 2 - 7)) + 2
    return rolls * min((grid - 14) * (grid - 14), a2 * b2)


def predicted_kernel(grid, length_x, length_y, rolls, large_evals=LARGE_EVALS, low_rank=False):
    sel = estimated_evals(grid, length_x, length_y, rolls)
    if sel >= large_evals:
        return FEAT_SERIAL_LR if low_rank else FEAT_SERIAL
    return FEAT_SMALL if sel <= K_SMALL_EVALS else FEAT_WAVES16 if sel <= K_WAVES16_EVALS else FEAT_WAVES8


def smallest_square_above(threshold, rolls, grid):
    """The smallest L with an L x L search area on a grid x grid grid whose estimate exceeds `threshold` (None: no such L)."""
    for L in range(16, grid + 1):
        if estimated_evals(grid, L, L, rolls) > threshold:
            return L
    return None


class Case:
    """One request of the GPU test: name, the kernel it must reach, grid, search area, rolls, cloud, model, environment, form."""

    def __init__(self, row, kernel, grid, lx, ly, heights, model, variant=None, env=(), rolls=2, roll_step=25, two_region=False):
        self.two_region = two_region        # the feature file of two_region_features(), every row a HAF feature
        self.row, self.kernel, self.grid, self.lx, self.ly, self.heights, self.model = row, kernel, grid, lx, ly, heights, model
        self.variant, self.env, self.rolls, self.roll_step = variant, dict(env), rolls, roll_step
        self.id = "-".join([row, heights] + (["form%d" % variant] if variant is not None else []) + (["nofast"] if "HAF_NO_FAST_GROUPS" in self.env else []) +
                           (["tworegion"] if two_region else []))

    def feature_file(self):
        return two_region_features() if self.two_region else FEATURES

    def nshaf(self):
        return 324 if self.two_region else 302

    def oracle(self):
        key = (self.model, self.two_region)
        if key not in _ORACLES:
            from oracle import oracle as O
            _ORACLES[key] = O.Oracle(self.feature_file(), RANGE, hc.model_path(self.model)) if self.two_region else hc.oracle(self.model)
        return _ORACLES[key]

    def cfg_kw(self):
        kw = dict(n_rolls=self.rolls, roll_step_deg=self.roll_step, grid_h=self.grid, grid_w=self.grid, max_points=2 * self.grid * self.grid)
        if self.two_region:
            kw["nr_features_without_shaf"] = self.nshaf()
        return kw

    def in_kw(self):
        return dict(grasp_area_length_x=self.lx, grasp_area_length_y=self.ly)

    def cloud(self):
        return holes_cloud() if self.heights == "holes" else hc.cloud(self.heights, self.grid)

    def environment(self):
        e = dict(HAF_NO_DIRECT="1", HAF_NO_CALIBRATE="1")
        if self.variant is not None:
            e["HAF_SCREEN_VARIANT"] = str(self.variant)
        e.update(self.env)
        return e

    def low_rank(self):
        return self.kernel == FEAT_SERIAL_LR


def cases():
    """The rows of the issue's table.  Every threshold comes from the restated rule above: the smallest square areas above kSmallEvals
    and above 24 576 estimated evaluations (2 rolls), neither `large`."""
    out = []
    for h in HEIGHTS:                                               # k_features_small: hostile_cases.request() as it is
        for v in (0, 2):
            out.append(Case("small", FEAT_SMALL, hc.GRID, 46, hc.GRID, h, "surrogate", v))
    L16 = smallest_square_above(K_SMALL_EVALS, 2, 96)
    L8 = smallest_square_above(K_WAVES16_EVALS, 2, 128)
    assert L16 is not None and L8 is not None and estimated_evals(128, L8, L8, 2) < LARGE_EVALS
    for h in ("natural", "block1e6"):
        out.append(Case("waves16", FEAT_WAVES16, 96, L16, L16, h, "surrogate"))
        out.append(Case("waves8", FEAT_WAVES8, 128, L8, L8, h, "surrogate"))
    serial = dict(HAF_LARGE_EVALS="1", HAF_NO_LR="1")              # (96 x 96 > 8192 cells: without HAF_NO_LR form 2 would take the low-rank kernel)
    for h in HEIGHTS:
        for v in (0, 2):
            out.append(Case("serial", FEAT_SERIAL, 96, 46, 96, h, "surrogate", v, serial))
        out.append(Case("serial", FEAT_SERIAL, 96, 46, 96, h, "surrogate", 0, dict(serial, HAF_NO_FAST_GROUPS="1")))
    out.append(Case("serial", FEAT_SERIAL, HOLES_GRID, HOLES_GRID, HOLES_GRID, "holes", "surrogate", None, serial, rolls=1, roll_step=90))
    lr = dict(HAF_LARGE_EVALS="1", HAF_T0B="0")
    for h in HEIGHTS:
        out.append(Case("lowrank", FEAT_SERIAL_LR, 128, 38, 128, h, "random", 2, lr))
        out.append(Case("lowrank", FEAT_SERIAL_LR, 128, 38, 128, h, "clustered", 3, lr))
    # a flat grid (beyond the issue's four heights): every HAF feature is the residue of two region terms 1e5 times its size, so the "%.4g"
    # rounding -- which carries the noise bound everywhere else -- is far below the fp32 roundings of the products, and the bound rests
    # on what it charges for THOSE (measured: nu2 is 207 x the reference on path A there, 1.002 at the least on path C)
    out.append(Case("lowrank", FEAT_SERIAL_LR, 128, 38, 128, "flat", "random", 2, lr))
    # Every slot a two-region HAF feature (two_region_features): every group is a fast group, so on a path-A wave nu2 is made of
    # pair_math's charges alone -- |q4f - v| and kNbRound (|r0| + |r1|) -- and nothing of screen_pair3's stands in for them.  With the
    # committed feature file the 32 three-region slots' own charge (kNbRound3) hides a kNbRound that is too small.
    for h in ("natural", "flat"):
        out.append(Case("lowrank", FEAT_SERIAL_LR, 128, 38, 128, h, "random", 2, lr, two_region=True))
    return out


_WANT, _TABLES, _ORACLES, _TWO_REGION = {}, {}, {}, []


def two_region_features():
    """Path of a feature file made from the committed one: the third region's weight of every row set to 0.  Used with
    nr_features_without_shaf = 324 (no row takes the SHAF rule), every attribute is then a HAF feature of at most two regions, a linear
    functional of the window.  The range file and the models stay as they are (the attributes' ranges no longer fit the features; the
    engine and the oracle scale them all the same)."""
    if not _TWO_REGION:
        import atexit
        import shutil
        import tempfile
        d = tempfile.mkdtemp(prefix="haf_two_region_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        rows = [ln.split() for ln in open(FEATURES).read().splitlines() if ln.strip()]
        assert all(len(r) == 20 for r in rows)
        with open(os.path.join(d, "Features.txt"), "w") as f:
            for r in rows:
                r[18] = "0"
                f.write("\t".join(r) + "\n")
        _TWO_REGION.append(os.path.join(d, "Features.txt"))
    return _TWO_REGION[0]


def oracle_want(case):
    """orc.run of the case's request, once per process (shared, read-only)."""
    from oracle import oracle as O
    from oracle_inputs import oracle_input
    key = (case.heights, case.model, case.grid, case.lx, case.ly, case.rolls, case.roll_step, case.two_region)
    if key not in _WANT:
        ocfg = O.make_cfg(n_rolls=case.rolls, roll_step_deg=case.roll_step, H=case.grid, W=case.grid, nshaf=case.nshaf())
        want = case.oracle().run(case.cloud(), ocfg, oracle_input(case.in_kw()))
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def table_for(case, form):
    """slot_table of the case's model and grid under the case's table switches, once per process."""
    key = (case.model, case.grid, form, "HAF_NO_FAST_GROUPS" in case.env, "HAF_NO_LR" in case.env, case.two_region)
    if key not in _TABLES:
        saved = {k: os.environ.get(k) for k in ("HAF_NO_FAST_GROUPS", "HAF_NO_LR")}
        try:
            for k in saved:
                os.environ.pop(k, None)
                if k in case.env:
                    os.environ[k] = case.env[k]
            _TABLES[key] = slot_table(hc.model_path(case.model), case.grid, form, case.feature_file(), case.nshaf())
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
    return _TABLES[key]


def form_of(case):
    """The ScreenParams instance that serves the case: the low-rank kernel under a centred variant and every other kernel under
    variants 2 / 3 read screen_cr, variants 0 / 1 screen (screen_lrp in the low-rank form)."""
    v = 0 if case.variant is None else case.variant
    return "screen_cr" if v >= 2 else "screen_lrp" if case.low_rank() else "screen"


def reference(case, tab, ii, cells, idx, exact=False):
    """Everything the kernels must write for the evaluations cells[idx]: dict(V, F, q4f, u1, uh, sums, hard[, vex, rmin, noise])."""
    orc = case.oracle()
    win = windows(ii, np.asarray(cells)[idx], case.grid, case.grid)
    V, F = slot_values(orc, win, tab)
    q4f, u1, uh, hard = operands(V, tab)
    ref = dict(win=win, V=V, F=F, q4f=q4f, u1=u1, uh=uh, sums=sums(u1, uh, tab), hard=hard)
    if exact:
        ref["vex"], ref["rmin"] = v_exact(win, tab, orc)
        ref["noise"] = noise_sum(u1, ref["vex"], tab)
    return ref
