"""What the screening SWEEP must compute, ten-step and low-rank, from a definition (numpy fp64; no csrc/ arithmetic).

The sweep kernels (csrc/screen.hip: k_svm_screen<variant, PART>, k_screen_combine, the list compaction) read the fp16 operand images,
bands and a_x the feature pass left -- tests/screen_operand_cases.py holds those to a definition -- and the SV tile images of the
model.  This module restates what they make of them:

  tiles     the SV tile image: 32 SVs per tile, the fp16 value of (SV j of the tile, slot k) at byte h_image_offset(j, k) -- the same
            formula as the operand image's, screen_operand_cases.image_offset -- and behind the 20 480 image bytes the tail piece
            {t_n [32], coef_n [32]} in fp32; the SVs with coef >= 0 first, padded to whole tiles, then the others; padding columns zero.
            decode_tiles() reads a table of the device-free build (haf_test_host_sweep_tables), model_tiles() makes the same arrays
            from the MODEL FILE: w^_n = RN_fp16(c sum of s_n over the slot's attributes), magnitudes below 2^-14 flushed to zero,
            t_n = fl32(-|c s_n|^2 / 2) over all attributes, coef as fl32; the centred form q^_n = RN_fp16(c sum s_n - (1 + extra) mu),
            b_n = fl32(coef_n 2^(-|c s_n - mu|^2 / 2)), t = 0.  tests/test_sweep_cpu.py holds the one to the other.
  sums      per evaluation and TILE, in fp64 from the fp16 operands and fp16 SV images: z_n = u^.w^_n + t_n;
            PLAIN / SUMSQ  sum coef_n 2^z_n, and sum (coef_n 2^z_n)^2;  CR_EXP  sum b_n psi(z_n), psi(z) = 2^z - 1 - z ln2f;
            CR_POLY  sum b_n z^2 (a2 + a3 z + a4 z^2 + a5 z^3) with the kernel's fp32 constants (its truncation belongs to k_psi in the
            band, not to this comparison); beside each sum the sum of the terms' magnitudes and the per-term share of T_arith below.
            Per tile, so that the class sums P (tiles before sv_tile_neg), N (the rest) and the sums of any SV range of the PART form
            are additions of them.
  tail      screen_tail_vals restated in fp64: val, err1, err2, the choice `centred`, err, the COMBINED unit, label, flagged.
  T_arith   what the kernel's own arithmetic may differ by from these sums.  Reference and kernel read the SAME fp16 operands, so
            no term of the band that bounds operand rounding enters (eta, dn, d_max, lin, abs_c, quad*, cL).  What remains, with its
            BANDS.md row:
              `acc`         per term |coef_n| K_n ln2 acc_rel (|t_n| + sum_k |u^_k w^_nk|)   -- the exact per-term form, not its maximum
                            (CR forms: the same through |psi'(z)| = ln2 |2^z - 1|, second order included)
              `guard_acc0`  1.04 guard_acc0 S (guard_acc0_s for SUMSQ); S = sum |coef| K, S_psi in the CR forms
              COMBINED      1.2e-7 S when the partial sums of SV ranges were combined (`guard_acc0` row)
              `k_psi`       the epilogue's own unit: CR_POLY 10 u per unit of S_psi.  CR_EXP 2.4e-7: per unit of S_psi AND, as the same
                            row says ("2.4e-7 (sum|b| + ln2 ph C_q1) into c_abs"), per unit of sum |b_n| 2^z_n -- an ulp of v_exp_f32
                            is an ulp of 2^z, not of psi(z), which is 1e-3 of it where z is small.  This is the per-term form
                            sum |b_n| (|psi_n| + 1 + ln2 |z_n|) of what screen_finish_cr puts into c_abs for it.
              `D`           its 6e-7 share (the cast of a_x, v_exp_f32, the two products of the common factor) on |val| + |rho|
              `guard_abs`
Low-rank form: the same sums over the decoded svt_lr (192 projected slots, t = 0, the centred form's b_n; CR_POLY of degree 4) from the
projected operands y^ -- on the device the six-step images k_project wrote, on the CPU RN_fp16 of the fp64 product of the decoded projection
tiles (decode_projection) with the operands -- with acc6 in `acc` and the band of lr_finish_band / lr_finish_band_plain evaluated on
the host (haf_test_lr_finish_band).  The projection's own bound is acc10 sum |B^||p^| per component.
The requests are single rolls of a 64-grid whose search area gives each class of evaluation counts (1..31, 33..63, 65..255 and no
multiple of 64, 257..511), and hostile_cases.request()'s two rolls."""
import ctypes as C
import math
import os

import numpy as np

import hostile_cases as hc
import models
import screen_operand_cases as sc
from haf_grasping_amd import capi

SV_TILE, SV_TILE_BYTES, MAT_BYTES = 32, 21504, 20480
# low-rank form (kernels.h: kLrK = 192 projected slots, six k-steps): 12 KiB images, 13 KiB SV tiles, six projection tiles of 20 KiB
LR_K, LR_MAT_BYTES, LR_TILE_BYTES, PROJ_TILE_BYTES = 192, 12288, 13312, 20480
F16_MIN_NORMAL = 2.0 ** -14
U24 = 2.0 ** -24
PLAIN, SUMSQ, CR_EXP, CR_POLY = range(4)
VARIANT_NAMES = ("PLAIN", "SUMSQ", "CR_EXP", "CR_POLY")
LN2F = float(np.float32(0.693147180559945))
PSI_A = tuple(float(np.float32(x)) for x in (0.240226506959101, 0.0555041086648216, 0.00961812910762848, 0.00133335581464284))
# screen.hip: screen_parts()
MAX_PARTS, PART_BLOCKS, MIN_PART_TILES, BLOCK_EVALS = 16, 256, 8, 256
# fp32 operations between the class sums and `err` in screen_tail_vals, counted on its longest path (SUMSQ or PLAIN, the centred
# estimate): P, N, P - N (3); gacc 1.04, + gB, + 1.2e-7, x sabs (4); abs_c sc (1); P + N, - rho, corr, dv - corr (4); the two sums of
# magnitudes, cm + 2.4e-7, their product (4); the two additions, x 1.002, + guard_abs (4): 20.  Every operand is non-negative, so each
# rounding costs at most 2^-24 of err.  + the division of the margin and the test's own division by it: 22; 24 taken.
TAIL_ROUNDINGS = 24
TAU0 = TAIL_ROUNDINGS * U24


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the models of the issue's table -----------------------------------------------------------------------------------------------

MODELS = {
    "m1+1": dict(nsv=2, n_pos=1, seed=41),
    "m32+32": dict(nsv=64, n_pos=32, seed=42),
    "m33+31": dict(nsv=64, n_pos=33, seed=43),
    "m1+95": dict(nsv=96, n_pos=1, seed=44),
    "m256+288": dict(nsv=544, n_pos=256, seed=45),
    "m224+544": dict(nsv=768, n_pos=224, seed=46),
    "m1200": dict(nsv=1200, n_pos=600, seed=47),
    "sparse": dict(nsv=100, n_pos=40, seed=48, density=0.5),
}
# write_clustered_model(260, seed=5) as hostile_cases has it, with rho at the median decision value of hostile_cases.request(): the
# decisions cross zero, so that the polynomial centred-remainder form -- whose band is a few 1e-2 there -- leaves some of them undecided
CLUSTERED = {"clustered0": dict(nsv=260, seed=5, rho=-0.64),
             # ten times the gamma: |z| reaches 1, where the fourth- and fifth-degree terms of the polynomial epilogue weigh something
             "clustered_z": dict(nsv=260, seed=5, gamma=1e-3)}
TILES = {"m1+1": (1, 1), "m32+32": (1, 1), "m33+31": (2, 1), "m1+95": (1, 3), "m256+288": (8, 9), "m224+544": (7, 17), "m1200": (19, 19),
         "sparse": (2, 2)}
_PATHS, _ORACLES, _WANT, _TABLES = {}, {}, {}, {}


def model_path(name):
    """The model file of a row of the table (written once per process), or hostile_cases' surrogate / clustered / random."""
    if name in CLUSTERED and name not in _PATHS:
        _PATHS[name] = models.write_clustered_model(os.path.join(hc._tmp(), "sweep_%s.model" % name), **CLUSTERED[name])
    if name not in MODELS and name not in _PATHS:
        return hc.model_path(name)
    if name not in _PATHS:
        kw = dict(MODELS[name])
        nsv = kw.pop("nsv")
        _PATHS[name] = models.write_random_model(os.path.join(hc._tmp(), "sweep_%s.model" % name.replace("+", "_")), nsv, balanced=True, **kw)
    return _PATHS[name]


def oracle(name):
    if name not in _ORACLES:
        from oracle import oracle as O
        _ORACLES[name] = O.Oracle(sc.FEATURES, sc.RANGE, model_path(name))
    return _ORACLES[name]


# ---- the requests ------------------------------------------------------------------------------------------------------------------

GRID = 64
CLASSES = {"n1..31": (1, 31), "n33..63": (33, 63), "n65..255": (65, 255), "n257..511": (257, 511)}
# search areas (cells) of one roll of the 64-grid whose mask count falls into each class: found on the CPU from the oracle's mask
# (tests/test_sweep_cpu.py asserts the class of each)
AREAS = {"n1..31": (18, 18), "n33..63": (20, 20), "n65..255": (24, 24), "n257..511": (32, 34)}


class Request:
    def __init__(self, name, grid, lx, ly, rolls=1, roll_step=25, heights="natural"):
        self.name, self.grid, self.lx, self.ly, self.rolls, self.roll_step, self.heights = name, grid, lx, ly, rolls, roll_step, heights

    def cfg_kw(self):
        return dict(n_rolls=self.rolls, roll_step_deg=self.roll_step, grid_h=self.grid, grid_w=self.grid, max_points=2 * self.grid * self.grid)

    def in_kw(self):
        return dict(grasp_area_length_x=self.lx, grasp_area_length_y=self.ly)

    def cloud(self):
        return hc.cloud(self.heights, self.grid)


def request(name, heights="natural"):
    if name == "hostile":
        return Request(name, hc.GRID, 46, hc.GRID, rolls=2, heights=heights)
    if name == "rolls27":         # 27 rolls of the 64-grid: (64 - 14)^2 x 27 = 67 500 evaluation slots, 264 workgroups, 1 056 flag words
        return Request(name, GRID, 24, 24, rolls=27, roll_step=5, heights=heights)
    if name.startswith("lr_"):    # the small classes on the 128-grid, one roll: with HAF_LARGE_EVALS = 1 the low-rank form serves them
        lx, ly = AREAS[name[3:]]
        return Request(name, 128, lx, ly, heights=heights)
    if name == "lowrank":         # screen_operand_cases' `lowrank` rows: with HAF_LARGE_EVALS = 1 the low-rank form serves it
        return Request(name, 128, 38, 128, rolls=2, heights=heights)
    lx, ly = AREAS[name]
    return Request(name, GRID, lx, ly, heights=heights)


def oracle_want(model, req):
    """orc.run of the request against the model, once per process (shared, read-only)."""
    from oracle import oracle as O
    from oracle_inputs import oracle_input
    key = (model, req.name, req.heights)
    if key not in _WANT:
        ocfg = O.make_cfg(n_rolls=req.rolls, roll_step_deg=req.roll_step, H=req.grid, W=req.grid)
        want = oracle(model).run(req.cloud(), ocfg, oracle_input(req.in_kw()))
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


# ---- the sweep's tables ------------------------------------------------------------------------------------------------------------

def sweep_tables(model, grid):
    """haf_test_host_sweep_tables of the model on a grid x grid engine (no device): dict(svt0, svt0_cr: uint8 or None; n_sv_tiles,
    sv_tile_neg, gv0, gv1; rho, guard_acc0, guard_acc0_s, guard_abs, sqrt_cmax, B0, rho_cr, acc_rel, acc_rel_cr, compact_words)."""
    key = (model, grid)
    if key in _TABLES:
        return _TABLES[key]
    cfg = capi.default_config(feature_file=sc.FEATURES, range_file=sc.RANGE, model_file=model_path(model), grid_h=grid, grid_w=grid)
    out = {}
    ints, scal, msg = np.zeros(4, np.int32), np.zeros(12), C.create_string_buffer(512)
    for which, name in ((0, "svt0"), (1, "svt0_cr"), (2, "svt_lr"), (3, "lr_btiles")):
        n = C.c_longlong()
        rc = capi.testlib().haf_test_host_sweep_tables(C.byref(cfg), sc.KAPPA, sc.KAPPA, which, None, 0, C.byref(n), _p(ints), _p(scal), msg, len(msg))
        assert rc == 0, (rc, msg.value.decode())
        buf = np.zeros(n.value, np.uint8)
        if n.value:
            rc = capi.testlib().haf_test_host_sweep_tables(C.byref(cfg), sc.KAPPA, sc.KAPPA, which, _p(buf), n.value, C.byref(n), _p(ints), _p(scal), msg, len(msg))
            assert rc == 0, (rc, msg.value.decode())
        out[name] = buf if n.value else None
    out.update(n_sv_tiles=int(ints[0]), sv_tile_neg=int(ints[1]), gv0=int(ints[2]), gv1=int(ints[3]))
    out.update(zip(("rho", "guard_acc0", "guard_acc0_s", "guard_abs", "sqrt_cmax", "B0", "rho_cr", "acc_rel", "acc_rel_cr", "acc6", "acc10"), (float(x) for x in scal)))
    out["compact_words"] = int(scal[11])
    _TABLES[key] = out
    return out


_HALF_INDEX = np.array([[sc.image_offset(j, k) // 2 for k in range(sc.K)] for j in range(SV_TILE)])


def decode_tiles(raw, n_tiles, lr=False):
    """(W fp16 [n_tiles * 32, 320], t fp32 [n_tiles * 32], coef fp32 [n_tiles * 32], pad: the tail piece's unused bytes) of a tile table.
    lr: the low-rank form's table (192 slots, 13 KiB tiles; the same offsets for slots below 192)."""
    tile_bytes, mat, K = (LR_TILE_BYTES, LR_MAT_BYTES, LR_K) if lr else (SV_TILE_BYTES, MAT_BYTES, sc.K)
    assert raw is not None and len(raw) == n_tiles * tile_bytes, (None if raw is None else len(raw), n_tiles)
    tiles = raw.reshape(n_tiles, tile_bytes)
    img = np.ascontiguousarray(tiles[:, :mat]).view(np.uint16).reshape(n_tiles, mat // 2)
    W = img[:, _HALF_INDEX[:, :K]].view(np.float16).reshape(n_tiles * SV_TILE, K)
    tail = np.ascontiguousarray(tiles[:, mat:]).view(np.float32).reshape(n_tiles, -1)
    return W, tail[:, :SV_TILE].reshape(-1).copy(), tail[:, SV_TILE:2 * SV_TILE].reshape(-1).copy(), tail[:, 2 * SV_TILE:]


def decode_projection(raw):
    """B^ fp16 [320 input slots, 192 output slots] of lr_btiles: six projection tiles (32 output slots each) in the layout of a ten-step
    SV tile image; row j of a tile is output slot 32 sp + 8 g + r + 4 n, n = j / 16, g = (j % 16) / 4, r = j % 4 (screen.hip: k_project --
    the rows are permuted so that a lane's accumulators are its eight halves of the six-step image)."""
    assert raw is not None and len(raw) == (LR_K // 32) * PROJ_TILE_BYTES
    img = raw.view(np.uint16).reshape(LR_K // 32, PROJ_TILE_BYTES // 2)[:, _HALF_INDEX].view(np.float16)     # [sp, j, k]
    B = np.zeros((sc.K, LR_K), np.float16)
    for sp in range(LR_K // 32):
        for j in range(32):
            B[:, 32 * sp + 8 * ((j % 16) // 4) + (j % 4) + 4 * (j // 16)] = img[sp, j]
    return B


def lr_rows(Y, evals):
    """fp16 [len(evals), 192]: the projected operands of the given evaluations out of the six-step images Y (uint8, whole tiles)."""
    tiles = np.ascontiguousarray(Y[:len(Y) // LR_MAT_BYTES * LR_MAT_BYTES]).view(np.uint16).reshape(-1, LR_MAT_BYTES // 2)
    evals = np.asarray(evals)
    return tiles[(evals // 32)[:, None], _HALF_INDEX[:, :LR_K][evals % 32]].view(np.float16)


def lr_finish_band(model, grid, raw, variant):
    """haf_test_lr_finish_band: lr_finish_band_plain (PLAIN) / lr_finish_band (CR_EXP, CR_POLY) on the host -> band [n, 8] fp32."""
    cfg = capi.default_config(feature_file=sc.FEATURES, range_file=sc.RANGE, model_file=model_path(model), grid_h=grid, grid_w=grid)
    raw = np.ascontiguousarray(raw, np.float32)
    out, msg = np.zeros((len(raw), 8), np.float32), C.create_string_buffer(512)
    rc = capi.testlib().haf_test_lr_finish_band(C.byref(cfg), sc.KAPPA, sc.KAPPA, _p(raw), len(raw), {PLAIN: 0, CR_EXP: 1, CR_POLY: 2}[variant],
                                                _p(out), msg, len(msg))
    assert rc == 0, (rc, msg.value.decode())
    return out


def tile_rule(coef):
    """(n_sv_tiles, sv_tile_neg, column of every SV) by the restated rule: coef >= 0 first, padded to whole tiles, then the others."""
    pos = coef >= 0
    npos, nneg = int(pos.sum()), int((~pos).sum())
    pt = (npos + SV_TILE - 1) // SV_TILE
    col = np.zeros(len(coef), np.int64)
    col[pos] = np.arange(npos)
    col[~pos] = pt * SV_TILE + np.arange(nneg)
    nt = pt + (nneg + SV_TILE - 1) // SV_TILE
    return nt, (pt if nneg else nt), col


def _f16_flushed(x):
    h = np.asarray(x, np.float64).astype(np.float32).astype(np.float16)
    return np.where(np.abs(h.astype(np.float64)) < F16_MIN_NORMAL, np.float16(0), h)


def slot_members(orc, tab):
    """For every used slot the attributes (rows of the feature file) it stands for: the rule of screen_operand_cases.check_table."""
    lower, upper, fmin, fmax, present = orc.range_table()
    reg, w = orc.feature_table()
    kept = [a for a in range(min(len(w), 323)) if present[a + 1] and fmin[a + 1] != fmax[a + 1]]

    def key(a):
        act = sc.region_active(reg[a], w[a])
        return (tuple((k, sc.region_corners(reg[a], k), float(w[a, k])) for k in range(3) if act[k]), float(fmin[a + 1]), float(fmax[a + 1]), a >= tab["nshaf"])
    rep_of, members = {}, {}
    for a in kept:
        r = rep_of.setdefault(key(a), a)
        members.setdefault(r, []).append(a)
    out = []
    for s in range(sc.K):
        a = int(tab["attr"][s])
        out.append(members[a] if a >= 0 else [])
    return out


def model_tiles(orc, tab, centred=False):
    """The SV tile arrays from the MODEL FILE (see the module's docstring) -> (W fp16 [n_pad, 320], t fp32, coef fp32, n_tiles, neg,
    exact: dict(W fp64 [n_sv, 320] slot-space operands c s (centred: minus (1 + extra) mu), t fp64, coef fp64, col)).  tab: the slot
    table of the form (screen_operand_cases.slot_table): plain for centred=False, screen_cr for centred=True."""
    m = orc.model_arrays()
    c = tab["c"]
    sv, coef = m["sv"], m["coef"]
    n_sv, dim = sv.shape
    nt, neg, col = tile_rule(coef)
    members = slot_members(orc, tab)
    Wx = np.zeros((n_sv, sc.K))
    in_slot = np.full(dim, -1)
    for s, att in enumerate(members):
        for a in att:
            if a < dim:
                Wx[:, s] += sv[:, a] * c
                in_slot[a] = s
    if centred:
        mu, mult = tab["mu"], 1.0 + tab["extra"].astype(np.float64)
        full = sv * c
        for a in range(dim):
            if in_slot[a] >= 0:
                full[:, a] -= mu[in_slot[a]]
        qq = (full * full).sum(axis=1)
        Wx = Wx - (mult * mu)[None, :] * (np.array([len(a) > 0 for a in members])[None, :])
        tx = np.zeros(n_sv)
        cx = coef * np.exp2(-0.5 * qq)
    else:
        tx = -0.5 * ((sv * c) ** 2).sum(axis=1)
        cx = coef.copy()
    W = np.zeros((nt * SV_TILE, sc.K), np.float16)
    t, cf = np.zeros(nt * SV_TILE, np.float32), np.zeros(nt * SV_TILE, np.float32)
    W[col] = _f16_flushed(Wx)
    t[col] = tx.astype(np.float32)
    cf[col] = cx.astype(np.float32)
    return W, t, cf, nt, neg, dict(W=Wx, t=tx, coef=cx, col=col)


# ---- the sums ----------------------------------------------------------------------------------------------------------------------

def tile_sums(U, W, t, coef, variant, acc_rel, exact=False, degree=5):
    """Per evaluation and tile, fp64: dict(sum, mag, sq, acc, unit) [n, n_tiles] -- the sum of the terms, of their magnitudes, of their
    squares (PLAIN / SUMSQ), the per-term accumulation share of T_arith, and the epilogue's own unit (CR forms).  U: fp16 or fp64
    operands [n, 320]; W, t, coef as decode_tiles gives them.  Non-finite operands give non-finite sums.  exact: psi itself with
    ln 2 in fp64 in both CR forms (the decision function, not the kernel's epilogue)."""
    U64, W64 = np.asarray(U).astype(np.float64), np.asarray(W).astype(np.float64)
    t64, c64 = np.asarray(t).astype(np.float64), np.asarray(coef).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        Z = U64 @ W64.T + t64[None, :]
        A = np.abs(U64) @ np.abs(W64).T + np.abs(t64)[None, :]
        dz = acc_rel * A
        if variant in (PLAIN, SUMSQ):
            term = c64[None, :] * np.exp2(Z)
            acc = np.abs(term) * math.log(2.0) * dz
            unit = np.zeros_like(term)
        elif variant == CR_EXP or exact:
            e = np.exp2(Z)
            psi = (e - 1.0) - Z * (math.log(2.0) if exact else LN2F)
            term = c64[None, :] * psi
            slope = math.log(2.0) * (np.abs(e - 1.0) + e * math.log(2.0) * dz * 1.01)
            acc = np.abs(c64)[None, :] * slope * dz
            unit = 2.4e-7 * np.abs(c64)[None, :] * (np.abs(psi) + 1.0 + math.log(2.0) * np.abs(Z))
        else:
            a2, a3, a4, a5 = PSI_A if degree == 5 else PSI_A[:3] + (0.0,)      # (the low-rank sweep's polynomial has degree 4)
            poly = lambda z: z * z * (a2 + z * (a3 + z * (a4 + z * a5)))
            dpoly = lambda z: np.abs(z) * (2 * a2 + np.abs(z) * (3 * a3 + np.abs(z) * (4 * a4 + np.abs(z) * 5 * a5)))
            term = c64[None, :] * poly(Z)
            acc = np.abs(c64)[None, :] * dpoly(np.abs(Z) + dz) * dz
            unit = 10.0 * U24 * np.abs(term)
        n, nt = len(U64), len(t64) // SV_TILE
        per = lambda x: x.reshape(n, nt, SV_TILE).sum(axis=2)
        return dict(sum=per(term), mag=per(np.abs(term)), sq=per(term * term), acc=per(acc), unit=per(unit))


def class_sums(ts, neg, tiles=None):
    """P, N (the sums over the tiles before / from `neg`), their magnitudes, squares and T_arith shares, over all tiles or a subset."""
    nt = ts["sum"].shape[1]
    sel = np.zeros(nt, bool)
    sel[np.arange(nt) if tiles is None else np.asarray(tiles, int)] = True
    pos, ng = sel & (np.arange(nt) < neg), sel & (np.arange(nt) >= neg)
    g = lambda k, m: ts[k][:, m].sum(axis=1)
    return dict(P=g("sum", pos), N=g("sum", ng), magP=g("mag", pos), magN=g("mag", ng), sq=g("sq", sel), acc=g("acc", sel), unit=g("unit", sel))


def screen_parts(n_evals, n_tiles, neg, forced):
    """screen.hip: screen_parts(), restated."""
    blocks = (n_evals + BLOCK_EVALS - 1) // BLOCK_EVALS
    k = forced if forced > 0 else (512 // blocks if blocks > 0 else 1)
    k = min(k, MAX_PARTS)
    if forced <= 0:
        k = min(k, n_tiles // MIN_PART_TILES)
    k = min(k, min(neg, n_tiles - neg))
    return max(k, 1)


def part_tiles(k, K, n_tiles, neg):
    """The tiles slice k of K sweeps (k_svm_screen<., true>): the k-th share of the non-negative tiles and of the negative ones."""
    nn = n_tiles - neg
    return list(range(neg * k // K, neg * (k + 1) // K)) + list(range(neg + nn * k // K, neg + nn * (k + 1) // K))


def splits(launcher_parts, blocks, n_tiles):
    """launch_svm_screen's rule for the PART form (parts: 0 the engine's rule, 1 never, n forced)."""
    return launcher_parts != 1 and blocks <= PART_BLOCKS and (launcher_parts > 1 or n_tiles >= 4 * MIN_PART_TILES)


# ---- the tail ----------------------------------------------------------------------------------------------------------------------

def tail(cs, band, nax, tb, variant, combined):
    """screen_tail_vals in fp64 on class sums cs (class_sums), the 8 band floats and a_x per evaluation, the table scalars tb ->
    dict(val, err, err1, err2, centred, S, T_arith, flagged, label).  NaN in, NaN out (and flagged)."""
    g = np.asarray(band, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        scf = np.exp2(np.asarray(nax, np.float64))
        gacc = tb["guard_acc0_s"] if variant == SUMSQ else tb["guard_acc0"]
        comb = 1.2e-7 if combined else 0.0
        if variant in (CR_EXP, CR_POLY):
            Ps, Ns = cs["P"], cs["N"]
            val = scf * ((tb["B0"] + g[:, 0]) + (Ps + Ns)) - tb["rho_cr"]
            spsi = (Ps - Ns) * (1.0000003 if combined else 1.0)
            raw = g[:, 1] + (gacc * 1.04 + g[:, 2]) * spsi + 1.8e-7 * (np.abs(g[:, 0]) + np.abs(Ps) + np.abs(Ns))
            rho = abs(float(np.float32(tb["rho_cr"])))
            err = (raw * scf * 1.002 + (g[:, 3] + 2.4e-7) * (np.abs(val) + rho)) * 1.002 + tb["guard_abs"]
            err1 = err2 = err
            centred = np.zeros(len(g), bool)
            S = scf * (cs["magP"] + cs["magN"])
        else:
            P, N = cs["P"] * scf, cs["N"] * scf
            dv = (P + N) - tb["rho"]
            sabs = P - N
            w2 = np.sqrt(cs["sq"]) * scf if variant == SUMSQ else tb["sqrt_cmax"] * np.sqrt(sabs)
            lin = np.fmin(g[:, 0] * w2, g[:, 2] * sabs)
            sterm = (gacc * 1.04 + g[:, 1] + comb) * sabs
            rho = abs(tb["rho"])
            err1 = (lin + sterm + g[:, 3] * (np.abs(dv) + rho)) * 1.002 + tb["guard_abs"]
            corr = g[:, 4] * scf
            dvc = dv - corr
            err2 = (g[:, 5] * scf + sterm + (g[:, 3] + 2.4e-7) * (np.abs(dvc) + np.abs(corr) + rho)) * 1.002 + tb["guard_abs"]
            centred = err2 < err1
            val, err = np.where(centred, dvc, dv), np.where(centred, err2, err1)
            S = scf * (cs["magP"] + cs["magN"])
        T = scf * (cs["acc"] + cs["unit"]) + (1.04 * gacc + comb) * S + 6.0e-7 * (np.abs(val) + rho) + tb["guard_abs"]
        flagged = ~(np.abs(val) > err)
    return dict(val=val, err=err, err1=err1, err2=err2, centred=centred, S=S, T=T, flagged=flagged,
                label=np.where(val > 0, tb["gv0"], tb["gv1"]), sc=scf)


def part_tolerance(cs, tb, variant):
    """What a slice's two class sums (raw, before the common factor) may differ by: the slice's share of T_arith -- its terms'
    accumulation and epilogue shares and 1.04 guard_acc0 of its own S."""
    gacc = tb["guard_acc0_s"] if variant == SUMSQ else tb["guard_acc0"]
    return cs["acc"] + cs["unit"] + 1.04 * gacc * (cs["magP"] + cs["magN"])


def flag_bits(words, n):
    """bool [n]: bit e % 64 of word e / 64."""
    w = np.asarray(words, np.uint64)
    e = np.arange(n)
    return ((w[e // 64] >> (e % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


class OperandCase:
    """What screen_operand_cases.reference() reads of a case: the oracle and the grid."""

    def __init__(self, model, req):
        self.model, self.grid, self.req = model, req.grid, req

    def oracle(self):
        return oracle(self.model)


_SLOT_TABLES = {}


def slot_table(model, grid, form):
    """screen_operand_cases.slot_table of the model, once per process (every call of a device-free hook builds the model's tables anew)."""
    key = (model, grid, form)
    if key not in _SLOT_TABLES:
        _SLOT_TABLES[key] = sc.slot_table(model_path(model), grid, form)
    return _SLOT_TABLES[key]


def host_screen_finish(model, grid, form, cr_poly, sums):
    """haf_test_host_screen_finish: screen_finish with the constants of the device-free build -> (band [n, 8] fp32, a_x [n] fp32)."""
    cfg = capi.default_config(feature_file=sc.FEATURES, range_file=sc.RANGE, model_file=model_path(model), grid_h=grid, grid_w=grid)
    sums = np.ascontiguousarray(sums, np.float64)
    band, nax, msg = np.zeros((len(sums), 8), np.float32), np.zeros(len(sums), np.float32), C.create_string_buffer(512)
    rc = capi.testlib().haf_test_host_screen_finish(C.byref(cfg), sc.KAPPA, sc.KAPPA, sc.FORMS.index(form), int(cr_poly), _p(sums), len(sums),
                                                    _p(band), _p(nax), msg, len(msg))
    assert rc == 0, (rc, msg.value.decode())
    return band, nax
