"""The reference of the screening sweep, ten-step and low-rank (tests/sweep_cases.py), held to the model file and to the oracle, without a GPU.

  * the SV tile images of the device-free table build (haf_test_host_sweep_tables) decode to what the MODEL FILE defines: svt0 and svt0_cr
    bit for bit for every model of the table; padding columns and the tail piece's unused bytes are zero; n_sv_tiles and sv_tile_neg are
    the restated rule's.  The low-rank tables at the 128-grid (test_low_rank_tables_decode): lr_btiles is a matrix with orthonormal
    columns up to its fp16 rounding, svt_lr carries t = 0, the centred form's b_n bit for bit and q~^_n within 4 x 2^-11 |q_n| of the
    least-squares coordinates of the model file's centred SV in those columns.
  * the reference is the SVM: with u^, w^ replaced by the exact operands (c x of the oracle's scaled row, c s_n) its decision value is
    the oracle's within 1e-12 S, for every evaluation of every case, in the plain and in the centred-remainder form.
  * the band is sound for EVERY evaluation, decided or not: with the fp16 operands of screen_operand_cases.reference (which
    tests/test_screen_operands_gpu.py holds bit-equal to the device's), the band of screen_finish on the host and the decoded tiles,
    |val_ref - dec_oracle| + T_arith <= err_ref.  Requests above 1 200 evaluations are SAMPLED (three whole grid rows per roll and 300
    seeded evaluations, screen_operand_cases.sample), except `clustered0`, which runs whole.  The same for the low-rank form on the
    `lowrank` request, from the oracle alone (_evaluate_lr).
  * coverage from the reference alone: every request class, both branches of `centred`, and at least 20 decided and 20 flagged evaluations
    away from the band's edge in each of ten families: PLAIN, SUMSQ, CR_EXP, CR_POLY, PART, list, low-rank plain / CR_EXP / CR_POLY, gather."""
import math

import numpy as np
import pytest

import hostile_cases as hc
import screen_operand_cases as sc
import sweep_cases as sw

SMALL_MODELS = tuple(sw.MODELS)
COVER, _DONE = {}, set()


def _cells(want):
    cells = sc.evaluation_order(want["mask"])
    assert len(cells) == want["n_evals"]
    return cells


@pytest.mark.parametrize("model", SMALL_MODELS + ("surrogate", "clustered"))
def test_tile_images_decode_to_the_model_file(model):
    orc, tb = sw.oracle(model), sw.sweep_tables(model, sw.GRID)
    if model in sw.TILES:
        assert (tb["sv_tile_neg"], tb["n_sv_tiles"] - tb["sv_tile_neg"]) == sw.TILES[model]
    for centred, key, form in ((False, "svt0", "screen"), (True, "svt0_cr", "screen_cr")):
        tab = sw.slot_table(model, sw.GRID, form)
        assert tab is not None and tb[key] is not None, (model, form)
        sc.check_table(orc, orc.model_arrays()["gamma"], tab)
        W, t, cf, pad = sw.decode_tiles(tb[key], tb["n_sv_tiles"])
        W2, t2, cf2, nt, neg, ex = sw.model_tiles(orc, tab, centred)
        assert (nt, neg) == (tb["n_sv_tiles"], tb["sv_tile_neg"])
        assert (W.view(np.uint16) == W2.view(np.uint16)).all(), (model, form, "fp16 image")
        assert (t.view(np.uint32) == t2.view(np.uint32)).all() and (cf.view(np.uint32) == cf2.view(np.uint32)).all(), (model, form, "tail piece")
        assert (pad.view(np.uint32) == 0).all()
        live = np.zeros(nt * sw.SV_TILE, bool)
        live[ex["col"]] = True
        assert (W[~live].view(np.uint16) == 0).all() and (t[~live] == 0).all() and (cf[~live] == 0).all(), "padding columns"
        assert (cf[:neg * sw.SV_TILE][live[:neg * sw.SV_TILE]] >= 0).all() and (cf[neg * sw.SV_TILE:][live[neg * sw.SV_TILE:]] < 0).all()
        if centred:
            assert (t == 0).all()


def test_request_classes():
    for name, (lo, hi) in sw.CLASSES.items():
        n = sw.oracle_want("m33+31", sw.request(name))["n_evals"]
        assert lo <= n <= hi and n % 64 != 0, (name, n)
    assert 1500 <= sw.oracle_want("surrogate", sw.request("hostile"))["n_evals"] <= 6000


def _exact_rows(orc, want, cells, grid):
    """c x per SLOT-defining attribute is taken from the oracle's scaled rows: x [n, 323] through both text round trips."""
    skip = np.zeros(325, np.uint8)
    skip[324] = 1
    X = []
    for cid in cells:
        r, rem = divmod(int(cid), grid * grid)
        i, j = divmod(rem, grid)
        f = orc.feature_values(want["integral"][r][i - 7:i + 8, j - 7:j + 8])
        X.append(orc.scale_row(hc.q4_row(orc, f), 323, skip))
    return np.array(X)


def ts_abs(Z):
    """psi(z) = 2^z - 1 - z ln 2"""
    return np.exp2(Z) - 1.0 - Z * math.log(2.0)


def _cases():
    # every model of the table at the largest class, the three models of the GPU test's matrix at every class (each device-free hook
    # call builds the model's tables anew: a second per call)
    out = [(m, r, "natural") for m in SMALL_MODELS for r in sw.CLASSES if r == "n257..511" or m in ("m1+1", "m33+31", "m256+288")]
    out += [(m, "hostile", "natural") for m in ("surrogate", "clustered")]
    out += [("m33+31", "n257..511", "pits"), ("m33+31", "hostile", "block1e6"), ("surrogate", "hostile", "scale8"), ("surrogate", "hostile", "pits")]
    out += [("clustered0", "hostile", "natural"), ("clustered0", "hostile", "pits")]     # (every evaluation: FULL)
    return out


FULL = ("clustered0",)


@pytest.mark.parametrize("model,rname,heights", _cases(), ids=lambda x: str(x))
def test_reference_is_the_svm_and_the_band_is_sound(model, rname, heights):
    _evaluate(model, rname, heights)


def _evaluate(model, rname, heights):
    """Asserts both properties for one case and counts its evaluations into COVER (once per process)."""
    if (model, rname, heights) in _DONE:
        return
    _DONE.add((model, rname, heights))
    req = sw.request(rname, heights)
    orc, want = sw.oracle(model), sw.oracle_want(model, req)
    G = req.grid
    cells = _cells(want)
    if len(cells) > 1200 and model not in FULL:
        cells = cells[sc.sample(cells, G, G, n_random=300)]
    br, rem = np.divmod(cells, G * G)
    dec = want["dec"][br, rem // G, rem % G]
    sabs = want["sabs"][br, rem // G, rem % G]
    tb = sw.sweep_tables(model, G)
    m = orc.model_arrays()
    X = _exact_rows(orc, want, cells, G)
    for centred, key, form, variants in ((False, "svt0", "screen", (sw.PLAIN, sw.SUMSQ)), (True, "svt0_cr", "screen_cr", (sw.CR_EXP, sw.CR_POLY))):
        tab = sw.slot_table(model, G, form)
        members = sw.slot_members(orc, tab)
        _, _, _, nt, neg, ex = sw.model_tiles(orc, tab, centred)
        # ---- the reference is the SVM: exact operands ----
        Ux = np.zeros((len(cells), sc.K))
        mult = 1.0 + tab["extra"].astype(np.float64)
        for s, att in enumerate(members):
            if att:
                Ux[:, s] = tab["c"] * X[:, att[0]] - (tab["mu"][s] if centred else 0.0)
                for a in att[1:]:
                    assert (X[:, a] == X[:, att[0]]).all(), "attributes of one slot take one value"
        Wp = np.zeros((nt * sw.SV_TILE, sc.K))
        tp, cp = np.zeros(nt * sw.SV_TILE), np.zeros(nt * sw.SV_TILE)
        Wp[ex["col"]], tp[ex["col"]], cp[ex["col"]] = ex["W"], ex["t"], ex["coef"]
        # (the common factor inside the exponent, z_n + t_n - |u|^2 / 2 = -|u - w_n|^2 / 2 <= 0: hostile heights put |u|^2 beyond 2000)
        ax = 0.5 * (mult[None, :] * Ux * Ux).sum(axis=1)
        K = np.exp2(Ux @ Wp.T + tp[None, :] - ax[:, None])
        val = (cp[None, :] * K).sum(axis=1) - m["rho"]
        S = (np.abs(cp)[None, :] * K).sum(axis=1)
        fin = np.isfinite(dec)
        assert (np.abs(val[fin] - dec[fin]) <= 1e-12 * np.maximum(S[fin], sabs[fin]) + 1e-300).all(), \
            (form, float((np.abs(val[fin] - dec[fin]) / np.maximum(S[fin], 1e-300)).max()))
        # ... and the reference's route to the same number: per-tile sums, class sums, the common factor outside (centred form: B0 + L + R)
        ts = sw.tile_sums(Ux, Wp, tp, cp, sw.CR_EXP if centred else sw.PLAIN, 0.0, exact=True)
        cs = sw.class_sums(ts, neg)
        with np.errstate(invalid="ignore", over="ignore"):
            A = np.exp2(-ax)
            if centred:
                Z = Ux @ Wp.T
                val2 = A * (cp.sum() + math.log(2.0) * (Z * cp[None, :]).sum(axis=1) + cs["P"] + cs["N"]) - m["rho"]
                S2 = A * (np.abs(cp)[None, :] * (np.abs(ts_abs(Z)) + 1.0 + math.log(2.0) * np.abs(Z))).sum(axis=1)
            else:
                val2, S2 = A * (cs["P"] + cs["N"]) - m["rho"], A * (cs["magP"] + cs["magN"])
        tame = fin & np.isfinite(val2) & (ax < 500.0)
        assert tame.any() and (np.abs(val2[tame] - val[tame]) <= 1e-12 * S2[tame] + 1e-300).all(), (form, "per-tile route")
        # ---- the band bounds the reference's error on every evaluation ----
        ref = sc.reference(sw.OperandCase(model, req), tab, want["integral"], cells, np.arange(len(cells)))
        Sm = ref["sums"]
        sums5 = np.stack([Sm["su2"][0], Sm["sd2"][0], Sm["sx2"][0], Sm["cr"][0], Sm["ub"][0]], 1)
        W, t, cf, _ = sw.decode_tiles(tb[key], tb["n_sv_tiles"])
        bands = {}
        for v in variants:
            if (form, v == sw.CR_POLY) not in bands:            # (PLAIN and SUMSQ read one band)
                bands[(form, v == sw.CR_POLY)] = sw.host_screen_finish(model, G, form, v == sw.CR_POLY, sums5)
            band, nax = bands[(form, v == sw.CR_POLY)]
            ts = sw.tile_sums(ref["uh"], W, t, cf, v, tb["acc_rel_cr" if centred else "acc_rel"])
            tl = sw.tail(sw.class_sums(ts, neg), band, nax, tb, v, combined=False)
            ok = np.isfinite(tl["err"]) & np.isfinite(tl["val"]) & fin
            with np.errstate(invalid="ignore"):
                hole = ok & ~(np.abs(tl["val"] - dec) + tl["T"] <= tl["err"])
            assert not hole.any(), (sw.VARIANT_NAMES[v], int(hole.sum()), "first", int(np.flatnonzero(hole)[0]),
                                    float(np.abs(tl["val"] - dec)[hole][0]), float(tl["T"][hole][0]), float(tl["err"][hole][0]))
            assert tl["flagged"][~ok].all(), "a non-finite value or band is never trusted"
            with np.errstate(invalid="ignore", divide="ignore"):
                away = ok & ~(np.abs(np.abs(tl["val"]) - tl["err"]) <= sw.TAU0 * tl["err"] + tl["T"])
            _count("PART", sw.tail(sw.class_sums(ts, neg), band, nax, tb, v, combined=True), ok)      # (the same sums, combined: + 1.2e-7 S)
            if v == sw.PLAIN:
                plain_flagged = tl["flagged"].copy()
            if v == sw.CR_EXP:                                  # tier 0b's list mode: the centred-remainder form on what the plain form flags
                _count("LIST", {k: (x[plain_flagged] if isinstance(x, np.ndarray) else x) for k, x in tl.items()}, ok[plain_flagged])
            fam = COVER.setdefault(sw.VARIANT_NAMES[v], dict(decided=0, flagged=0, centred=0, plain=0, nonfinite=0, classes=set(), models=set()))
            fam["decided"] += int((away & ~tl["flagged"]).sum())
            fam["flagged"] += int((away & tl["flagged"]).sum())
            fam["centred"] += int((ok & tl["centred"]).sum())
            fam["plain"] += int((ok & ~tl["centred"]).sum())
            fam["nonfinite"] += int((~ok).sum())
            fam["classes"].add(rname)
            fam["models"].add(model)


LR_CASES = (("random", sw.PLAIN, "natural"), ("surrogate", sw.PLAIN, "natural"), ("random", sw.CR_EXP, "natural"),
            ("surrogate", sw.CR_EXP, "scale8"), ("random", sw.CR_EXP, "pits"), ("surrogate", sw.PLAIN, "pits"), ("clustered", sw.CR_POLY, "natural"), ("clustered0", sw.CR_POLY, "natural"), ("clustered0", sw.CR_POLY, "pits"))
LR_GRID = 128


def _count(fam, tl, ok):
    with np.errstate(invalid="ignore", divide="ignore"):
        away = ok & ~(np.abs(np.abs(tl["val"]) - tl["err"]) <= sw.TAU0 * tl["err"] + tl["T"])
    c = COVER.setdefault(fam, dict(decided=0, flagged=0))
    c["decided"] += int((away & ~tl["flagged"]).sum())
    c["flagged"] += int((away & tl["flagged"]).sum())


@pytest.mark.parametrize("model", ("random", "clustered", "surrogate"))
def test_low_rank_tables_decode(model):
    """svt_lr and lr_btiles of the device-free build at the 128-grid: the projection B^ has orthonormal columns up to its fp16 rounding
    (and 192 - rank - pass-through zero columns); the projected SV images carry t = 0 and the centred form's b_n bit for bit in the same
    columns, zeros in the padding; and q~^_n is the least-squares coordinate vector of the centred SV q_n of the MODEL FILE in the columns
    of B^: |q~^_n - (B^'B^)^-1 B^'q_n| <= (3 x 2^-11 + 2^-11) |q_n| -- the build solves with the fp64 basis B, which B^ is the fp16 rounding
    of (2^-11 per entry: the Gram matrix and the right-hand side move by at most that each, the solution by the sum to first order, a third
    share for the second order), and rounds the result to fp16."""
    orc, tb = sw.oracle(model), sw.sweep_tables(model, LR_GRID)
    assert tb["svt_lr"] is not None and tb["lr_btiles"] is not None
    nt, neg = tb["n_sv_tiles"], tb["sv_tile_neg"]
    W, t, cf, pad = sw.decode_tiles(tb["svt_lr"], nt, lr=True)
    _, _, cfc, _ = sw.decode_tiles(tb["svt0_cr"], nt)
    assert (t == 0).all() and (cf.view(np.uint32) == cfc.view(np.uint32)).all() and (pad.view(np.uint32) == 0).all()
    tab = sw.slot_table(model, LR_GRID, "screen_cr")
    _, _, _, nt2, neg2, ex = sw.model_tiles(orc, tab, True)
    assert (nt2, neg2) == (nt, neg)
    live = np.zeros(nt * sw.SV_TILE, bool)
    live[ex["col"]] = True
    assert (W[~live].view(np.uint16) == 0).all()
    B = sw.decode_projection(tb["lr_btiles"]).astype(np.float64)
    used = np.abs(B).sum(axis=0) > 0
    Gm = B[:, used].T @ B[:, used]
    assert np.abs(Gm - np.eye(used.sum())).max() <= 320 * 2.0 ** -11 * 2.0 ** -4, "B^'B^ = I up to the fp16 rounding of B"
    assert (W[:, ~used].view(np.uint16) == 0).all(), "no projected SV has a component in an unused column"
    Q = ex["W"]
    sol = np.linalg.solve(Gm, B[:, used].T @ Q.T).T
    d = np.linalg.norm(W[ex["col"]][:, used].astype(np.float64) - sol, axis=1)
    assert (d <= 4 * 2.0 ** -11 * np.linalg.norm(Q, axis=1) + 1e-12).all(), float((d / np.linalg.norm(Q, axis=1)).max())


@pytest.mark.parametrize("model,variant,heights", LR_CASES, ids=lambda x: sw.VARIANT_NAMES[x] if isinstance(x, int) else x)
def test_low_rank_band_is_sound(model, variant, heights):
    _evaluate_lr(model, variant, heights)


def _evaluate_lr(model, variant, heights):
    """The low-rank form from the oracle alone, on the sampled evaluations of the `lowrank` request (three whole rows per roll and 300
    seeded ones): operands and raw sums of screen_operand_cases.reference, nu2 = its noise sum + (lr_rho M)^2 with M the roll's sum of
    |height|, y = B^'p^ in fp64, y^ = RN_fp16(y), sdy2 = |y^ - y|^2, the band of lr_finish_band on the host, the sums over the decoded
    svt_lr.  |val_ref - dec_oracle| + T_arith <= err_ref on every one of them; then the gather form on what the plain epilogue flags."""
    if ("lr", model, variant, heights) in _DONE:
        return
    _DONE.add(("lr", model, variant, heights))
    G = LR_GRID
    req = sw.request("lowrank", heights)
    want, tb = sw.oracle_want(model, req), sw.sweep_tables(model, G)
    cells = _cells(want)
    idx = np.arange(len(cells)) if model in FULL else sc.sample(cells, G, G, n_random=300)      # (`clustered0` runs whole: its polynomial band leaves few undecided)
    br, rem = np.divmod(cells[idx], G * G)
    dec = want["dec"][br, rem // G, rem % G]
    tab = sw.slot_table(model, G, "screen_cr" if variant >= sw.CR_EXP else "screen_lrp")
    ref = sc.reference(sw.OperandCase(model, req), tab, want["integral"], cells, idx, exact=True)
    S = ref["sums"]
    M = np.abs(want["heights"].astype(np.float64)).reshape(req.rolls, -1).sum(axis=1)[br]
    B = sw.decode_projection(tb["lr_btiles"]).astype(np.float64)
    y = ref["uh"].astype(np.float64) @ B
    yh = y.astype(np.float16)
    raw = np.zeros((len(idx), 8))
    raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 6] = S["su2"][0], S["sd2"][0], S["sx2"][0], S["cr"][0], S["ub"][0]
    raw[:, 4] = ref["noise"] + (tab["lr_rho"] * M) ** 2
    raw[:, 5] = ((yh.astype(np.float64) - y) ** 2).sum(axis=1)
    nax = (-0.5 * S["sx2"][0]).astype(np.float32)
    W, t, cf, _ = sw.decode_tiles(tb["svt_lr"], tb["n_sv_tiles"], lr=True)
    ts = sw.tile_sums(yh, W, t, cf, variant, tb["acc6"], degree=4)
    cs = sw.class_sums(ts, tb["sv_tile_neg"])

    def sound(tl, fam, sel):
        ok = np.isfinite(tl["err"]) & np.isfinite(tl["val"]) & np.isfinite(dec[sel])
        with np.errstate(invalid="ignore"):
            hole = ok & ~(np.abs(tl["val"] - dec[sel]) + tl["T"] <= tl["err"])
        assert not hole.any(), (fam, int(hole.sum()), float(np.abs(tl["val"] - dec[sel])[hole][0]), float(tl["T"][hole][0]), float(tl["err"][hole][0]))
        _count(fam, tl, ok)

    tl = sw.tail(cs, sw.lr_finish_band(model, G, raw, variant), nax, tb, variant, False)
    sound(tl, "LR_" + sw.VARIANT_NAMES[variant], slice(None))
    if variant == sw.PLAIN:                                         # the gather form: CR_EXP on what the plain epilogue leaves, L from raw[6]
        sel = np.flatnonzero(tl["flagged"])
        rw = raw[sel].copy()
        rw[:, 3] = rw[:, 6]
        cg = sw.class_sums(sw.tile_sums(yh[sel], W, t, cf, sw.CR_EXP, tb["acc6"], degree=4), tb["sv_tile_neg"])
        sound(sw.tail(cg, sw.lr_finish_band(model, G, rw, sw.CR_EXP), nax[sel], tb, sw.CR_EXP, False), "GATHER", sel)


def test_coverage_from_the_reference_alone():
    for case in _cases():                       # (counted once per process: the parametrised test above has usually been here)
        _evaluate(*case)
    for name in sw.VARIANT_NAMES:
        fam = COVER[name]
        assert fam["decided"] >= 20 and fam["flagged"] >= 20, (name, fam)
        assert fam["classes"] >= set(sw.CLASSES) | {"hostile"} and fam["models"] >= set(sw.MODELS), (name, fam)
    for case in LR_CASES:
        _evaluate_lr(*case)
    for name in ("PART", "LIST", "LR_PLAIN", "LR_CR_EXP", "LR_CR_POLY", "GATHER"):
        assert COVER[name]["decided"] >= 20 and COVER[name]["flagged"] >= 20, (name, COVER[name])
    assert COVER["PLAIN"]["centred"] > 0 and COVER["PLAIN"]["plain"] > 0, COVER["PLAIN"]
    assert COVER["PLAIN"]["nonfinite"] > 0, "block1e6: a non-finite band"


def test_sweep_table_export_under_address_and_ub_sanitizers(tmp_path):
    """The table builder on the models with one tile per class, a last tile with one live column and 8 / 9 tiles, under
    -fsanitize=address,undefined: tests/sanitize/table_paths.cpp (a program of its own, no device) in its `sweep` mode walks the SV
    tile images the way they are handed out and decoded here.  Any report fails."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    assert clang is not None, "no host C++ compiler"
    csrc = os.path.join(root, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "table_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
             "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")]
    subprocess.run([clang] + flags + [os.path.join(csrc, "model_tables.cpp"), os.path.join(csrc, "parsers.cpp"),
                                      os.path.join(root, "tests", "sanitize", "table_paths.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    names = ("m1+1", "m33+31", "m256+288")
    manifest = tmp_path / "manifest"
    manifest.write_text("".join("%s %s %s 0 %d 0\n" % (sc.FEATURES, sc.RANGE, sw.model_path(m), sw.GRID) for m in names))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(manifest), "sweep"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "table sanitizer job ok (3 cases)" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    for m, line in zip(names, [ln for ln in p.stdout.splitlines() if "sweep tables" in ln]):
        assert line.strip() == "sweep tables: %d tiles, first negative %d" % (sum(sw.TILES[m]), sw.TILES[m][0]), (m, line)
