"""What the screening SWEEP computes (ten-step and low-rank), against a definition, per evaluation, on the MI355X (tests/sweep_cases.py).

Every other test of the sweep looks at it through the guard band and the exact tiers behind it: a sweep that loses a tile, takes a
coefficient from the wrong column block or folds its sums wrongly only makes requests slower, a band term that came out too small is a
label error on inputs nobody ran, one that came out too wide costs undecided evaluations inside loose count limits.  Here the snapshot
of what every sweep launch of a request left (Engine.fetch_sweep: dec, margin, flag words, output list, counters, the partial sums of
the PART form, tier 0b's list-indexed input) is compared with the fp64 definition evaluated on the sweep's ACTUAL input -- the
snapshot's operand images, bands and a_x -- for every live evaluation:

  decision value   |dec_device - val_ref| <= T_arith (sweep_cases: what the kernel's own arithmetic may differ by); NaN where the
                   reference is NaN.  PART form: each slice's two class sums (and sum of squares) against the reference's sums over
                   that slice's tiles, within the slice's share of T_arith -- a slice boundary off by a tile shows here even where the
                   combined value hides it.
  band             decided evaluations: err_device = |dec_device| / margin_device against err_ref, TWO-SIDED, within
                   tau = TAIL_ROUNDINGS 2^-24 + T_arith / err_ref.
  decision rule    flagged => |val_ref| <= err_ref (1 + tau) + T_arith and margin == 0; decided => |val_ref| >= err_ref (1 - tau) - T_arith
                   and margin > 1.
  words, list      the flag words' bits are the evaluations with margin == 0, none at or beyond the live count; the output list is the
                   ascending flagged evaluation ids (list mode: evaluation ids, not slots), cut at flag0_cap; the counter holds the
                   uncapped total.
  labels           every live evaluation of a launch carries gv0 / gv1 by the sign of the device's value, right behind the launch.
  list mode        an evaluation that is not on the input list keeps the first pass's dec and margin bits.

Which kernel ran is asserted through Engine.sweep_form: k_svm_screen<0..3, false>, <0..3, true> + k_screen_combine at HAF_SCREEN_PARTS
2, 16 and by the engine's own rule (m1200), list mode with and without PART (tier 0b), the one-workgroup compaction and, on a 27-roll request
of 264 workgroups, k_screen_count + k_screen_compact.  Then compare_full on the same engine: the labels are still the oracle's.
The low-rank sweep has a test of its own at the end of the file: k_project and k_svm_screen_lr<PLAIN | CR_EXP | CR_POLY> in two launches
against the definition, the fused form against the two launches bit for bit, the gather form.  sweep_stats.json: per case the worst and the median of |dec - val_ref| / T_arith and of
err_device / err_ref, and the flagged share."""
import ctypes as C

import numpy as np
import pytest

import screen_operand_cases as sc
import sweep_cases as sw
from haf_grasping_amd import capi
from test_engine_gpu import compare_full, dump_stats, make_engine

pytestmark = pytest.mark.gpu

STATS = {}
CNT_EVALS, CNT_FLAGGED0, CNT_FLAGGED0B = 0, 4, 7


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module", autouse=True)
def _dump_stats():
    yield
    dump_stats(STATS, "sweep_stats.json")


class Case:
    def __init__(self, model, variant, parts=None, t0b=False, requests=("n1..31", "n257..511"), heights="natural", flag0_cap=None):
        self.model, self.variant, self.parts, self.t0b, self.requests, self.heights, self.flag0_cap = model, variant, parts, t0b, requests, heights, flag0_cap
        self.id = "-".join([model, sw.VARIANT_NAMES[variant], "parts%s" % (parts or "rule")] + (["t0b"] if t0b else []) +
                           ([heights] if heights != "natural" else []) + (["cap%d" % flag0_cap] if flag0_cap else []) + list(requests if len(requests) == 1 else []))

    def environment(self):
        e = dict(HAF_NO_DIRECT="1", HAF_SCREEN_VARIANT=str(self.variant), HAF_T1_SKIP="0", HAF_T0B="1" if self.t0b else "0")
        if not self.t0b:
            e["HAF_NO_CALIBRATE"] = "1"             # (HAF_T0B is read by the calibration: the list-mode cases let it run)
        if self.parts:
            e["HAF_SCREEN_PARTS"] = str(self.parts)
        if self.flag0_cap:
            e["HAF_FLAG0_CAP"] = str(self.flag0_cap)
        return e


def cases():
    out = []
    for v in range(4):
        for m in ("m1+1", "m33+31"):                    # (one tile per class: every forced split is K = 1, still the PART kernels)
            out += [Case(m, v), Case(m, v, parts=16)]
        out += [Case("m256+288", v), Case("m256+288", v, parts=2), Case("m256+288", v, parts=16)]
    for m in ("m1+1", "m33+31", "m256+288"):            # list mode: tier 0b behind the plain form, with and without PART
        out += [Case(m, sw.PLAIN, parts=1, t0b=True), Case(m, sw.PLAIN, parts=2, t0b=True)]
    for parts in (1, 2):                                # ... and on a list of thousands: the surrogate leaves the plain form 85 % of the request
        out.append(Case("surrogate", sw.PLAIN, parts=parts, t0b=True, requests=("hostile",)))
    for m in ("m32+32", "m1+95", "m224+544", "m1200", "sparse"):
        out.append(Case(m, sw.PLAIN, requests=("n257..511",)))
    out.append(Case("surrogate", sw.PLAIN, requests=("hostile",)))
    out.append(Case("clustered", sw.CR_EXP, requests=("hostile",)))
    out.append(Case("clustered0", sw.CR_POLY, requests=("hostile",)))
    out.append(Case("clustered_z", sw.CR_POLY, parts=2, requests=("n257..511",)))
    out.append(Case("surrogate", sw.CR_EXP, requests=("hostile",), heights="scale8"))
    out.append(Case("m33+31", sw.PLAIN, requests=("hostile",), heights="block1e6"))
    out.append(Case("m33+31", sw.PLAIN, requests=("rolls27",)))       # 264 workgroups: the two-launch compaction
    out.append(Case("surrogate", sw.PLAIN, requests=("hostile",), heights="pits", flag0_cap=256))
    return out


def _engine_acc_rel(eng):
    meas, used = (C.c_double * 2)(), (C.c_double * 2)()
    assert eng._L.haf_test_mfma_kappa(eng._h, meas, used) == 0
    return 10.0 * used[0] * sw.U24


def _check_launch(eng, slot, case, variant, U, band, nax, ids, n, tb, acc_rel, forced_parts, st, first=None, cells=None, lr=None):
    """One sweep launch against the reference.  U / band / nax: its input by SLOT (the first n are live), ids [n]: the evaluation each
    slot holds.  first: (dec, margin) of the first pass for a list launch.  cells: the request's evaluation list (cell ids), for the
    labels.  lr: dict(fused, gather) for a launch of the low-rank sweep (U: the projected operands, band: lr_finish_band's).
    -> the ascending flagged evaluation ids."""
    form = eng.sweep_form(slot)
    centred = variant >= sw.CR_EXP
    nt, neg = tb["n_sv_tiles"], tb["sv_tile_neg"]
    blocks = form["blocks"]
    want_part = lr is None and sw.splits(forced_parts, blocks, nt)
    two_launch = blocks * 4 > tb["compact_words"]                        # (the launcher's rule, from the code's constant)
    assert (form["variant"], form["lr"], form["part"], form["compaction"]) == (variant, lr is not None, want_part, int(two_launch)), form
    if lr is None:
        assert form["list"] == (first is not None) and not form["fused"] and not form["gather"], form
        W, t, cf, _ = sw.decode_tiles(tb["svt0_cr" if centred else "svt0"], nt)
        ts = sw.tile_sums(U[:n], W, t, cf, variant, acc_rel)
    else:
        assert (form["fused"], form["gather"], form["list"]) == (lr["fused"], lr["gather"], False), form
        W, t, cf, _ = sw.decode_tiles(tb["svt_lr"], nt, lr=True)
        ts = sw.tile_sums(U[:n], W, t, cf, variant, acc_rel, degree=4)
    st["compaction"] = "two launches" if two_launch else "one workgroup"
    tl = sw.tail(sw.class_sums(ts, neg), band[:n], nax[:n], tb, variant, combined=want_part)
    dec, margin = eng.fetch_sweep("dec", slot), eng.fetch_sweep("margin", slot)
    assert len(margin) == len(dec) and len(dec) >= (ids.max() + 1 if n else 0)
    d, mg = dec[ids].astype(np.float64), margin[ids].astype(np.float64)
    val, err, T = tl["val"], tl["err"], tl["T"]
    # ---- decision value ----
    nanr = np.isnan(val)
    assert (np.isnan(d) == nanr).all(), ("NaN where the reference is NaN, and only there", int(np.isnan(d).sum()), int(nanr.sum()))
    fin = ~nanr & np.isfinite(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        use = np.where(fin & (T > 0), np.abs(d - val) / T, 0.0)
    bad = fin & ~(np.abs(d - val) <= T)
    assert not bad.any(), ("decision value", int(bad.sum()), "first: slot %d evaluation %d device %r reference %r T_arith %r" %
                           (np.flatnonzero(bad)[0], ids[bad][0], d[bad][0], val[bad][0], T[bad][0]))
    # ---- PART: every slice's sums ----
    if want_part:
        K = sw.screen_parts(n, nt, neg, forced_parts if forced_parts > 1 else 0)
        part = eng.fetch_sweep("part", slot).reshape(-1, 4)
        stride = blocks * sw.BLOCK_EVALS
        assert len(part) >= K * stride
        Pd, Nd, Qd = np.zeros(n), np.zeros(n), np.zeros(n)
        for k in range(K):
            Pd, Nd, Qd = (a + part[k * stride:k * stride + n, i].astype(np.float64) for i, a in enumerate((Pd, Nd, Qd)))
            ck = sw.class_sums(ts, neg, sw.part_tiles(k, K, nt, neg))
            tol = sw.part_tolerance(ck, tb, variant)
            got = part[k * stride:k * stride + n].astype(np.float64)
            ok = np.isfinite(ck["P"]) & np.isfinite(ck["N"]) & np.isfinite(tol)
            for name, g, w in (("P", got[:, 0], ck["P"]), ("N", got[:, 1], ck["N"])):
                b = ok & ~(np.abs(g - w) <= tol)
                assert not b.any(), ("slice %d of %d, sum %s" % (k, K, name), int(b.sum()), float(g[b][0]), float(w[b][0]), float(tol[b][0]))
            if variant == sw.SUMSQ:
                # (d sum t^2 = sum 2 t dt <= 2 max|t| sum|dt|; the squares' own single-level fp32 sum: guard_acc0_s of it)
                b = ok & ~(np.abs(got[:, 2] - ck["sq"]) <= 2.0 * tol * (ck["magP"] + ck["magN"]) + 1.04 * tb["guard_acc0_s"] * ck["sq"])
                assert not b.any(), ("slice %d of %d, sum of squares" % (k, K), int(b.sum()))
            else:
                assert (got[:, 2] == 0).all()
        st["parts"] = K
        # ... and k_screen_combine's tail on the DEVICE's own partial sums: what it made of them is then a matter of fp32 roundings
        # alone, so the band is held two-sided within TAU0 -- no share of T_arith, which in `tau` below hides a band term of its own size
        # (guard_acc0, the COMBINED unit) -- and the value within the roundings of P sc, N sc, their sum and - rho
        own = sw.tail(dict(P=Pd, N=Nd, magP=np.abs(Pd), magN=np.abs(Nd), sq=Qd, acc=0.0, unit=0.0), band[:n], nax[:n], tb, variant, combined=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            okv = np.isfinite(own["val"])
            assert (np.abs(d - own["val"])[okv] <= (6.0e-7 * (np.abs(own["val"]) + abs(tb["rho"])) + 4 * sw.U24 * own["S"] + tb["guard_abs"])[okv]).all(), "the combined value"
            dcd = (mg > 0) & okv & np.isfinite(own["err"])
            r_own = (np.abs(d) / mg)[dcd] / own["err"][dcd]
            # (6e-7: the reference takes sc = 2^a_x in fp64, the kernel by v_exp_f32 -- an ulp, 1.2e-7 -- and sc enters err through
            # P sc and N sc in sabs and through abs_c sc; D charges the same three operations 6e-7: BANDS.md, row `D`)
            off = ~(np.abs(r_own - 1.0) <= sw.TAU0 + 6.0e-7)
            assert not off.any(), ("band of the combined sums", int(off.sum()), float(r_own[off][0]))
            if dcd.any():
                st.update(own_err_ratio_min=float(r_own.min()), own_err_ratio_max=float(r_own.max()))
    # ---- band, two-sided, and the decision rule ----
    flagged = mg == 0
    decided = ~flagged
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = sw.TAU0 + T / err
        assert (mg[decided] > 1.0).all(), "a decided evaluation lies outside its band"
        errd = np.abs(d) / mg
        ratio = errd[decided] / err[decided]
        off = ~(np.abs(ratio - 1.0) <= tau[decided])
        assert not off.any(), ("band", int(off.sum()), "err_device / err_ref = %r, tau %r" % (float(ratio[off][0]), float(tau[decided][off][0])))
        assert (np.abs(val[decided]) >= err[decided] * (1.0 - tau[decided]) - T[decided]).all(), "decided inside the reference's band"
        fl = flagged & fin & np.isfinite(err)
        assert (np.abs(val[fl]) <= err[fl] * (1.0 + tau[fl]) + T[fl]).all(), "flagged outside the reference's band"
    assert flagged[nanr | ~np.isfinite(err)].all(), "a NaN value or a non-finite band is never trusted"
    # ---- labels: every live evaluation of the launch carries gv0 / gv1 by the sign of the device's value (NaN: gv1) ----
    if cells is not None:
        lab = eng.fetch_sweep("labels", slot)
        with np.errstate(invalid="ignore"):
            want_lab = np.where(d > 0, tb["gv0"], tb["gv1"])
        assert (lab[cells[ids]] == want_lab).all(), ("labels behind the launch", int((lab[cells[ids]] != want_lab).sum()))
    # ---- flag words, list, counters ----
    words = eng.fetch_sweep("words", slot)
    assert len(words) >= blocks * 4
    live_blocks = (n + sw.BLOCK_EVALS - 1) // sw.BLOCK_EVALS            # (workgroups beyond the live count leave at once: their words are nobody's)
    bits = sw.flag_bits(words, live_blocks * sw.BLOCK_EVALS)
    assert (bits[:n] == flagged).all(), "flag words against margin == 0"
    assert not bits[n:].any(), "no bits at or beyond the live count in the last block"
    want_list = ids[flagged]
    assert (np.diff(want_list) > 0).all()
    counters = eng.fetch_sweep("counters", slot)
    out_cnt = int(counters[CNT_FLAGGED0B if first is not None else CNT_FLAGGED0])
    assert int(counters[CNT_EVALS]) == (n if first is None else int(counters[CNT_EVALS]))
    assert out_cnt == len(want_list), ("the counter holds the uncapped total", out_cnt, len(want_list))
    lst = eng.fetch_sweep("list", slot)
    kept = min(len(want_list), len(lst))
    assert (lst[:kept] == want_list[:kept]).all(), "the output list is the ascending flagged evaluation ids"
    # ---- list mode writes nothing else ----
    if first is not None:
        assert len(dec) == len(first[0]) and len(margin) == len(first[1])
        other = np.ones(len(dec), bool)
        other[ids] = False
        same = lambda a, b: (a[other].view(np.uint32) == b[other].view(np.uint32)).all()
        assert same(dec, first[0]) and same(margin, first[1]), "an evaluation that is not on the input list keeps the first pass's dec and margin"
    with np.errstate(invalid="ignore"):
        st.update(n=int(n), flagged_share=float(flagged.mean()) if n else 0.0, worst_dec_over_T=float(use.max()) if n else 0.0,
                  median_dec_over_T=float(np.median(use)) if n else 0.0, kernel="k_svm_screen<%s, %s>%s" % (sw.VARIANT_NAMES[variant], "true" if want_part else "false", " list" if first is not None else ""))
        if decided.any():
            st.update(err_ratio_min=float(ratio.min()), err_ratio_median=float(np.median(ratio)), err_ratio_max=float(ratio.max()))
    return want_list, (dec, margin)


@pytest.mark.parametrize("case", cases(), ids=lambda c: c.id)
def test_sweep_against_the_reference(data_dir, monkeypatch, case):
    for k, v in case.environment().items():
        monkeypatch.setenv(k, v)
    if not case.parts:
        monkeypatch.delenv("HAF_SCREEN_PARTS", raising=False)
    reqs = [sw.request(r, case.heights) for r in case.requests]
    G = reqs[0].grid
    tb = sw.sweep_tables(case.model, G)
    eng = make_engine(data_dir, sw.model_path(case.model), 0, testing=True, **reqs[0].cfg_kw())
    try:
        eng.snapshot_screen(True)
        acc_rel = _engine_acc_rel(eng)
        for req in reqs:
            st = STATS.setdefault(case.id + "/" + req.name, {})
            xyz = req.cloud()
            eng.score(xyz, capi.default_input(**req.in_kw()))
            n = eng.last_counts()["n_evals"]
            assert n > 0 and eng.screen_low_rank()["last_used"] is False
            X = eng.fetch_snapshot(0)
            gb = eng.fetch_snapshot(1).view(np.float32).reshape(-1, sc.BAND_FLOATS)
            ax = eng.fetch_snapshot(2).view(np.float32)
            U = sc.image_rows(X, np.arange(n)).view(np.float16)
            forced = int(case.parts) if case.parts else 0
            cells = eng.fetch_list(0)
            assert len(cells) == n
            flagged0, first = _check_launch(eng, 0, case, case.variant, U, gb, ax, np.arange(n), n, tb, acc_rel, forced, st.setdefault("pass0", {}), cells=cells)
            assert (st["pass0"]["compaction"] == "two launches") == (req.name == "rolls27"), "k_screen_count + k_screen_compact on the 27-roll request only"
            cap = len(eng.fetch_sweep("list", 0))
            if case.flag0_cap:
                assert cap == case.flag0_cap and len(flagged0) > cap, "the list is cut at flag0_cap (and the guard zones behind it are intact: _canaries)"
            if case.t0b:
                assert len(flagged0) <= cap
                f1 = eng.sweep_form(1)
                assert f1["variant"] == sw.CR_EXP and f1["list"] and not f1["lr"], f1
                n1 = len(flagged0)
                U1 = sc.image_rows(eng.fetch_sweep("in_X", 1), np.arange(n1)).view(np.float16) if n1 else np.zeros((0, sc.K), np.float16)
                gb1 = eng.fetch_sweep("in_gband", 1).reshape(-1, sc.BAND_FLOATS)
                ax1 = eng.fetch_sweep("in_ax", 1)
                _check_launch(eng, 1, case, sw.CR_EXP, U1, gb1, ax1, flagged0, n1, tb, acc_rel, forced, st.setdefault("tier0b", {}), first=first, cells=cells)
            else:
                assert eng.sweep_form(1)["variant"] == -1
            if not case.flag0_cap:
                compare_full(eng, sw.oracle(case.model), xyz, req.cfg_kw(), req.in_kw(), check_dec=False, want=sw.oracle_want(case.model, req))
    finally:
        eng.close()


# ---- the low-rank sweep ------------------------------------------------------------------------------------------------------------
# screen_operand_cases' `lowrank` request (128-grid, 2 rolls, HAF_LARGE_EVALS = 1) against its two models.  In two launches
# (HAF_LR_UNFUSED) k_project leaves the projected images Y and raw[5] in memory: the projection is held to the fp64 product of the decoded
# projection tiles with the snapshot's ten-step images, the sweep k_svm_screen_lr<., false, false> to the definition on Y exactly as the
# ten-step sweep above, with lr_finish_band / lr_finish_band_plain evaluated on the host on the raw sums the sweep read.  The fused form
# keeps Y in registers: it must give the two-launch form's dec and margin bit for bit.  The gather form (tier 0b behind the fused plain
# pass) is held to the CR_EXP epilogue on the two-launch run's Y rows of the listed evaluations, with L from raw[6].
LR_ENV = dict(HAF_LARGE_EVALS="1", HAF_NO_DIRECT="1", HAF_T1_SKIP="0")
KF32ACC = sc.KF32ACC


def _lr_engine(data_dir, monkeypatch, model, variant, unfused, req, t0b=False):
    for k in ("HAF_LR_UNFUSED", "HAF_NO_CALIBRATE", "HAF_SCREEN_PARTS", "HAF_T0B_NO_GATHER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(LR_ENV, HAF_SCREEN_VARIANT=str(variant), HAF_T0B="1" if t0b else "0").items():
        monkeypatch.setenv(k, v)
    if unfused:
        monkeypatch.setenv("HAF_LR_UNFUSED", "1")
    if not t0b:
        monkeypatch.setenv("HAF_NO_CALIBRATE", "1")
    eng = make_engine(data_dir, sw.model_path(model), 0, testing=True, **req.cfg_kw())
    eng.snapshot_screen(True)
    return eng


def _lr_score(eng, req):
    eng.score(req.cloud(), capi.default_input(**req.in_kw()))
    assert eng.screen_low_rank()["last_used"] is True
    n = eng.last_counts()["n_evals"]
    assert n > 0
    return n


def _lr_two_launches(eng, req, model, variant, tb, st):
    """k_project + k_svm_screen_lr<variant, false, false> of one request against the definition -> what the other forms are held to."""
    G = req.grid
    kappa_scale = _engine_acc_rel(eng) / (10.0 * sc.KAPPA * sw.U24)      # (the engine's measured kappa over the table build's 12)
    acc6, acc10 = tb["acc6"] * kappa_scale, tb["acc10"] * kappa_scale
    n = _lr_score(eng, req)
    cells = eng.fetch_list(0)
    X = sc.image_rows(eng.fetch_snapshot(0), np.arange(n)).view(np.float16)
    ax = eng.fetch_snapshot(2).view(np.float32)
    raw = eng.fetch_sweep("raw", 0).reshape(-1, sc.BAND_FLOATS)
    Y = sw.lr_rows(eng.fetch_sweep("Y", 0), np.arange(n))
    # ---- the projection: every component of Y within acc10 sum |B^||p^| of the fp64 product, before its cast ----
    B = sw.decode_projection(tb["lr_btiles"]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        P64 = X.astype(np.float64)
        y, tol = P64 @ B, acc10 * (np.abs(P64) @ np.abs(B))
        lo, hi = (y - tol).astype(np.float16).astype(np.float64), (y + tol).astype(np.float16).astype(np.float64)
        Yd = Y.astype(np.float64)
        fin = np.isfinite(y) & np.isfinite(tol)
        inside = (Yd >= lo) & (Yd <= hi)
        assert inside[fin].all(), ("projection: the stored fp16 is not the image of a value within acc10 sum|B^||p^| of the fp64 product", int((~inside[fin]).sum()))
        assert not np.isfinite(Yd[~fin & np.isnan(y)]).any()
        # raw[5] = sum (y^ - y32)^2 for some y32 in that interval, summed in fp32
        dist = np.abs(Yd - y)
        s_lo, s_hi = (np.maximum(0.0, dist - tol) ** 2).sum(axis=1), ((dist + tol) ** 2).sum(axis=1)
        rowfin = fin.all(axis=1)
        sdy = raw[:n, 5].astype(np.float64)
        assert ((sdy >= s_lo * (1.0 - KF32ACC)) & (sdy <= s_hi * (1.0 + KF32ACC)))[rowfin].all(), "raw[5] outside what the projection's interval allows"
    # ---- the sweep on Y ----
    band = sw.lr_finish_band(model, G, raw[:n], variant)
    flagged, first = _check_launch(eng, 0, None, variant, Y, band, ax, np.arange(n), n, tb, acc6, 0, st.setdefault("two launches", {}),
                                   cells=cells, lr=dict(fused=False, gather=False))
    compare_full(eng, sw.oracle(model), req.cloud(), req.cfg_kw(), req.in_kw(), check_dec=False, want=sw.oracle_want(model, req))
    return dict(n=n, cells=cells, raw=raw, Y=Y, ax=ax, flagged=flagged, first=first, acc6=acc6)


def _lr_fused(eng, req, variant, res):
    """k_svm_screen_lr<variant, true, false>: the two-launch form's dec, margin, list and counter, bit for bit."""
    assert _lr_score(eng, req) == res["n"]
    n, f = res["n"], eng.sweep_form(0)
    assert f["lr"] and f["fused"] and not f["gather"] and f["variant"] == variant, f
    for what, want in (("dec", res["first"][0]), ("margin", res["first"][1])):
        got = eng.fetch_sweep(what, 0)
        assert (got[:n].view(np.uint32) == want[:n].view(np.uint32)).all(), ("fused against two launches, bit for bit", what)
    lst = eng.fetch_sweep("list", 0)
    assert (lst[:len(res["flagged"])] == res["flagged"]).all() and int(eng.fetch_sweep("counters", 0)[CNT_FLAGGED0]) == len(res["flagged"])


def _lr_gather(eng, req, model, tb, res, st, min_list):
    """k_svm_screen_lr<CR_EXP, true, true>, tier 0b behind the fused plain pass: the CR_EXP epilogue on the listed rows of Y, L from raw[6]."""
    assert _lr_score(eng, req) == res["n"]
    raw, Y, ax, acc6, ids = res["raw"], res["Y"], res["ax"], res["acc6"], res["flagged"]
    n1, f1 = len(ids), eng.sweep_form(1)
    assert f1["lr"] and f1["fused"] and f1["gather"] and f1["variant"] == sw.CR_EXP, f1
    assert n1 >= min_list and (eng.fetch_sweep("list", 0)[:n1] == ids).all(), "the gather launch's input list is the first pass's"
    rw = raw[ids].copy()
    rw[:, 3] = raw[ids, 6]                                    # L rides in raw[6]; raw[3] is the plain form's correction sum
    band1 = sw.lr_finish_band(model, req.grid, rw, sw.CR_EXP)
    first_f = (eng.fetch_sweep("dec", 0), eng.fetch_sweep("margin", 0))
    _check_launch(eng, 1, None, sw.CR_EXP, Y[ids], band1, ax[ids], ids, n1, tb, acc6, 0, st.setdefault("gather", {}), first=first_f, cells=res["cells"],
                  lr=dict(fused=True, gather=True))
    if n1 < 20:
        return
    # ... and the assertion above sees raw[3] taken for L: on the reference the two differ by more than T_arith on most evaluations
    W, t, cf, _ = sw.decode_tiles(tb["svt_lr"], tb["n_sv_tiles"], lr=True)
    cs = sw.class_sums(sw.tile_sums(Y[ids], W, t, cf, sw.CR_EXP, acc6, degree=4), tb["sv_tile_neg"])
    right = sw.tail(cs, band1, ax[ids], tb, sw.CR_EXP, False)
    wrong = sw.tail(cs, sw.lr_finish_band(model, req.grid, raw[ids], sw.CR_EXP), ax[ids], tb, sw.CR_EXP, False)
    with np.errstate(invalid="ignore"):
        seen = np.abs(right["val"] - wrong["val"]) > right["T"]
    assert seen.mean() > 0.5, ("raw[3] for raw[6] would go unseen", float(seen.mean()))
    st["gather"]["raw3_for_raw6_seen_share"] = float(seen.mean())


SMALL = ("lr_n1..31", "lr_n257..511")


def _lr_params():
    # the `lowrank` request (5 4xx evaluations): the surrogate leaves the plain epilogue most of it, so the gather form serves a list of
    # thousands; `pits`: negative heights, the feature kernel's path B sums
    out = [("random", sw.PLAIN, "natural", ("lowrank",)), ("surrogate", sw.PLAIN, "natural", ("lowrank",)), ("random", sw.CR_EXP, "natural", ("lowrank",)),
           ("random", sw.CR_EXP, "pits", ("lowrank",)), ("clustered", sw.CR_POLY, "natural", ("lowrank",))]
    # the edges of the low-rank sweep's own loops -- its 3-deep ring at nt = 2, a sign group of one tile, a last tile with one live column,
    # the fold at 8 and 9 tiles -- at 25 and 399 evaluations of one roll (a last workgroup of 25 and of 143 live evaluations)
    out += [(m, v, "natural", SMALL) for m in ("m1+1", "m33+31", "m256+288") for v in (sw.PLAIN, sw.CR_EXP, sw.CR_POLY)]
    # the rest of the table: the low-rank plain form
    out += [(m, sw.PLAIN, "natural", SMALL[1:]) for m in ("m32+32", "m1+95", "m224+544", "m1200", "sparse")]
    return out


@pytest.mark.parametrize("model,variant,heights,rnames", _lr_params(),
                         ids=lambda x: sw.VARIANT_NAMES[x] if isinstance(x, int) else "small" if x == SMALL else x[0] if isinstance(x, tuple) else x)
def test_low_rank_sweep_against_the_reference(data_dir, monkeypatch, model, variant, heights, rnames):
    reqs = [sw.request(r, heights) for r in rnames]
    tb = sw.sweep_tables(model, reqs[0].grid)
    assert tb["svt_lr"] is not None and tb["lr_btiles"] is not None and tb["acc6"] > 0 and tb["acc10"] > 0
    stats = {r.name: STATS.setdefault("lowrank-%s-%s-%s/%s" % (model, sw.VARIANT_NAMES[variant], heights, r.name), {}) for r in reqs}
    res = {}
    eng = _lr_engine(data_dir, monkeypatch, model, variant, True, reqs[0])
    try:
        for r in reqs:
            res[r.name] = _lr_two_launches(eng, r, model, variant, tb, stats[r.name])
    finally:
        eng.close()
    eng = _lr_engine(data_dir, monkeypatch, model, variant, False, reqs[0])
    try:
        for r in reqs:
            _lr_fused(eng, r, variant, res[r.name])
    finally:
        eng.close()
    if variant != sw.PLAIN:
        return
    eng = _lr_engine(data_dir, monkeypatch, model, variant, False, reqs[0], t0b=True)
    try:
        for r in reqs:
            _lr_gather(eng, r, model, tb, res[r.name], stats[r.name], 1000 if model == "surrogate" else 0)
    finally:
        eng.close()
