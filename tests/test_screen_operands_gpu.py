"""What the screening feature kernels WRITE, against a host reference, slot by slot, on the MI355X (tests/screen_operand_cases.py).

Every label of the default mode rests on the operands, sums and a_x of the screening feature pass, and every other test of that pass
works behind the guard band, which is exactly what hides an operand that is slightly wrong or a sum that is slightly small.  Here the
snapshot of the pass (Engine.snapshot_screen) is compared with the definition, per evaluation, for the smallest requests that reach
each of the five kernels (asserted through haf_test_feature_form) and each route inside them -- the LDS band with screen_group, with
screen_pair3 (HAF_NO_FAST_GROUPS), per-lane loads, the wave-form kernels, the low-rank paths A, B and C:

  operand image   the 640 bytes of the evaluation equal the reference's RN_fp16(fmaf(fl32(decq4_scr(v)), scr_mul, scr_add)) bit for bit; NaN
                  stands where the reference has NaN, with any payload.  No other exception was needed on any route.
  sums            low-rank form: raw slots 0, 1, 2, 3, 6 = su2, sd2, sx2, cr, ub within kF32Acc x the sum of their terms' magnitudes
                  of the fp64 sums.  Other forms: the finished band holds `cr` still in the open -- band[4] = fl32(ln2 cr) in the plain forms,
                  band[0] = fl32(cr) in the centred-remainder form -- and that is held to the same bound (plus the cast's 2^-24).
  a_x             low-rank form: == -0.5f * raw[2] bit for bit; other forms: within kF32Acc |a_x| of -sx2 / 2.
  band            other forms: screen_finish (csrc/screen_finish.h, host and device) evaluated on the host on the reference's fp64 sums with the
                  engine's own constants (haf_test_screen_finish): band_device[i] >= band_host[i] (1 - 2 kF32Acc) for i = 0..3 and 5 in the
                  plain forms, i = 1..3 in the centred-remainder form (whose band[0] is L, the `cr` sum itself, and whose band[5] is 0); an
                  infinity on the host requires one on the device, and band[1] = +inf wherever the reference's sums are not finite or
                  a_x >= 30.
  nu2             low-rank form: nu2 (1 + kF32Acc) >= sum (u' - u_lin)^2 + (lr_rho M)^2 with M from the (cloud, roll)'s |height| total;
                  finite wherever every operand is finite and the smallest region sum is >= 0; +inf for an evaluation with a negative
                  region sum on a predicted path-A wave -- a rule NO case here reaches (it takes a grid without negative heights whose
                  fp32 corners leave a near-empty region at -1..-3 ulp; `pits` has no path A): only
                  test_engine_gpu.py::test_low_rank_pass_never_trusts_a_negative_computed_region_sum covers it.
                  How far above: screen_operand_stats.json (min, median, q99, max per path).
  padding rows    of the last block of 256: zero image, zero band, a_x = 0, raw slot 4 = +inf in the low-rank form.

Per case every evaluation of three whole grid rows per roll, 500 seeded ones and every padding row.  Then compare_full on the same
engine: the request's labels are still the oracle's.  Coverage is asserted from the reference alone (and proven without a GPU in
tests/test_screen_operands_cpu.py): both wave kinds on the 96-grid, paths B and C and no A under `pits`, A and C under `natural` on
the 128-grid, a NaN operand under block1e6, every group outside fast_groups.  Two low-rank cases run on a feature file whose rows are
all two-region HAF features (screen_operand_cases.two_region_features): every group is fast, so nu2 on path A is pair_math's charge
alone.  Which one-line mutation of the kernels each assertion catches, and the one it cannot see: DESIGN.md 3."""
import numpy as np
import pytest

import hostile_cases as hc
import screen_operand_cases as sc
from haf_grasping_amd import capi
from test_engine_gpu import compare_full, dump_stats, make_engine

pytestmark = pytest.mark.gpu

STATS = {}
LN2 = 0.69314718056                      # the constant screen_finish multiplies cr by
U24 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module", autouse=True)
def _dump_stats():
    yield
    dump_stats(STATS, "screen_operand_stats.json")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _within(dev, val, mag, extra_rel=0.0, what=""):
    """|dev - val| <= kF32Acc mag (+ extra_rel |val|) where the reference is finite; not finite where it is not."""
    dev = np.asarray(dev, np.float64)
    fin = np.isfinite(val) & np.isfinite(mag)
    assert not np.isfinite(dev[~fin]).any(), (what, "finite on the device where the reference's sum is not", int(np.isfinite(dev[~fin]).sum()))
    err = np.abs(dev[fin] - val[fin])
    bound = sc.KF32ACC * mag[fin] + extra_rel * np.abs(val[fin])
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), "worst |device - fp64| / bound = %.3g" % float((err[bad] / np.maximum(bound[bad], 1e-300)).max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        used = np.where(bound > 0, err / bound, 0.0)
    return float(used.max()) if len(used) else 0.0


def _snapshot(eng):
    X = eng.fetch_snapshot(0)
    gb = eng.fetch_snapshot(1).view(np.float32).reshape(-1, sc.BAND_FLOATS)
    ax = eng.fetch_snapshot(2).view(np.float32)
    return X, gb, ax


@pytest.mark.parametrize("case", sc.cases(), ids=lambda c: c.id)
def test_screening_feature_pass_against_the_reference(data_dir, monkeypatch, case):
    for k, v in case.environment().items():
        monkeypatch.setenv(k, v)
    cfg_kw, in_kw = case.cfg_kw(), case.in_kw()
    G = case.grid
    assert sc.predicted_kernel(G, case.lx, case.ly, case.rolls, 1 if "HAF_LARGE_EVALS" in case.env else sc.LARGE_EVALS, case.low_rank()) == case.kernel
    xyz = case.cloud()
    if case.two_region:
        eng = capi.Engine(case.feature_file(), sc.RANGE, hc.model_path(case.model), testing=True, flags=capi.FLAG_KEEP_DEBUG | capi.FLAG_PROFILE, **cfg_kw)
    else:
        eng = make_engine(data_dir, hc.model_path(case.model), 0, testing=True, **cfg_kw)
    try:
        eng.snapshot_screen(True)
        eng.score(xyz, capi.default_input(**in_kw))
        ran = eng.feature_form(per_roll=True)
        kernel, flags, iiabs = ran["kernel"], ran["flags"], ran["iiabs"]
        assert kernel == case.kernel, ("feature kernel", eng.FEATURE_FORMS[kernel], "expected", eng.FEATURE_FORMS[case.kernel])
        assert eng.screen_low_rank()["last_used"] == case.low_rank()
        form = eng.SCREEN_PARAMS[ran["params"]]                   # the ScreenParams set the pass was launched with (the engine may change its form behind a request)
        if case.variant is not None:
            assert form == sc.form_of(case), (form, sc.form_of(case))
        tab = sc.table_for(case, form)
        assert tab is not None, form
        cells = eng.fetch_list(0)
        n = len(cells)
        assert n == eng.last_counts()["n_evals"] and n > 0
        ii = np.stack([eng.debug(capi.DBG_INTEGRAL, 0, r) for r in range(case.rolls)])
        X, gb, ax = _snapshot(eng)
        n_pad = (n + sc.BLOCK_EVALS - 1) // sc.BLOCK_EVALS * sc.BLOCK_EVALS
        assert len(ax) >= n_pad and len(gb) >= n_pad and len(X) >= n_pad // sc.TILE_EVALS * sc.TILE_BYTES, "the snapshot holds the whole last block"

        idx = sc.sample(cells, G, G)
        lr = case.low_rank()
        ref = sc.reference(case, tab, ii, cells, idx, exact=lr)
        st = STATS.setdefault(case.id, {})
        st.update(kernel=eng.FEATURE_FORMS[kernel], form=form, n_evals=int(n), compared=int(len(idx)), fma_ties_settled_exactly=int(ref["hard"]))

        # ---- operand image ----
        want_h = ref["uh"].view(np.uint16)
        got_h = sc.image_rows(X, idx)
        nan_w, nan_g = np.isnan(ref["uh"]), np.isnan(got_h.view(np.float16))
        diff = (got_h != want_h) & ~(nan_w & nan_g)
        if diff.any():
            e, s = np.argwhere(diff)[0]
            raise AssertionError(("operand image", int(diff.sum()), "first: evaluation %d slot %d device 0x%04x reference 0x%04x u' %r v %r" %
                                  (idx[e], s, got_h[e, s], want_h[e, s], float(ref["u1"][e, s]), float(ref["V"][e, s]))))
        st["nan_operands"] = int(nan_w.sum())

        # ---- sums and a_x ----
        S = ref["sums"]
        band, a_x = gb[idx], ax[idx]
        sx2, _ = S["sx2"]
        if lr:
            for name, slot in (("su2", 0), ("sd2", 1), ("sx2", 2), ("cr", 3), ("ub", 6)):
                st["used_" + name] = _within(band[:, slot], S[name][0], S[name][1], what=name)
            want_ax = (np.float32(-0.5) * band[:, 2]).astype(np.float32)
            same = (_bits(a_x) == _bits(want_ax)) | (np.isnan(a_x) & np.isnan(want_ax))
            assert same.all(), ("a_x != -0.5f raw[2]", int((~same).sum()))
            assert (band[:, 5] == 0).all() and (band[:, 7] == 0).all()
        else:
            st["used_ax"] = _within(a_x, -0.5 * sx2, 0.5 * sx2, what="a_x")
            cr, cr_mag = S["cr"]
            if tab["cr"]:
                st["used_cr"] = _within(band[:, 0], cr, cr_mag, extra_rel=U24, what="cr (band[0])")
            else:
                on = np.isfinite(band[:, 5]) | (band[:, 4] != 0)          # (band[4] = 0, band[5] = inf: the centred estimate is switched off)
                if on.any():
                    st["used_cr"] = _within(band[on, 4], LN2 * cr[on], LN2 * cr_mag[on], extra_rel=2 * U24, what="cr (band[4])")
            fin = np.isfinite(sx2) & np.isfinite(S["su2"][0]) & np.isfinite(S["sd2"][0]) & np.isfinite(cr)
            never = ~fin | (0.5 * sx2 >= 30.0 * (1.0 + sc.KF32ACC))
            assert np.isposinf(band[never, 1]).all(), ("band[1] is finite where the reference's sums are not, or a_x >= 30", int((~np.isposinf(band[never, 1])).sum()))
            st["never_trusted"] = int(never.sum())
            # the band floats against screen_finish on the host, evaluated on the reference's fp64 sums with this engine's constants
            host_band, host_ax = eng.screen_finish(np.stack([S["su2"][0], S["sd2"][0], sx2, cr, S["ub"][0]], 1))
            same_ax = np.abs(a_x.astype(np.float64) - host_ax) <= sc.KF32ACC * np.abs(host_ax)
            assert (same_ax | (np.isnan(a_x) & np.isnan(host_ax))).all(), "a_x against screen_finish on the host"
            worst = {}
            for i in ((1, 2, 3) if tab["cr"] else (0, 1, 2, 3, 5)):                # (centred-remainder form: band[0] is L itself -- the `cr` sum above -- and band[5] is 0)
                h, d = host_band[:, i].astype(np.float64), band[:, i].astype(np.float64)
                assert np.isposinf(d[np.isposinf(h)]).all(), ("band[%d]: an infinity on the host, none on the device" % i)
                assert not np.isfinite(d[np.isnan(h)]).any(), ("band[%d]: finite on the device where the host's is NaN" % i)
                ok = np.isfinite(h)
                short = d[ok] < h[ok] * (1.0 - 2.0 * sc.KF32ACC)
                assert not short.any(), ("band[%d] below screen_finish of the fp64 sums" % i, int(short.sum()), float((d[ok][short] / h[ok][short]).min()))
                pos = ok & (h > 0) & np.isfinite(d)
                if pos.any():
                    worst[i] = float((d[pos] / h[pos]).min())
            st["band_device_over_host_min"] = worst

        # ---- low-rank form: the noise bound ----
        fast = sc.wave_kinds(cells)
        if lr:
            paths = sc.predict_paths(cells, ii, G, G, flags)
            wave_path = paths[idx // 64]
            M = iiabs[cells[idx] // (G * G)].astype(np.float64) * 2.0 ** -20
            for r in range(case.rolls):
                assert float(iiabs[r]) * 2.0 ** -20 >= float(np.abs(ii[r]).max()), "the |height| total bounds every corner"
            nu2 = band[:, 4].astype(np.float64)
            want_nu2 = ref["noise"] + (tab["lr_rho"] * M) ** 2
            fin = np.isfinite(want_nu2)
            assert not np.isfinite(nu2[~fin]).any(), "nu2 finite where a HAF operand is not"
            all_fin = ~np.isnan(ref["u1"]).any(axis=1)                 # (a NaN in a SHAF slot may poison nu2 as it poisons su2: never trusted either way)
            assert not np.isnan(nu2[all_fin]).any()
            low = nu2[fin] * (1.0 + sc.KF32ACC) < want_nu2[fin]
            assert not low.any(), ("nu2 below sum (u' - u_lin)^2 + (lr_rho M)^2", int(low.sum()), wave_path[fin][low][:8].tolist(),
                                   float((nu2[fin][low] / want_nu2[fin][low]).min()))
            neg = ref["rmin"] < 0
            must_be_finite = all_fin & ~neg
            assert np.isfinite(nu2[must_be_finite]).all(), ("nu2 not finite for %d evaluations without a negative region sum" % int((~np.isfinite(nu2[must_be_finite])).sum()))
            void = fin & neg & (wave_path == "A")
            assert np.isposinf(nu2[void]).all(), "a negative region sum on a path-A wave must void the evaluation"
            st["void_on_path_A"] = int(void.sum())                     # (0 in every case here: see the docstring)
            for p in "ABC":
                m = fin & (wave_path == p) & np.isfinite(nu2) & (want_nu2 > 0)
                st["waves_" + p] = int((paths == p).sum())
                if m.any():
                    q = nu2[m] / want_nu2[m]
                    st["nu2_ratio_" + p] = dict(n=int(m.sum()), min=float(q.min()), median=float(np.median(q)), q99=float(np.quantile(q, 0.99)), max=float(q.max()))

        # ---- padding rows of the last block ----
        if n_pad > n:
            pad = np.arange(n, n_pad)
            assert (sc.image_rows(X, pad) == 0).all(), "padding rows: operand image"
            zero = gb[pad].copy()
            if lr:
                assert np.isposinf(zero[:, 4]).all(), "padding rows: raw slot 4"
                zero[:, 4] = 0
            assert (_bits(zero) == 0).all() and (_bits(ax[pad]) == 0).all(), "padding rows: band and a_x"
        st["padding_rows"] = int(n_pad - n)

        # ---- coverage, from the reference alone ----
        if case.grid == 96 and case.row == "serial":
            assert fast.any() and not fast.all(), "96-grid: both wave kinds"
        if case.heights == "holes":
            wg = np.add.reduceat(fast.astype(int), np.arange(0, len(fast), 4))
            full = np.add.reduceat(np.ones(len(fast), int), np.arange(0, len(fast), 4)) == 4
            assert ((wg > 0) & (wg < 4) & full).any(), "fast and per-lane waves inside one workgroup"
        if case.heights == "block1e6":
            assert nan_w.any(), "block1e6: a NaN operand"
        if lr and case.heights == "pits":
            assert (flags & 2).all() and (paths == "B").any() and (paths == "C").any() and not (paths == "A").any()
        if lr and case.heights == "natural":
            assert (paths == "A").any() and (paths == "C").any()
        # (every group outside fast_groups holds a used slot, so a fast wave of the thread-per-evaluation kernels takes it through screen_pair3)
        slow_groups = [g for g in range(sc.K // 8) if not (tab["fast_groups"] >> g) & 1]
        assert (len(slow_groups) > 0) != case.two_region and all((tab["attr"][8 * g:8 * g + 8] >= 0).any() for g in slow_groups)
        if case.kernel in (sc.FEAT_SERIAL, sc.FEAT_SERIAL_LR):
            assert fast.any()
        st["fast_waves"], st["waves"] = int(fast.sum()), int(len(fast))

        # ---- and the labels behind all of it ----
        compare_full(eng, case.oracle(), xyz, cfg_kw, in_kw, check_dec=False, want=sc.oracle_want(case))
    finally:
        eng.close()
