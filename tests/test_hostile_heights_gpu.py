"""The attribute pipeline and the decision tiers on HOSTILE heights (tests/hostile_cases.py), against the oracle, on the MI355X.

Every other parity test keeps its heights natural, so the escape branches between the integral image and the label -- a screening band
set to infinity, the exact-integer tier's overflow flag, an fp16 operand image holding an infinity, decq4's range test -- were never
compared with the oracle: a wrong comparison direction in one of them would flip labels silently.  The reference has none of these
limits, so every case has a well-defined answer; the engine must give it, through whichever branch.

Testing build; the guard zones around every device buffer are checked after every request and after each test.  The oracle runs once
per (case, model) and process (hostile_cases.oracle_run).  What the tests measure on the way -- the share of evaluations each form of
the screening pass handed on, the tier counts, the worst decision error per exact tier -- goes to hostile_heights_stats.json, next to test_engine_gpu's
test_stats.json.

Share of the evaluations (5305 but for leftblock) the screening pass handed on (no calibration; surrogate / random model), as measured on the MI355X:
  first choice (plain form)   natural 0.85 / 0.001, scale8 0.017 / 0.015, half64 0.92 / 0.58, block1e6 0.89 / 0.25, ramp6 0.86 / 0.86,
                              spikes 0.97 / 0.76, pits 0.86 / 0.001, dyadic 0.87 / 0.001, flat 0.99 / 0.000,
                              leftblock (4934 evaluations) 0.70 / 0.56
  half64    plain 0.92 / 0.58, sumsq 0.87 / 0.58, centred-remainder/exp 0.59 / 0.58, /poly 0.89 / 0.85
  block1e6  plain 0.89 / 0.25, sumsq 0.78 / 0.25, centred-remainder/exp 0.26 / 0.25, /poly 0.87 / 0.73
  ramp6     plain 0.86 / 0.86, sumsq 0.86 / 0.86, centred-remainder/exp 1.00 / 0.86, /poly 1.00 / 1.00
  low-rank form, 128 x 128 (random under /exp, clustered under /poly): half64 0.56 / 0.057, block1e6 0.19 / 0.19, pits 0.000 / 0.000
What it hands on is decided by the three-pass kernel in list mode; beyond it the exact-integer tier saw 1281 / 1279 evaluations of
block1e6 (1279 of them on to the fp64 tier: the fp16 images hold an infinity), 425 of spikes (all on), 28 / 29 of ramp6 (28 on), none of
half64 (every kernel value of its hostile half underflows: S = 0, dec = -rho); nothing reached the strict tier."""
import numpy as np
import pytest

import hostile_cases as hc
from haf_grasping_amd import capi
from test_engine_gpu import DEC_ABS, MODES, _bits32, _bits64, compare_full, compare_probability, dump_stats, make_engine

pytestmark = pytest.mark.gpu

STATS = {}
HOSTILE = [c for c in hc.CASES if c != "natural"]
TIER_CASES = ["half64", "block1e6", "pits", "dyadic"]
FORM_CASES = ["half64", "block1e6", "ramp6"]


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module", autouse=True)
def _dump_stats():
    yield
    dump_stats(STATS, "hostile_heights_stats.json")


def _stat(*keys):
    d = STATS
    for k in keys:
        d = d.setdefault(str(k), {})
    return d


def _regimes(name, model, roll=0, grid=hc.GRID, length_x=46):
    orc = hc.oracle(model)
    return hc.regimes(orc, hc.oracle_run(name, model, grid, length_x), orc.model_arrays(), roll=roll)


def _check_empty_kernel_sums(eng, want, model):
    """Wherever the oracle's S = sum |coef| K is 0 (every kernel value underflows), the decision value is -rho."""
    rho = hc.oracle(model).model_arrays()["rho"]
    n = 0
    for roll in range(want["rolls_done"]):
        z = (want["mask"][roll] == 1) & (want["sabs"][roll] == 0)
        if z.any():
            d = eng.debug(capi.DBG_DECISION, 0, roll)[z]
            assert (np.abs(d + rho) <= DEC_ABS).all(), ("S == 0", roll, float(np.abs(d + rho).max()))
            n += int(z.sum())
    return n


def _tiers(eng):
    c = dict(eng.last_counts())
    c.update(eng.last_exact_tiers())
    return c


@pytest.mark.parametrize("route", ["direct", "tiers"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", hc.CASES)
def test_every_mode_stage_by_stage(data_dir, monkeypatch, name, mode, route):
    """compare_full in the three modes, both models: heights, integral image, mask, labels, vote grids and the grasp are the oracle's;
    decision values within the exact modes' bar (the default mode's bar is stated for attributes inside the range file only), and
    -rho wherever every kernel value underflows.  "direct": as the product serves a request of this size -- exact attributes and the
    fp64 decision of every evaluation in one launch, whatever the mode; "tiers" (HAF_NO_DIRECT): the mode's own first pass and the
    tiers behind it."""
    if route == "tiers":
        monkeypatch.setenv("HAF_NO_DIRECT", "1")
    cfg_kw, in_kw = hc.request()
    for model in hc.MODELS:
        want = hc.oracle_run(name, model)
        eng = make_engine(data_dir, hc.model_path(model), mode, testing=True, **cfg_kw)
        try:
            compare_full(eng, hc.oracle(model), hc.cloud(name), cfg_kw, in_kw, check_dec=bool(mode), want=want)
            n0 = _check_empty_kernel_sums(eng, want, model)
            c = _tiers(eng)
            assert (c["n_rechecked"] == c["n_fp64"] == c["n_evals"] and c["n_integer"] == 0) == (route == "direct"), c
            _stat("modes", name, model, route)[{0: "screen", capi.FLAG_SPLIT_F16: "splitf16", capi.FLAG_FP32_MFMA: "f32mfma"}[mode]] = \
                dict(c, n_s_zero=n0, screen_form=eng.screen_form())
        finally:
            eng.close()


def _check_margins(eng, name, model, want, grid=hc.GRID, length_x=46):
    """The header's rule for HAF_DBG_SCREEN_MARGIN: > 1 for the cells the screening pass decided, 0 for the cells it handed on -- and
    every cell whose attributes the screening arithmetic cannot hold (a feature outside decq4_float_scr's range, a scaled attribute
    beyond fp16) is one it handed on.  -> (cells looked at, of them handed on)"""
    seen = hostile = 0
    for roll in range(want["rolls_done"]):
        mg = eng.debug(capi.DBG_SCREEN_MARGIN, 0, roll)
        msk = want["mask"][roll] == 1
        assert np.isnan(mg[~msk]).all() and not np.isnan(mg[msk]).any(), ("margin grid", roll)
        decided = mg[msk] != 0
        assert (mg[msk][decided] > 1.0).all(), ("decided inside its band", roll, float(mg[msk][decided].min()))
        r = _regimes(name, model, roll, grid, length_x)
        never = r["big"] | r["f16"]
        got = mg[r["cells"][:, 0], r["cells"][:, 1]]
        assert (got[never] == 0).all(), ("the screening pass decided %d cells it cannot represent" % int((got[never] != 0).sum()), roll,
                                         r["cells"][never][got[never] != 0][:4].tolist())
        seen += len(never)
        hostile += int(never.sum())
    return seen, hostile


@pytest.mark.parametrize("name,variant", [(n, None) for n in hc.CASES] + [(n, v) for n in FORM_CASES for v in (0, 1, 2, 3)])
def test_screening_pass_hands_on_what_it_never_trusts(data_dir, monkeypatch, name, variant):
    """Default mode, the screening pass itself (no shortcut to the exact kernel, no calibration; the form pinned or the engine's
    first choice): stages and labels the oracle's, and the margin rule of _check_margins."""
    monkeypatch.setenv("HAF_NO_DIRECT", "1")
    monkeypatch.setenv("HAF_NO_CALIBRATE", "1")
    if variant is not None:
        monkeypatch.setenv("HAF_SCREEN_VARIANT", str(variant))
    cfg_kw, in_kw = hc.request()
    for model in hc.MODELS:
        want = hc.oracle_run(name, model)
        eng = make_engine(data_dir, hc.model_path(model), 0, testing=True, **cfg_kw)
        try:
            form = eng.screen_form()
            compare_full(eng, hc.oracle(model), hc.cloud(name), cfg_kw, in_kw, check_dec=False, want=want)
            _check_empty_kernel_sums(eng, want, model)
            seen, hostile = _check_margins(eng, name, model, want)
            c = _tiers(eng)
            assert c["n_evals"] == want["n_evals"]
            _stat("screening", name, model)["auto" if variant is None else "form%d" % variant] = \
                dict(c, form=form, refined_share=c["n_refined"] / max(1, c["n_evals"]), sampled=seen, sampled_never_trusted=hostile)
            if name in ("block1e6", "spikes", "ramp6"):
                assert hostile > 0
        finally:
            eng.close()


def _check_attr(eng, name, want, rolls, only_computed=False):
    """debug_attr of the sampled cells of every roll against the oracle's feature / q4 / scaled values, bit for bit."""
    orc = hc.oracle("surrogate")
    n = 0
    for roll in rolls:
        cells, attr, comp = eng.debug_attr(0, roll)
        mask_cells = np.stack(np.nonzero(want["mask"][roll]), 1)
        assert (cells == mask_cells).all(), ("cell list", roll)
        r = hc.regimes(orc, want, orc.model_arrays(), roll=roll)
        W = want["mask"].shape[2]
        pos = np.searchsorted(cells[:, 0] * W + cells[:, 1], r["cells"][:, 0] * W + r["cells"][:, 1])
        assert (cells[pos] == r["cells"]).all()
        if only_computed:
            mg = eng.debug(capi.DBG_SCREEN_MARGIN, 0, roll)
            assert (comp == (mg[cells[:, 0], cells[:, 1]] == 0)).all(), ("computed != handed on", roll)
            keep = comp[pos]
        else:
            assert comp.all()
            keep = np.ones(len(pos), bool)
        a = attr[pos[keep]]
        assert (_bits32(a["feature"]) == _bits32(r["F"][keep])).all(), (name, roll, "feature")
        assert (_bits64(a["q4"]) == _bits64(r["Q"][keep])).all(), (name, roll, "q4")
        assert (_bits64(a["scaled"][:, :323] + 0.0) == _bits64(r["S"][keep] + 0.0)).all(), (name, roll, "scaled")
        assert (a["scaled"][:, 323] == 0).all()
        n += int(keep.sum())
    return n


@pytest.mark.parametrize("route", ["direct", "splitf16", "f32mfma", "serial", "list"])
@pytest.mark.parametrize("name", HOSTILE)
def test_attribute_pipeline_bit_exact(data_dir, monkeypatch, name, route):
    """The fp32 feature, its "%.4g" round trip and the scaled value of 200 seeded cells per roll against hafo_feature_values /
    hafo_q4 / hafo_scale_row, bit for bit, through every kernel that writes attribute records:
      direct    as the product serves a request of this size: the one-launch exact kernel (k_small_direct), whatever the mode;
      splitf16, f32mfma (HAF_NO_DIRECT)  the wave-parallel exact-form feature kernels of the two exact modes (XMODE_SPLIT, XMODE_F32);
                the 82-cell rows give them a whole 64-chunk and a left-over.  The counters show that the request did not go direct;
      serial    k_features_serial (HAF_LARGE_EVALS), both exact modes;
      list      the list route behind the screening pass, which computes exactly the cells that pass handed on.
    An attribute of a cell whose kernel values all underflow cannot be caught through its label or decision value (dec = -rho
    whatever the attribute): these records are the only check of it."""
    cfg_kw, in_kw = hc.request()
    want = hc.oracle_run(name, "surrogate")
    if route == "serial":
        monkeypatch.setenv("HAF_LARGE_EVALS", "1")
    if route in ("splitf16", "f32mfma", "list"):
        monkeypatch.setenv("HAF_NO_DIRECT", "1")
    if route == "list":
        monkeypatch.setenv("HAF_NO_CALIBRATE", "1")
    modes = {"direct": [capi.FLAG_SPLIT_F16], "splitf16": [capi.FLAG_SPLIT_F16], "f32mfma": [capi.FLAG_FP32_MFMA],
             "serial": [capi.FLAG_SPLIT_F16, capi.FLAG_FP32_MFMA], "list": [0]}[route]
    for mode in modes:
        eng = make_engine(data_dir, hc.model_path("surrogate"), mode, testing=True, **cfg_kw)
        try:
            eng.score(hc.cloud(name), capi.default_input(**in_kw))
            c = _tiers(eng)
            went_direct = c["n_rechecked"] == c["n_fp64"] == c["n_evals"] and c["n_integer"] == 0
            assert went_direct == (route == "direct"), (route, c)
            n = _check_attr(eng, name, want, range(cfg_kw["n_rolls"]), only_computed=route == "list")
            if route == "list":
                assert sum(int(eng.debug_attr(0, r)[2].sum()) for r in range(cfg_kw["n_rolls"])) == c["n_refined"]
                _stat("attr_list_route", name)["checked"] = n
            else:
                assert n == min(200, int((want["mask"][0] == 1).sum())) + min(200, int((want["mask"][1] == 1).sum()))
        finally:
            eng.close()


def _handed_on_by_the_integer_tier(eng, H, W):
    """Linear indices (roll * H * W + row * W + col, sorted) of the evaluations on the exact-integer tier's hand-over list."""
    cells = eng.fetch_list(0)
    return np.sort(cells[eng.fetch_list(2)])


TIER_ENV = {"integer": dict(HAF_GUARD_REL="1e30"),
            "fp64": dict(HAF_GUARD_REL="1e30", HAF_NO_I8="1", HAF_GUARD0_REL="1e30"),
            "strict": dict(HAF_GUARD_REL="1e30", HAF_NO_I8="1", HAF_GUARD0_REL="1e30", HAF_GUARD2_REL="1e30", HAF_HOST_EXP_ALL="1")}
TIER_TOL = {"integer": 1e-6, "fp64": 2.0 ** -40, "strict": 0.0}      # (of S; the bars of test_exact_integer_tier / test_recheck_tiers_forced)


@pytest.mark.parametrize("tier", ["integer", "fp64", "strict"])
@pytest.mark.parametrize("name", TIER_CASES)
def test_each_exact_tier_alone(data_dir, monkeypatch, name, tier):
    """Every evaluation forced through one exact tier (the bands in front of it wide open), both models.  Labels, stages and the grasp
    are the oracle's (hard).  Exact-integer tier: every evaluation enters it; every evaluation with a scaled attribute beyond its
    fixed point (|x| > 15.874: the overflow flag; which ones, the ORACLE's attribute rows of all masked cells say) is on its hand-over
    list, and what that list holds besides -- evaluations inside the tier's own band -- stays under the 5 % of
    test_exact_integer_tier.  Strict tier with the host's exp: the decision values are the oracle's bit for bit (same order, same
    libm: no matter the magnitudes).  For the two tiers in front of it the worst decision error relative to S, over S > 0, is
    MEASURED against the bar their own tests use on natural data and written to the stats file with the cell; it is not asserted
    (labels are).  Measured on the MI355X (surrogate / random model): exact-integer tier 1.4e-9 / 8.2e-10 (half64),
    7.8e-10 / 5.0e-10 (block1e6), 7.9e-10 / 5.3e-10 (pits), 6.9e-10 / 5.3e-10 (dyadic) against 1e-6; fp64 tier 4.6e-15 / 9.2e-16,
    6.4e-16 / 8.8e-16, 8.7e-16 / 8.7e-16, 7.7e-16 / 8.9e-16 against 2^-40 = 9.1e-13: none above its bar.  3109 evaluations of half64
    and 1307 of block1e6 lie beyond the fixed point; the hand-over lists held 3109 and 1307 entries."""
    for k, v in TIER_ENV[tier].items():
        monkeypatch.setenv(k, v)
    cfg_kw, in_kw = hc.request()
    ovf = hc.beyond_fixed_point_cells(name) if tier == "integer" else None
    n_ovf = None if ovf is None else len(ovf)
    for model in hc.MODELS:
        want = hc.oracle_run(name, model)
        eng = make_engine(data_dir, hc.model_path(model), 0 if tier == "fp64" else capi.FLAG_SPLIT_F16, testing=True, **cfg_kw)
        try:
            compare_full(eng, hc.oracle(model), hc.cloud(name), cfg_kw, in_kw, check_dec=False, want=want)
            _check_empty_kernel_sums(eng, want, model)
            c = _tiers(eng)
            if tier == "integer":
                assert c["n_integer"] == c["n_rechecked"] == c["n_evals"] == want["n_evals"], c
                handed = _handed_on_by_the_integer_tier(eng, cfg_kw["grid_h"], cfg_kw["grid_w"])
                assert len(handed) == c["n_fp64"] and len(np.unique(handed)) == len(handed), (c, len(handed))
                missing = np.setdiff1d(ovf, handed)
                assert len(missing) == 0, ("beyond the fixed point but not handed on", len(missing), missing[:5].tolist())
                assert c["n_fp64"] - n_ovf < 0.05 * c["n_evals"], (c, n_ovf)
            elif tier == "fp64":
                assert c["n_refined"] == c["n_rechecked"] == c["n_evals"] == want["n_evals"] and c["n_integer"] == 0, c
            else:
                assert c["n_strict"] == c["n_evals"] == eng.last_strict_host() == want["n_evals"], c
            worst, where = 0.0, None
            for roll in range(want["rolls_done"]):
                d = eng.debug(capi.DBG_DECISION, 0, roll)
                m = want["mask"][roll] == 1
                if tier == "strict":
                    assert (d[m].view(np.uint64) == want["dec"][roll][m].view(np.uint64)).all(), ("strict tier decision bits", roll)
                s = (want["sabs"][roll] > 0) & m
                if s.any():
                    rel = np.zeros(d.shape)
                    rel[s] = np.abs(d[s] - want["dec"][roll][s]) / want["sabs"][roll][s]
                    if rel.max() > worst:
                        i, j = np.unravel_index(np.argmax(rel), rel.shape)
                        worst = float(rel.max())
                        where = dict(roll=roll, cell=(int(i), int(j)), dec=float(want["dec"][roll][i, j]), got=float(d[i, j]), S=float(want["sabs"][roll][i, j]))
            print(name, tier, model, c, "worst |dec - oracle| / S = %.3g" % worst, where)
            _stat("tiers", name, model)[tier] = dict(c, worst_rel_S=worst, bar=TIER_TOL[tier], above_bar=worst > TIER_TOL[tier], where=where,
                                                     n_beyond_fixed_point=n_ovf)
        finally:
            eng.close()


@pytest.mark.parametrize("name", ["half64", "block1e6", "pits"])
def test_low_rank_form(data_dir, monkeypatch, name):
    """The low-rank form of the screening pass (128 x 128 grid, thread-per-evaluation feature kernel: path A needs "no negative
    height in the grid", the band carries what the projection drops) on a strip of 38 x 128: the random model under the
    centred-remainder/exp form, the clustered model under the polynomial form.  The pass ran in the low-rank form, every stage and
    label is the oracle's, and the margin rule holds."""
    monkeypatch.setenv("HAF_NO_DIRECT", "1")
    monkeypatch.setenv("HAF_LARGE_EVALS", "1")
    monkeypatch.setenv("HAF_T0B", "0")
    G, LX = 128, 38
    cfg_kw, in_kw = hc.request(G, LX)
    for model, v in (("random", 2), ("clustered", 3)):
        monkeypatch.setenv("HAF_SCREEN_VARIANT", str(v))
        want = hc.oracle_run(name, model, G, LX)
        eng = make_engine(data_dir, hc.model_path(model), 0, testing=True, **cfg_kw)
        try:
            assert eng.screen_low_rank()["available"]
            compare_full(eng, hc.oracle(model), hc.cloud(name, G), cfg_kw, in_kw, check_dec=False, want=want)
            assert eng.screen_low_rank()["last_used"]
            _check_empty_kernel_sums(eng, want, model)
            seen, hostile = _check_margins(eng, name, model, want, G, LX)
            c = _tiers(eng)
            _stat("low_rank", name, model)["form%d" % v] = dict(c, refined_share=c["n_refined"] / max(1, c["n_evals"]), sampled=seen,
                                                               sampled_never_trusted=hostile)
            if name == "block1e6":
                assert hostile > 0
            if name == "pits":
                assert (want["heights"] < 0).sum() >= 100
        finally:
            eng.close()


def test_probability_mode(data_dir):
    """half64 with the surrogate's probability model: svm_predict_probability's labels, both "%g" probabilities of every cell, the
    fp32 vote grid and the grasp."""
    cfg_kw, in_kw = hc.request()
    eng = make_engine(data_dir, hc.model_path("surrogate_prob"), capi.FLAG_PROBABILITY, testing=True, **cfg_kw)
    try:
        got, want = compare_probability(eng, hc.oracle("surrogate_prob"), hc.cloud("half64"), cfg_kw, in_kw)
        assert want["n_evals"] > 5000
        _stat("probability")["half64"] = _tiers(eng)
    finally:
        eng.close()
