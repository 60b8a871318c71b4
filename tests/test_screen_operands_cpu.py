"""The reference of the screening feature pass (tests/screen_operand_cases.py) held to the oracle's truth, without a GPU.

  * u' against u = c x, x the oracle's scaled attribute through the REAL "%.4g" and "%g" text round trips (hafo_q4, hafo_scale_row):
    per slot |u' - u| <= kScreenEtaRel |u'| plus, in norm over the slots, the table's eta_abs -- the claim in the comment above
    screen_attribute (csrc/feature_device.h) that the whole guard band starts from -- for every request of the GPU test, hostile heights
    included; and u' is NaN exactly where the feature value is outside decq4_float_scr's range (hostile_cases.regimes: "big").
  * the slot table of the device-free build against the range file (screen_operand_cases.check_table).
  * v_exact (Python integers) against math.fsum over the twelve corner terms with exact products, on 1 000 seeded windows.
  * the exact fp32 fma against fractions.Fraction, fp32 ties of the fp64 shortcut included.
  * the coverage the GPU test asserts, on the reference alone: wave kinds, predicted low-rank paths, NaN operands, finite noise sums."""
import math
from fractions import Fraction

import numpy as np
import pytest

import hostile_cases as hc
import screen_operand_cases as sc

CASES = sc.cases()


def _requests():
    """One case per distinct (heights, model, grid, search area): what the reference depends on."""
    seen, out = set(), []
    for c in CASES:
        key = (c.heights, c.model, c.grid, c.lx, c.ly, c.rolls, c.two_region)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _host_view(case):
    """(want, cells in the general pre-stages' order, per-roll flags word as the device would set bit 1)"""
    want = sc.oracle_want(case)
    cells = sc.evaluation_order(want["mask"])
    assert len(cells) == want["n_evals"]
    flags = np.array([2 if (want["heights"][r] < 0).any() else 0 for r in range(case.rolls)])
    return want, cells, flags


def _attr_rows(orc, ii, cells, nshaf):
    """(features fp32 [n, 324], scaled [n, 323]) of the oracle through both real text round trips (as hostile_cases.oracle_attr_rows,
    with the feature file's SHAF boundary given)."""
    skip = np.zeros(325, np.uint8)
    skip[324] = 1
    F, S = [], []
    for i, j in cells:
        f = orc.feature_values(ii[i - 7:i + 8, j - 7:j + 8], nshaf)
        F.append(f)
        S.append(orc.scale_row(hc.q4_row(orc, f), 323, skip))
    return np.array(F), np.array(S)


def test_exact_fma_against_fractions():
    rng = np.random.RandomState(3)
    q = (rng.standard_normal(4000) * 10.0 ** rng.randint(-6, 4, 4000)).astype(np.float32)
    m = (rng.standard_normal(4000) * 10.0 ** rng.randint(-3, 2, 4000)).astype(np.float32)
    a = (rng.standard_normal(4000) * 10.0 ** rng.randint(-3, 2, 4000)).astype(np.float32)
    # fp32 ties that the fp64 sum rounds onto: q m = an odd multiple of half an fp32 ulp of the result, a = far below fp64's last bit of it
    tq = np.array([1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, 3.0, 1.0 + 2.0 ** -12], np.float32)
    tm = np.array([1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, 0.5 + 2.0 ** -25, -(1.0 + 2.0 ** -12)], np.float32)
    ta = np.array([2.0 ** -90, -2.0 ** -90, 2.0 ** -80, 2.0 ** -90], np.float32)
    q, m, a = np.concatenate([q, tq]), np.concatenate([m, tm]), np.concatenate([a, ta])
    got, hard = sc.exact_fma32(q, m, a)
    assert hard >= 2, "the constructed ties must take the exact route"
    for i in range(len(q)):
        x = Fraction(float(q[i])) * Fraction(float(m[i])) + Fraction(float(a[i]))
        assert float(got[i]) == sc._rn32(x), (i, float(q[i]), float(m[i]), float(a[i]))
    # _rn32 itself: nearest, ties to even
    one, up = Fraction(1), Fraction(float(np.nextafter(np.float32(1), np.float32(2))))
    assert sc._rn32((one + up) / 2) == 1.0 and sc._rn32((one + up) / 2 + Fraction(1, 2 ** 60)) == float(up)
    assert np.isnan(sc.exact_fma32(np.float32(np.nan), np.float32(1), np.float32(1))[0])


@pytest.mark.parametrize("model,grid,nofast", [("surrogate", 96, False), ("surrogate", 96, True), ("surrogate", 128, False), ("surrogate", 160, False),
                                               ("random", 128, False), ("clustered", 128, False), ("random-tworegion", 128, False)])
def test_slot_table_against_the_range_file(monkeypatch, model, grid, nofast):
    if nofast:
        monkeypatch.setenv("HAF_NO_FAST_GROUPS", "1")
    if model == "random-tworegion":
        case = next(c for c in CASES if c.two_region)
        orc = case.oracle()
        gamma = orc.model_arrays()["gamma"]
        tabs = {form: sc.table_for(case, form) for form in sc.FORMS}
        for tab in tabs.values():
            sc.check_table(orc, gamma, tab)
            assert tab["fast_groups"] == (1 << 40) - 1 and (tab["pad"][tab["attr"] >= 0] != 0).all(), "every slot a two-region HAF feature"
        return
    orc = hc.oracle(model)
    gamma = orc.model_arrays()["gamma"]
    reg, w = orc.feature_table()
    assert (w[:, 3] == 0).all(), "the reference drops the fourth region's weight"
    tabs = {form: sc.slot_table(hc.model_path(model), grid, form) for form in sc.FORMS}
    assert all(t is not None for t in tabs.values()), "the models of the GPU test get all three forms"
    for tab in tabs.values():
        sc.check_table(orc, gamma, tab)
        assert (tab["attr"] < 323).all()
    plain, cr = tabs["screen"], tabs["screen_cr"]
    assert (plain["attr"] == cr["attr"]).all() and (plain["mul"] == cr["mul"]).all() and plain["fast_groups"] == cr["fast_groups"]
    assert cr["cr"] == 1 and plain["cr"] == 0 and cr["lr_rho"] > 0


@pytest.mark.parametrize("case", _requests(), ids=lambda c: "-".join([c.row, c.heights, c.model]))
def test_reference_against_the_oracle_and_coverage(case):
    want, cells, flags = _host_view(case)
    G = case.grid
    orc = case.oracle()
    tab = sc.table_for(case, "screen")
    ii = want["integral"]
    idx = sc.sample(cells, G, G)
    lr = case.low_rank()
    ref = sc.reference(case, tab, ii, cells, idx, exact=lr)
    used = tab["attr"] >= 0
    attr = tab["attr"][used]

    # ---- u' against the oracle's u = c x ----
    rc = np.stack(np.divmod(cells[idx] % (G * G), G), 1)
    roll = cells[idx] // (G * G)
    F = np.empty((len(idx), orc.n_features), np.float32)
    X = np.empty((len(idx), 323))
    for r in range(case.rolls):
        m = roll == r
        if m.any():
            F[m], X[m] = _attr_rows(orc, ii[r], rc[m], case.nshaf())
    assert (F.view(np.uint32) == ref["F"].view(np.uint32)).all()
    Fu = F[:, attr].astype(np.float64)
    big = (np.abs(Fu) >= hc.DECQ_MAX) | ((Fu != 0) & (np.abs(Fu) < hc.DECQ_MIN))
    u1 = ref["u1"][:, used].astype(np.float64)
    assert (np.isnan(u1) == big).all(), "u' is NaN exactly where the feature value leaves the decimal path's range"
    u = tab["c"] * X[:, attr]
    with np.errstate(invalid="ignore"):
        excess = np.where(big, 0.0, np.maximum(0.0, np.abs(u1 - u) - sc.ETA_REL * np.abs(u1)))
    norm = np.sqrt((excess * excess).sum(axis=1))
    worst = int(np.argmax(norm))
    print(case.id, "worst |u' - u| beyond the relative part: %.3g of eta_abs %.3g" % (norm[worst], tab["eta_abs"]))
    assert norm[worst] <= tab["eta_abs"], (int(idx[worst]), float(norm[worst]), tab["eta_abs"])
    # the same claim for the centred table (every form 2 / 3 and low-rank case reads it): p' + mu against c x, relative to |u'| = |p' + mu|,
    # with the centred table's own eta_abs
    tab_c = sc.table_for(case, "screen_cr")
    assert tab_c is not None and (tab_c["attr"] == tab["attr"]).all()
    p1 = sc.operands(ref["V"], tab_c)[1][:, used].astype(np.float64)
    assert (np.isnan(p1) == big).all()
    uc = p1 + tab_c["mu"][used][None, :]
    with np.errstate(invalid="ignore"):
        excess_c = np.where(big, 0.0, np.maximum(0.0, np.abs(uc - u) - sc.ETA_REL * np.abs(uc)))
    norm_c = np.sqrt((excess_c * excess_c).sum(axis=1))
    print(case.id, "centred: worst %.3g of eta_abs %.3g" % (norm_c.max(), tab_c["eta_abs"]))
    assert norm_c.max() <= tab_c["eta_abs"], (int(idx[int(np.argmax(norm_c))]), float(norm_c.max()), tab_c["eta_abs"])

    # ---- coverage of the GPU test, from the reference alone ----
    fast = sc.wave_kinds(cells)
    if case.grid == 96:
        assert fast.any() and not fast.all()
    if case.heights == "holes":
        wg = np.add.reduceat(fast.astype(int), np.arange(0, len(fast), 4))
        full = np.add.reduceat(np.ones(len(fast), int), np.arange(0, len(fast), 4)) == 4
        assert ((wg > 0) & (wg < 4) & full).any()
    if case.heights == "block1e6":
        assert big.any()
    if lr:
        paths = sc.predict_paths(cells, ii, G, G, flags)
        if case.heights == "pits":
            assert flags.all() and (paths == "B").any() and (paths == "C").any() and not (paths == "A").any()
        if case.heights == "natural":
            assert (paths == "A").any() and (paths == "C").any()
        tab_cr = sc.table_for(case, "screen_cr")
        ref_cr = sc.reference(case, tab_cr, ii, cells, idx, exact=True)
        ok = ~np.isnan(ref_cr["u1"][:, tab_cr["pad"] != 0]).any(axis=1)
        assert np.isfinite(ref_cr["noise"][ok]).all() and (ref_cr["noise"][ok] >= 0).all() and ok.any()
        assert np.isnan(ref_cr["noise"][~ok]).all()
        if case.heights == "pits":
            assert (ref_cr["rmin"] < 0).any(), "pits: negative region sums among the sampled evaluations"


def test_v_exact_against_fsum():
    """1 000 seeded windows of the natural, block1e6 and pits grids: the integer route and math.fsum over exact products give the same
    correctly rounded double for every HAF slot."""
    case = next(c for c in CASES if c.row == "small" and c.heights == "natural")
    tab = sc.table_for(case, "screen")
    orc = hc.oracle("surrogate")
    rng = np.random.RandomState(11)
    wins = []
    for h, n in (("natural", 400), ("block1e6", 300), ("pits", 300)):
        want = hc.oracle_run(h, "surrogate")
        cells = sc.evaluation_order(want["mask"])
        wins.append(sc.windows(want["integral"], cells[rng.choice(len(cells), n, replace=False)], hc.GRID, hc.GRID))
    wins = np.concatenate(wins)
    vex, rmin = sc.v_exact(wins, tab, orc)
    haf = tab["pad"] != 0
    assert haf.sum() > 250 and np.isnan(vex[:, ~haf]).all() and (rmin <= 0).all() and (rmin < 0).any()
    for i, w in enumerate(wins):
        second = sc.v_exact_fsum(w, tab, orc)
        assert (second[haf] == vex[i, haf]).all(), i
    # and the fp32 feature value is v_exact up to the reference's own roundings (a sanity bound, not the kernel's)
    V, _ = sc.slot_values(orc, wins, tab)
    scale = np.abs(wins.reshape(len(wins), -1)).max(axis=1, keepdims=True).astype(np.float64)
    assert (np.abs(V[:, haf].astype(np.float64) - vex[:, haf]) <= 40 * 2.0 ** -24 * scale).all()


def test_image_layout_and_order():
    offs = np.array([[sc.image_offset(r, k) for k in range(sc.K)] for r in range(sc.TILE_EVALS)])
    assert len(np.unique(offs)) == offs.size and offs.min() == 0 and offs.max() == sc.TILE_BYTES - 2 and (offs % 2 == 0).all()
    assert [sc.image_offset(0, k) for k in range(9)] == [0, 2, 4, 6, 8, 10, 12, 14, 256]
    assert sc.image_offset(1, 0) == 16 and sc.image_offset(16, 0) == 1024 and sc.image_offset(0, 32) == 2048
    mask = np.zeros((1, 3, 200), np.uint8)
    mask[0, 1, 10:150] = 1                                           # 140 cells: remainder 12 from the row's start, two whole chunks
    mask[0, 2, 5:45] = 1                                             # 40 cells: all remainder
    cells = sc.evaluation_order(mask)
    assert list(cells[:128]) == list(200 + np.arange(22, 150)) and list(cells[128:140]) == list(200 + np.arange(10, 22))
    assert list(cells[140:]) == list(400 + np.arange(5, 45))
    assert list(sc.wave_kinds(cells)) == [True, True, False]
