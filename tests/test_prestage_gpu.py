"""The pre-stage kernels (csrc/prestages.hip) on the MI355X against the oracle's stage functions, on every case of prestage_cases: grids
of 56 .. 1100 cells -- every size at which the launchers change the kernel, the pass count or the row ownership -- and clouds made to
hurt.  Per case and roll the height grid, the integral image and the mask equal the reference in every word, n_evals is the mask's sum, the
evaluation list equals its definition element for element, Engine.prestage_forms() names the kernels the case was built for, and no
integral image needed the sequential order.  Engines are reused across cases, in two orders.  At 601 and 1100 the features, the
decision and the vote run at W > 512 under a check.  Every comparison is an equality.  Testing build, the guard zones checked inside
every request and after every test."""
import os

import numpy as np
import pytest

import prestage_cases as pc
import vote_cases as vc
from haf_grasping_amd import capi
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U32 = np.uint32
FORMS_SEEN = {}


def _files(data_dir):
    return os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")          # every request checks the guard zones itself, too
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def engines(data_dir, surrogate):
    """one engine per grid size, made on first use and kept: the reuse tests go on where the case tests stopped"""
    made = {}

    def get(H):
        if H not in made:
            f, r = _files(data_dir)
            made[H] = capi.Engine(f, r, surrogate, testing=True, flags=capi.FLAG_KEEP_DEBUG, **pc.engine_kw(H))
        return made[H]
    get.drop = lambda H: made.pop(H).close()
    yield get
    for e in made.values():
        e.close()
    for H, seen in sorted(FORMS_SEEN.items()):            # which kernels every grid size ran (pytest -s shows it)
        print("prestage forms at %4d: %s" % (H, "; ".join(sorted(seen))))


def run_case(eng, case):
    """scores the case and compares everything the pre-stages left with the reference -> what a second run has to reproduce byte for byte"""
    name, H, _, in_kw, clouds, (first, count) = case
    ref = pc.case_reference(case)
    B, HW = len(clouds), H * H
    rec = eng.score_rolls(clouds, [capi.default_input(**in_kw)] * B, first, count)
    forms = eng.prestage_forms()
    FORMS_SEEN.setdefault(H, set()).add("%s / %s%s" % (eng.BIN_FORMS[forms["bin"]], eng.INTEGRAL_FORMS[forms["integral"]],
                                                    " (bucket path refused)" if forms["bucket_refused"] else ""))
    want_forms = pc.expected_forms(H, [len(c) for c in clouds])
    assert {k: forms[k] for k in want_forms} == want_forms, (name, forms, want_forms)
    assert forms["n_inexact_grids"] == 0 and eng.last_prestage()["n_inexact_grids"] == 0, (name, forms)
    snap = [rec.tobytes()]
    for b in range(B):
        r = ref["per_cloud"][b]
        for k in range(count):
            h, ii, m = (eng.debug(what, b, first + k) for what in (capi.DBG_HEIGHTS, capi.DBG_INTEGRAL, capi.DBG_MASK))
            bad = np.argwhere(h.view(U32) != r["heights"][k].view(U32))
            assert bad.size == 0, (name, "heights", b, k, len(bad), bad[:4].tolist())
            bad = np.argwhere(ii.view(U32) != r["integral"][k].view(U32))
            assert bad.size == 0, (name, "integral", b, k, len(bad), bad[:4].tolist())
            bad = np.argwhere(m != r["mask"][k])
            assert bad.size == 0, (name, "mask", b, k, len(bad), bad[:4].tolist())
            assert int(rec["n_evals"][b, k]) == int(r["mask"][k].sum()), (name, "n_evals", b, k)
            snap += [h.tobytes(), ii.tobytes(), m.tobytes()]
    want = ref["list"]
    lst = eng.fetch_list(0, cap=want.size + 64)
    assert lst.size == want.size, (name, "list length", lst.size, want.size)
    if forms["integral"] == pc.INTEGRAL_FUSED:
        # the fused kernel: a run of row-major cells per (cloud, roll), the order of the runs unspecified
        cut = np.flatnonzero(np.diff(lst // HW)) + 1
        runs = np.split(lst, cut) if lst.size else []
        grids = [int(s[0]) // HW for s in runs]
        assert len(set(grids)) == len(grids) == int((ref["masks"].reshape(B * count, -1).sum(axis=1) > 0).sum()), (name, grids)
        for g, s in zip(grids, runs):
            assert np.array_equal(s - g * HW, pc.row_major_list(ref["masks"][g // count, g % count])), (name, "list of grid", g)
    else:
        bad = np.flatnonzero(lst != want)
        assert bad.size == 0, (name, "list", len(bad), bad[:4].tolist(), lst[bad[:4]].tolist(), want[bad[:4]].tolist())
        snap.append(lst.tobytes())
    return snap


@pytest.mark.parametrize("H", [56, 63, 64, 70, 71, 128, 129, 192])
def test_small_and_boundary_grids(engines, H):
    """56 and 63 fused (63 the largest), 64 and 70 k_integral_small (70 the largest), 71 the smallest band form, 128 k_bin_lds at exactly
    64 KiB, 129 the first tiled grid with a one-cell last tile, 192 tiles of 3 x 3"""
    for case in pc.cases(H):
        run_case(engines(H), case)


def test_grid_576(engines):
    """W > 512: the second 512-column pass of the band form (carry, row_carry); buckets of 9 cells"""
    for case in pc.cases(576):
        run_case(engines(576), case)


@pytest.mark.parametrize("H", [56, 128, 192, 576])
def test_reused_engine_state(engines, H):
    """the same engine again, the cases in another order, an empty request between two large ones, and one case scored twice with
    identical fetches: the key fill, inexact_flags, bkt_count, the sorted buffer and the brslot epochs of a request owe nothing to the last"""
    eng = engines(H)
    cs = list(reversed(pc.cases(H)))
    n = [sum(len(x) for x in c[4]) for c in cs]
    at = next(i for i in range(len(cs) - 1) if min(n[i], n[i + 1]) >= 32767)
    cs.insert(at + 1, pc.empty(H, cs[at][5]))
    for case in cs:
        run_case(eng, case)
    twice = next(c for c in pc.cases(H) if c[0] == "one_bucket")
    assert run_case(eng, twice) == run_case(eng, twice)


def downstream(eng, case, data_dir, surrogate, cells_per_roll=200):
    """behind the pre-stages of a grid wider than 512: for random masked cells of every roll the engine's label equals the oracle's
    feature -> scale -> decision chain fed with the ENGINE's integral image; the vote grid equals hafo_vote on the engine's own label
    grid, the roll record hafo_vote's best"""
    name, H, _, in_kw, clouds, (first, count) = case
    f, r = _files(data_dir)
    o = O.Oracle(f, r, surrogate)
    m = o.model_arrays()
    skip = np.zeros(325, np.uint8)
    skip[324] = 1
    rng = np.random.RandomState(H)
    rec = eng.score_rolls(clouds, [capi.default_input(**in_kw)], first, count)[0]
    for k in range(count):
        ii, lab, msk = (eng.debug(what, 0, first + k) for what in (capi.DBG_INTEGRAL, capi.DBG_LABELS, capi.DBG_MASK))
        cells = np.argwhere(msk == 1)
        assert len(cells) == rec["n_evals"][k]
        for i, j in cells[rng.choice(len(cells), cells_per_roll, replace=False)]:
            feats = o.feature_values(ii[i - 7:i + 8, j - 7:j + 8])
            d = o.decision(o.scale_row(np.array([O.q4(v) for v in feats]), m["D"], skip))
            assert lab[i, j] == (m["label"][0] if d > 0 else m["label"][1]), (name, k, i, j, d)
        ev, (top, row, col) = vc.oracle_vote(lab)
        got, _ = eng.roll_grid(0, first + k)
        assert (got.view(U32) == ev.view(U32)).all(), (name, "vote grid", k)
        assert (int(rec["vote"][k]), int(rec["row"][k]), int(rec["col"][k])) == (top, row, col), (name, "record", k)


def test_grid_601(engines, data_dir, surrogate):
    """W > 512 with W % 4 != 0 (the scalar loads of the band form under the pass carry); 17 x 17 ... 10 x 10 tiles; the bucket grid of 97 x
    97 exceeds the LDS histogram, so 300 000 points go through k_bin -- and prestage_forms says so"""
    for case in pc.cases(601):
        run_case(engines(601), case)
    assert engines(601).prestage_forms()["bucket_refused"]
    downstream(engines(601), pc.cases(601)[0], data_dir, surrogate)
    engines.drop(601)


def test_grid_1100(engines, data_dir, surrogate):
    """H > 1024: a thread of k_scan owns two rows; W = 1100: three 512-column passes, W % 8 == 4 (a lane's last group of eight straddles
    W), buckets of 17 cells; the strip search area puts masked cells into every row of the grid at roll 0 and most at the others"""
    for case in pc.cases(1100):
        run_case(engines(1100), case)
    downstream(engines(1100), pc.cases(1100)[0], data_dir, surrogate)
    engines.drop(1100)
