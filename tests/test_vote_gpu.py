"""The stages behind the labels on the MI355X -- k_vote_small, k_vote_cells / k_vote_pick / k_vote_record and their ROI forms,
k_prob_vote_cells / k_prob_pick, k_top_grasps, k_grasp_map / k_map_best / k_cell_record -- on the hand-made grids of tests/vote_cases.py,
which no request through a model can produce: labels on the border, runs of chosen lengths across the kernels' seams, ties, negative
votes, label values up to 99, float grids for both branches of the truncating maximum.  haf_test_revote (testing build) replaces the
last batch's grids and runs the request path's own vote launchers on them.  Then models whose labels are not +-1 end to end.

Every comparison is an equality of integers or of float bit patterns.  Grid sizes, the smallest at which each path exists:
15 the smallest grid haf_create accepts; 56 k_vote_small with 16-byte label loads; 61 k_vote_small with byte loads; 128 k_vote_small at
its 16 384-cell limit; 131 scalar k_vote_cells, scalar pick; 132 quad k_vote_cells, scalar pick; 136 quad k_vote_cells, 8-wide pick and
three 64-column pieces in k_top_grasps.  One engine per size, max_clouds = 2 and 4 rolls: eight grids per launch, a case in each."""
import json
import os

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import models
import pcdio
import roi_cases as rc
import vote_cases as vc
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import compare_full, compare_probability
from test_roi_gpu import check_roi_state, expected
from top_grasps_cases import POSE, assert_same, mirror

pytestmark = pytest.mark.gpu

F = np.float32
B, R = 2, 4
TINY = np.array([[0.0, 0.0, 0.05], [0.01, 0.0, 0.05], [0.0, 0.01, 0.06]], F)


def _files(data_dir):
    return os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def prob_model(golden_dir, tmp_path_factory):
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    return models.write_probability_model(str(tmp_path_factory.mktemp("vote") / "surrogate_prob.model"), os.path.join(golden_dir, "surrogate.model"),
                                          pj["probA"], pj["probB"])


@pytest.fixture(scope="module")
def engines(data_dir, golden_dir, prob_model):
    """one engine per (grid size, probability) for the whole module, its last batch 2 clouds x 4 rolls of a tiny cloud"""
    made = {}

    def get(N, prob=False):
        if (N, prob) not in made:
            f, r = _files(data_dir)
            eng = capi.Engine(f, r, prob_model if prob else os.path.join(golden_dir, "surrogate.model"), testing=True, grid_h=N, grid_w=N,
                              n_rolls=R, max_clouds=B, max_points=1 << 15, flags=capi.FLAG_KEEP_DEBUG | (capi.FLAG_PROBABILITY if prob else 0))
            made[N, prob] = eng
        eng = made[N, prob]
        gi = capi.default_input(grasp_area_length_x=min(N - 2, 60), grasp_area_length_y=min(N - 2, 60))
        eng.score_batch([TINY, TINY], [gi, gi])
        return eng, gi
    yield get
    for eng in made.values():
        eng.close()


def heights_for(N, seed=0):
    """a height grid for the cases that bring none: values around -10 and 0, some exactly -10, zeros of both signs"""
    rng = np.random.RandomState(100 + seed)
    h = rng.uniform(-11.0, 1.0, size=(N, N)).astype(F)
    h[rng.uniform(size=(N, N)) < 0.05] = -10.0
    h[rng.uniform(size=(N, N)) < 0.02] = 0.0
    h[rng.uniform(size=(N, N)) < 0.02] = -0.0
    return h


def groups(items):
    """eight (grid, heights, ...) items per launch; the last launch is filled up with its first item"""
    for i in range(0, len(items), B * R):
        g = items[i:i + B * R]
        yield g + [g[0]] * (B * R - len(g)), len(g)


def stack(arrs, dt):
    return np.stack(arrs).astype(dt).reshape((B, R) + np.shape(arrs[0]))


def fetch(eng, slot):
    return eng.roll_grid(slot // R, slot % R)[0]


def int_family(N, fam):
    if fam.startswith("border"):
        return vc.border(N, -1 if fam == "border-1" else +1)
    return vc.FAMILIES[fam](N)


INT_FAMILIES = list(vc.FAMILIES) + ["border-1", "border+1"]


@pytest.mark.parametrize("fam", INT_FAMILIES)
@pytest.mark.parametrize("N", vc.SIZES)
def test_vote_and_record_plain(engines, N, fam):
    """the vote grid from haf_get_roll_grid and the record (vote, row, col, h_locmax) equal hafo_vote plus the mirror's z window, in every
    one of the eight slots; n_evals is the last request's, untouched"""
    cases = int_family(N, fam)
    if not cases:
        assert fam == "block_seams" and N < 129
        return
    eng, gi = engines(N)
    n_evals = eng.score_rolls([TINY, TINY], [gi, gi], 0, R)["n_evals"].reshape(-1)
    items = [(c, c.heights if c.heights is not None else heights_for(N, i % 5)) for i, c in enumerate(cases)]
    for grp, live in groups(items):
        rec = eng.revote(labels=stack([c.grid for c, _ in grp], np.int8), heights=stack([h for _, h in grp], F)).reshape(-1)
        for slot in range(live):
            c, h = grp[slot]
            ev, (top, row, col) = vc.oracle_vote(c.grid)
            got = fetch(eng, slot)
            assert (_bits(got) == _bits(ev)).all(), (c, slot, int((got != ev).sum()))
            r = rec[slot]
            assert (int(r["vote"]), int(r["row"]), int(r["col"])) == (top, row, col), (c, slot, r, (top, row, col))
            assert _bits(r["h_locmax"]) == _bits(vc.z_key(h, row, col)), (c, slot, r["h_locmax"], vc.z_key(h, row, col))
            assert r["n_evals"] == n_evals[slot]
            if slot == 0:                                    # the uploaded heights are what the getters see
                assert (eng.debug(capi.DBG_HEIGHTS, 0, 0).view(np.uint32) == h.view(np.uint32)).all()


def roi_state(eng, N):
    """a small haf_score_frames_roi request of two frames: the engine has its ROI cell sets, the last batch is 2 x 4 again"""
    img = np.zeros((1, 4, 3), F)
    img[0, :, :] = TINY[0]
    frame = capi.xyz_frame(img)
    gi = capi.default_input(grasp_area_length_x=min(N - 2, 60), grasp_area_length_y=min(N - 2, 60))
    eng.score_frames_roi([frame, frame], [np.ones((1, 4), np.uint8)] * 2, [gi, gi])


@pytest.mark.parametrize("N", vc.SIZES)
def test_vote_and_record_roi(engines, N):
    """the ROI form with S empty, full, a checkerboard, single cells at columns 63, 64 and N-5, one whole row: the gated mirror; with S
    full the ungated kernel's grids"""
    eng, gi = engines(N)
    with pytest.raises(capi.HafError) as ei:                 # no ROI request yet: no cell sets to vote under
        eng.revote(labels=np.full((B, R, N, N), -1, np.int8), roi_words=np.zeros((B, R, N, (N + 63) // 64), np.uint64))
    assert ei.value.code == capi.HAF_E_ARG and "ROI" in str(ei.value)
    roi_state(eng, N)
    cases = vc.ties(N) + vc.negative(N) + vc.random_grids(N)[3:] + vc.run_lengths(N)[::5] + vc.block_seams(N)[::3] + vc.constant(N)[2:4]
    items = [(c, heights_for(N, i % 5), name, S) for i, c in enumerate(cases) for name, S in vc.roi_sets(N)]
    sets = dict(vc.roi_sets(N))
    # a top that the gate removes: the gated grid's winner is another cell (the gate acts BEFORE the argmax)
    for c in vc.ties(N)[:4]:
        _, row, col = vc.record_int(vc.vote_int(c.grid))
        S = np.ones((N, N), bool)
        S[row, col] = False
        items.append((c, heights_for(N, 1), "all but the winner", S))
    plain = {}
    for grp, live in groups(items):
        rec = eng.revote(labels=stack([c.grid for c, _, _, _ in grp], np.int8), heights=stack([h for _, h, _, _ in grp], F),
                         roi_words=vc.roi_words(np.stack([S for _, _, _, S in grp]).reshape(B, R, N, N))).reshape(-1)
        for slot in range(live):
            c, h, name, S = grp[slot]
            want = vc.vote_int(c.grid, S)
            top, row, col = vc.record_int(want)
            got = fetch(eng, slot)
            assert (got == want.astype(F)).all(), (c, name, slot, int((got != want).sum()))
            r = rec[slot]
            assert (int(r["vote"]), int(r["row"]), int(r["col"])) == (top, row, col), (c, name, slot, r, (top, row, col))
            assert _bits(r["h_locmax"]) == _bits(vc.z_key(h, row, col)), (c, name, slot)
            if name == "full":
                plain[id(c)] = (c, got, (top, row, col))
            if name == "empty":
                assert not got.any() and (top, row, col) == (0, 0, N - 1 - N // 2)
    assert len(plain) == len(cases)
    for c, got, record in plain.values():                   # S full: what hafo_vote gives
        ev, rec = vc.oracle_vote(c.grid)
        assert (_bits(got) == _bits(ev)).all() and rec == record, c
    assert sets["full"].all()


@pytest.mark.parametrize("N", vc.FLOAT_SIZES)
def test_vote_and_record_probability(engines, N):
    """the probability form on every float family: d_evf bit for bit and the record equal hafo_vote_f; h_locmax is the sequential
    maximum of the reference (of -0.0 and +0.0 the first stays)"""
    eng, gi = engines(N, prob=True)
    hs = [c.heights for c in vc.height_cases(N)]
    items = [(c, hs[i % len(hs)]) for i, c in enumerate(vc.float_cases(N))]
    for zh in hs[-2:]:                                       # a winner at (6, 6) under the two zero-sign windows
        g = np.zeros((N, N), F)
        g[6, 6] = 1.0
        items.append((vc.Case("exact winner at 6,6", g, top=55, row=6, col=6), zh))
    seen = set()
    for grp, live in groups(items):
        rec = eng.revote(gridf=stack([c.grid for c, _ in grp], F), heights=stack([h for _, h in grp], F)).reshape(-1)
        for slot in range(live):
            c, h = grp[slot]
            ev, (top, row, col) = vc.oracle_vote(c.grid)
            assert (top, row, col) == vc.record_f32(vc.vote_f32(c.grid))[:3]
            seen.add(vc.record_f32(ev)[3])
            got = fetch(eng, slot)
            assert (_bits(got) == _bits(ev)).all(), (c, slot, int((_bits(got) != _bits(ev)).sum()))
            r = rec[slot]
            assert (int(r["vote"]), int(r["row"]), int(r["col"])) == (top, row, col), (c, slot, r, (top, row, col))
            assert _bits(r["h_locmax"]) == _bits(vc.z_seq(h, row, col)), (c, slot, r["h_locmax"], vc.z_seq(h, row, col))
    assert seen == {"run", "first", "later"}
    with pytest.raises(capi.HafError):                       # labels go with a plain engine
        eng.revote(labels=np.full((B, R, N, N), -1, np.int8))


RANK_PARAMS = [dict(), dict(k=1024, cell_radius=0, min_vote=1), dict(min_vote=30000)]


@pytest.mark.parametrize("params", RANK_PARAMS, ids=["default", "k1024_r0_v1", "v30000"])
@pytest.mark.parametrize("N", vc.SIZES)
def test_ranking(engines, N, params):
    """haf_top_grasps on re-voted grids of the run-length, tie, all-99, negative-vote and random families against the numpy mirror of
    its contract (top_grasps_cases.mirror), which reads the same grids back through haf_get_roll_grid.  The grids of 99s with holes
    need a third 8-bit digit of the sort key (test_vote_cpu.py asserts lbits + vbits > 16 for them).  min_vote is >= 1 in every set
    (the contract, see the next test), so k_top_grasps meets the zero and negative votes of these grids only as non-candidates: cells
    that end a run and that no candidate list may hold."""
    eng, gi = engines(N)
    cases = vc.ranking(N) + vc.ties(N) + vc.negative(N) + vc.random_grids(N) + vc.run_lengths(N)[::4] + vc.block_seams(N)[::6]
    items = [(c, heights_for(N, i % 5)) for i, c in enumerate(cases)]
    total = 0
    for grp, live in groups(items):
        rec = eng.revote(labels=stack([c.grid for c, _ in grp], np.int8), heights=stack([h for _, h in grp], F))
        got = eng.top_grasps(**params)
        assert len(got) == B
        for b in range(B):
            want = mirror(eng, gi, b, 0, R, rec["n_evals"][b], **params)
            assert_same(got[b], want, (N, [c.name for c, _ in grp[b * R:(b + 1) * R]], params))
            total += len(want)
            if params.get("cell_radius") == 0 and want:      # rank 1 is the best roll record; every record of the cloud that scores is a candidate
                best = max(range(R), key=lambda r: (int(rec["vote"][b, r]), -r))
                assert (want[0]["best_vote"], want[0]["best_roll"], want[0]["best_row"], want[0]["best_col"]) == \
                    (int(rec["vote"][b, best]), best, int(rec["row"][b, best]), int(rec["col"][b, best]))
    assert (total == 0) == (params.get("min_vote") == 30000)


@pytest.mark.parametrize("N", (15, 136))
def test_ranking_refuses_a_min_vote_below_one(engines, N):
    """haf_top_params.min_vote is >= 1 by contract (include/hafgrasp.h): zero runs and negative runs are never candidates, so
    min_vote = 0 and min_vote = -1000 are refused with HAF_E_ARG on re-voted grids as on scored ones, and the last batch stays usable"""
    eng, gi = engines(N)
    cases = vc.negative(N) + vc.ranking(N)
    eng.revote(labels=stack([c.grid for c in cases], np.int8), heights=stack([heights_for(N)] * 8, F))
    before = eng.top_grasps(min_vote=1, k=64)
    for mv in (0, -1000):
        with pytest.raises(capi.HafError) as ei:
            eng.top_grasps(min_vote=mv)
        assert ei.value.code == capi.HAF_E_ARG and "min_vote" in str(ei.value)
    assert eng.top_grasps(min_vote=1, k=64) == before and any(before)


def cell_centre_frame(N):
    """an XYZ frame with one point in the middle of every 1 cm cell of the N x N area around the origin, and its image"""
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    img = np.stack([(ii + 0.5) * 0.01 - N * 0.005, (jj + 0.5) * 0.01 - N * 0.005, np.full((N, N), 0.05)], -1).astype(F)
    return capi.xyz_frame(img), img


@pytest.mark.parametrize("N", vc.FLOAT_SIZES)
def test_maps(engines, N):
    """haf_grasp_map, haf_grasp_map_best and haf_cell_pose on re-voted grids, with a frame of points at cell centres: identical grids
    in all rolls (the first roll wins every tie), grids whose best votes are negative, masks, min_vote at its default and at -1000"""
    eng, gi = engines(N)
    frame, img = cell_centre_frame(N)
    in_kw = dict(grasp_area_length_x=min(N - 2, 60), grasp_area_length_y=min(N - 2, 60))
    Ms = rc.oracle_transforms(dict(grid_h=N, grid_w=N, n_rolls=R), in_kw, 0, R)
    words = fc.mirror_points(frame, img)
    zeros9 = np.zeros((N, N), np.int8)
    zeros9[::3] = -9                                         # every third row -9: the rows between vote -9 x their taps into those rows, nothing scores above 0
    assert vc.vote_int(zeros9).max() == 0 and vc.vote_int(zeros9).min() < 0
    batches = [("identical", [vc.random_grids(N)[8].grid] * 4), ("negative best", [vc.negative(N)[2].grid, zeros9, np.roll(zeros9, 1, axis=0), zeros9.T.copy()]),
               ("mixed", [vc.ranking(N)[0].grid, vc.ties(N)[0].grid, vc.random_grids(N)[4].grid, vc.negative(N)[1].grid])]
    h = heights_for(N, 2)
    rng = np.random.RandomState(3)
    for name, grids in batches:
        rec = eng.revote(labels=stack(grids + grids[::-1], np.int8), heights=stack([h] * 8, F))
        for b in range(B):
            mine = (grids + grids[::-1])[b * R:(b + 1) * R]
            fetched = np.stack([eng.roll_grid(b, r)[0] for r in range(R)])
            assert (fetched == np.stack([vc.vote_int(g) for g in mine]).astype(F)).all()
            got = eng.grasp_map(b, frame)
            ref = capi.grasp_map_ref(eng.cfg, gi, 0, fetched, frame)
            for k in ("vote", "roll", "cell"):
                assert (got[k] == ref[k]).all(), (name, b, k, int((got[k] != ref[k]).sum()))
            want = gm.mirror_map(Ms, fetched, 0, words, N, N)
            gm.assert_map_equal(got, want, (name, b))
            vote, roll, cell = got["vote"], got["roll"], got["cell"]
            assert (roll >= 0).sum() > N * N // 2
            if name == "identical":                          # equal votes in several rolls: the first of them is kept
                per_roll = np.stack([gm.mirror_map(Ms[r:r + 1], fetched[r:r + 1], r, words, N, N)[0] for r in range(R)]).astype(np.int64)
                tied = ((per_roll == per_roll.max(axis=0)).sum(axis=0) > 1) & (per_roll.max(axis=0) > gm.NO_CELL)
                assert tied.sum() > 100 and (roll.reshape(-1)[tied] == per_roll.argmax(axis=0)[tied]).all()
            if name == "negative best":
                assert vote[roll >= 0].max() <= 0 and (vote[roll >= 0] < 0).sum() > 50
            masks = [None, (rng.uniform(size=(N, N)) < 0.3).astype(np.uint8), ((vote < 0) & (roll >= 0)).astype(np.uint8) * 7,
                     np.zeros((N, N), np.uint8)]
            for mask in masks:
                for min_vote in (1, -1000):
                    w = gm.key_argmax(vote, roll, mask, min_vote)
                    g = eng.best_in_mask(b, frame, mask, min_vote)
                    assert (g is None) == (w is None), (name, b, min_vote)
                    if w is None:
                        continue
                    c, u, v = g
                    assert (u, v) == w, (name, b, min_vote, (u, v), w)
                    assert (c["best_vote"], c["best_roll"], c["best_row"] * N + c["best_col"]) == (int(vote[v, u]), int(roll[v, u]), int(cell[v, u]))
                    assert c == eng.cell_pose(b, int(roll[v, u]), int(cell[v, u]) // N, int(cell[v, u]) % N)
            neg = ((vote < 0) & (roll >= 0)).astype(np.uint8)
            if neg.any():                                    # under a mask of negative pixels only min_vote = -1000 finds one
                assert eng.best_in_mask(b, frame, neg, 1) is None and eng.best_in_mask(b, frame, neg, -1000)[0]["best_vote"] < 0
            # haf_cell_pose of the winner is rank 1 of haf_top_grasps; at the grid's corners it is the cell's own vote and clipped window
            top = eng.top_grasps(k=1, min_vote=1)[b]
            if top:
                t = top[0]
                c = eng.cell_pose(b, t["best_roll"], t["best_row"], t["best_col"])
                for f in t:
                    if f != "run_length":
                        assert np.array(c[f]).tobytes() == np.array(t[f]).tobytes(), (name, b, f)
                best = max(range(R), key=lambda r: (int(rec["vote"][b, r]), -r))
                assert (t["best_roll"], t["best_row"], t["best_col"], t["best_vote"]) == \
                    (best, int(rec["row"][b, best]), int(rec["col"][b, best]), int(rec["vote"][b, best]))
            for r, (row, col) in enumerate(((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1))):
                c = eng.cell_pose(b, r, row, col)
                assert (c["best_vote"], c["best_row"], c["best_col"], c["best_roll"]) == (0, row, col, r)
                assert _bits(c["h_locmax"]) == _bits(vc.z_key(h, row, col))
            row, col = N // 2, N // 2
            c = eng.cell_pose(b, 1, row, col)
            assert c["best_vote"] == int(fetched[1][row, col]) and _bits(c["h_locmax"]) == _bits(vc.z_key(h, row, col))


def test_revote_refusals(engines, data_dir, golden_dir):
    """any state other than a scored batch of the hook's kind is HAF_E_ARG"""
    eng, gi = engines(15)
    lab = np.full((B, R, 15, 15), -1, np.int8)
    for kw in (dict(), dict(heights=lab.astype(F)), dict(labels=lab, gridf=lab.astype(F)), dict(gridf=lab.astype(F))):
        with pytest.raises(capi.HafError) as ei:
            eng.revote(**kw)
        assert ei.value.code == capi.HAF_E_ARG
    with pytest.raises(capi.HafError) as ei:                 # the hook's own refusal of the same, behind the wrapper's
        eng._check(eng._L.haf_test_revote(eng._h, None, None, None, None, None))
    assert ei.value.code == capi.HAF_E_ARG
    f, r = _files(data_dir)
    fresh = capi.Engine(f, r, os.path.join(golden_dir, "surrogate.model"), testing=True, grid_h=15, grid_w=15, n_rolls=R, max_clouds=B, max_points=1 << 10)
    with pytest.raises(capi.HafError) as ei:
        fresh.revote(labels=lab)
    assert ei.value.code == capi.HAF_E_ARG and "no scored batch" in str(ei.value)
    with pytest.raises(capi.HafError) as ei:                 # nothing scored and nothing given: still the wrapper's refusal
        fresh.revote()
    assert ei.value.code == capi.HAF_E_ARG
    fresh.close()
    # arrays that are not the last batch's B x R grids are refused before the hook reads them
    for kw in (dict(labels=lab[:1]), dict(labels=lab[:, :2]), dict(labels=lab, heights=np.zeros((B, R, 15, 14), F)),
               dict(labels=lab, roi_words=np.zeros((B, 1, 15, 1), np.uint64))):
        with pytest.raises(capi.HafError) as ei:
            eng.revote(**kw)
        assert ei.value.code == capi.HAF_E_ARG and "last batch" in str(ei.value)
    # the engine still serves requests, and what a request leaves does not depend on the re-votes before it
    before = eng.score_batch([TINY, TINY], [gi, gi])
    grids = [eng.roll_grid(b, r)[0] for b in range(B) for r in range(R)]
    rec = eng.revote(labels=np.full((B, R, 15, 15), 99, np.int8))
    assert (rec["vote"] == 12177).all() and any((eng.roll_grid(b, r)[0] != grids[b * R + r]).any() for b in range(B) for r in range(R))
    assert eng.score_batch([TINY, TINY], [gi, gi]) == before
    assert all((eng.roll_grid(b, r)[0] == grids[b * R + r]).all() for b in range(B) for r in range(R))


# ---- models whose labels are not +-1 ----

def _label_request(N, data_dir):
    rq = vc.LABEL_REQUESTS[N]
    xyz = pcdio.load_pcd(os.path.join(data_dir, "pcd2.pcd")) if N == 56 else models.synthetic_cloud(grid=136)
    return rq, xyz


def _label_engine(data_dir, path, rq, flags=0, **kw):
    f, r = _files(data_dir)
    return capi.Engine(f, r, path, testing=True, flags=capi.FLAG_KEEP_DEBUG | capi.FLAG_PROFILE | flags, max_points=1 << 17, **dict(rq["cfg"], **kw))


LABEL_MODES = {(0, 1): capi.FLAG_SPLIT_F16, (99, -9): capi.FLAG_FP32_MFMA}      # one pair each additionally in the other contraction modes


@pytest.mark.parametrize("pair", list(vc.LABEL_PAIRS), ids=lambda p: "%d_%d" % p)
@pytest.mark.parametrize("N", (56, 136))
def test_label_pairs_against_the_oracle(data_dir, tmp_path, N, pair):
    """compare_full through a balanced random model with `label a b`: the label grid holds the pair's grid values, the vote grids, the
    records and the grasp are the oracle's.  An engine that could not serve a pair would have to refuse it at haf_create."""
    rq, xyz = _label_request(N, data_dir)
    path = models.write_random_model(str(tmp_path / "m.model"), vc.LABEL_NSV, seed=rq["seed"], balanced=True, labels=pair)
    f, r = _files(data_dir)
    o = O.Oracle(f, r, path)
    ga, gb = vc.LABEL_PAIRS[pair]
    for flags in [0] + ([LABEL_MODES[pair]] if pair in LABEL_MODES else []):
        eng = _label_engine(data_dir, path, rq, flags)
        got, want = compare_full(eng, o, xyz, rq["cfg"], rq["inp"])
        m = want["mask"] == 1
        assert ((want["labels"][m] == ga).sum() > 50) and ((want["labels"][m] == gb).sum() > 50) and (want["labels"][~m] == -1).all()
        eng.close()


@pytest.mark.parametrize("pair", [(1, 0), (99, -9)], ids=lambda p: "%d_%d" % p)
@pytest.mark.parametrize("N", (56, 136))
def test_label_pairs_ranking_maps_and_roi(data_dir, tmp_path, N, pair):
    """`label 1 0` and `label 99 -9` (votes of the negative class, negative votes, votes up to 12 177) through haf_top_grasps against its
    mirror, haf_grasp_map against haf_grasp_map_ref, and haf_score_frames_roi against the full request restricted to the mask"""
    rq, xyz = _label_request(N, data_dir)
    path = models.write_random_model(str(tmp_path / "m.model"), vc.LABEL_NSV, seed=rq["seed"], balanced=True, labels=pair)
    eng = _label_engine(data_dir, path, rq)
    Rn = rq["cfg"]["n_rolls"]
    img = gm.organised(xyz, width=256)
    frame = capi.xyz_frame(img)
    inp = capi.default_input(**rq["inp"])
    full_out = eng.score_frames([frame], [inp])[0]
    fm = np.stack([eng.debug(capi.DBG_MASK, 0, r) for r in range(Rn)])
    fl = np.stack([eng.debug(capi.DBG_LABELS, 0, r) for r in range(Rn)])
    fh = np.stack([eng.debug(capi.DBG_HEIGHTS, 0, r) for r in range(Rn)])
    fv = np.stack([eng.roll_grid(0, r)[0] for r in range(Rn)])
    ga, gb = vc.LABEL_PAIRS[pair]
    assert (fl[fm != 0] == ga).sum() > 50 and (fl[fm != 0] == gb).sum() > 50
    assert all((fv[r] == vc.vote_int(fl[r]).astype(F)).all() for r in range(Rn))
    if pair == (1, 0):
        assert (fv[fl == 0] > 0).any()                       # cells of the negative class score
    else:
        assert fv.max() > 123                                # votes above what +-1 labels can reach
    rec = eng.score_rolls([xyz], [inp], 0, Rn)
    for params in (dict(), dict(k=1024, cell_radius=0, min_vote=1), dict(k=16, roll_window=0)):
        got = eng.top_grasps(**params)
        assert_same(got[0], mirror(eng, inp, 0, 0, Rn, rec["n_evals"][0], **params), (N, pair, params))
    assert len(eng.top_grasps(k=16, min_vote=1)[0]) > 0
    eng.score_frames([frame], [inp])
    m = eng.grasp_map(0, frame)
    ref = capi.grasp_map_ref(eng.cfg, inp, 0, fv, frame)
    for k in ("vote", "roll", "cell"):
        assert (m[k] == ref[k]).all(), (N, pair, k)
    # the ROI request is the full request restricted to the mask
    words = fc.mirror_points(frame, img)
    Ms = rc.oracle_transforms(rq["cfg"], rq["inp"], 0, Rn)
    bu, bv = gm.key_argmax(m["vote"], m["roll"], None, 1)
    hh, ww = m["vote"].shape
    for name, mask in rc.masks(words, hh, ww, rect=(max(0, bv - 12), min(hh, bv + 12), max(0, bu - 40), min(ww, bu + 40)))[:3]:
        want = expected(eng, inp, Ms, words, mask, fm, fl, fv, fh)
        got = eng.score_frames_roi([frame], [mask], [inp])[0]
        check_roi_state(eng, 0, got, want, (N, pair, name))
        assert want[1].sum() > 0
    eng.close()


def test_probability_model_with_labels_0_1(data_dir, tmp_path):
    """a probability model with `label 0 1` against the oracle, in the pattern of test_probability_mode_against_oracle"""
    base = models.write_random_model(str(tmp_path / "b.model"), vc.LABEL_NSV, seed=vc.LABEL_REQUESTS[56]["seed"], balanced=True, labels=(0, 1))
    mp = models.write_probability_model(str(tmp_path / "p.model"), base, "-3.5", "0.25")
    f, r = _files(data_dir)
    o = O.Oracle(f, r, mp)
    eng = capi.Engine(f, r, mp, testing=True, flags=capi.FLAG_KEEP_DEBUG | capi.FLAG_PROFILE | capi.FLAG_PROBABILITY, n_rolls=4, max_points=1 << 17)
    xyz = pcdio.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    got, want = compare_probability(eng, o, xyz, dict(n_rolls=4), dict(grasp_area_length_x=32, grasp_area_length_y=44))
    m = want["mask"] == 1
    assert (want["labels"][m] == 0).sum() > 50 and (want["labels"][m] == 1).sum() > 50 and (want["graspsgrid"] > 0).any()
    compare_probability(eng, o, xyz, dict(n_rolls=4), dict(grasp_area_length_x=32, grasp_area_length_y=32, approach_vector=(0.2, -0.1, 1.0)))
    eng.close()
