"""haf_top_grasps on the MI355X against a numpy mirror of its contract (include/hafgrasp.h, steps 1-6), built from the engine's own
oracle-pinned grids of the last scored batch: votes from haf_get_roll_grid, heights from haf_debug_fetch(HEIGHTS), poses from
haf_roll_pose on a synthesised record array."""
import ctypes as C
import os

import numpy as np
import pytest

import models
from haf_grasping_amd import capi
from top_grasps_cases import POSE, assert_same, mirror

pytestmark = pytest.mark.gpu

PCDS = ["pcd%d" % i for i in range(1, 13)]
TABLES = ["table1_mult_obj_rcs_1428580506606673", "table2_mult_obj_rcs_1428580941635676", "table3_mult_obj_rcs_1428581033679923"]
PARAM_SETS = [dict(), dict(k=1), dict(k=1024), dict(cell_radius=0, k=64), dict(cell_radius=40, k=64), dict(roll_window=0, k=64),
              dict(roll_window=3, min_dist_m=0.05, k=64), dict(min_vote=1, k=32), dict(min_vote=30000)]


def _files(data_dir):
    return os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")


def _engine(data_dir, model, testing=False, **cfg):
    f, r = _files(data_dir)
    cfg.setdefault("flags", capi.FLAG_KEEP_DEBUG)
    return capi.Engine(f, r, model, testing=testing, **cfg)


def _check(eng, gi, rec, params, ctx, roll_first=0):
    got = eng.top_grasps(**params)
    R = rec.shape[-1]
    rec = rec.reshape(-1, R)
    assert len(got) == len(gi)
    for b in range(len(gi)):
        want = mirror(eng, gi[b], b, roll_first, R, rec["n_evals"][b], **params)
        assert_same(got[b], want, (ctx, b, params))
    return got


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


def test_pcd_files_against_mirror(data_dir, surrogate):
    eng = _engine(data_dir, surrogate, max_points=1 << 18)
    for name in PCDS:
        xyz = capi.load_pcd(os.path.join(data_dir, name + ".pcd"))
        gi = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44)
        rec = eng.score_rolls([xyz], [gi], 0, 12)
        for params in PARAM_SETS:
            got = _check(eng, [gi], rec, params, name)
            if params.get("min_vote") == 30000:
                assert got == [[]]
    eng.close()


def test_tabletop_clouds_against_mirror(data_dir, surrogate):
    eng = _engine(data_dir, surrogate, n_rolls=20, roll_step_deg=9, max_points=1 << 18)
    for name in TABLES:
        xyz = capi.load_pcd(os.path.join(data_dir, name + ".pcd"))
        gi = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
        rec = eng.score_rolls([xyz], [gi], 0, 20)
        for params in PARAM_SETS:
            _check(eng, [gi], rec, params, name)
    eng.close()


def test_full_size_c5_against_mirror(data_dir, tmp_path, monkeypatch):
    """512 x 512, 36 rolls of 5 degrees (circular), random 256-SV model; guard zones intact under HAF_CANARY_CHECK"""
    path = str(tmp_path / "rand256.model")
    models.write_random_model(path, 256, seed=4, balanced=True)
    xyz = models.synthetic_cloud(grid=512, k=2, seed=0)
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    eng = _engine(data_dir, path, testing=True, grid_h=512, grid_w=512, n_rolls=36, roll_step_deg=5, max_points=1 << 20)
    gi = capi.default_input(grasp_area_length_x=512, grasp_area_length_y=512)
    rec = eng.score_rolls([xyz], [gi], 0, 36)
    for params in (dict(k=32), dict(k=200, roll_window=2, min_dist_m=0.05), dict(k=64, cell_radius=0)):
        _check(eng, [gi], rec, params, "C5")
    bad, msg, nbuf = capi.check_canaries()
    assert bad == 0 and nbuf > 0, msg
    eng.close()


def test_rank_one_is_the_best_grasp(data_dir, surrogate):
    eng = _engine(data_dir, surrogate, max_points=1 << 18)
    for name in PCDS:
        xyz = capi.load_pcd(os.path.join(data_dir, name + ".pcd"))
        gi = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44)
        best = eng.score(xyz, gi)
        top = eng.top_grasps(min_vote=1, k=4)[0]
        if best["best_vote"] < 1:
            assert top == []
            continue
        t = top[0]
        for f in ("best_row", "best_col", "best_roll", "best_vote", "eval"):
            assert t[f] == best[f], (name, f)
        for f in POSE:
            assert np.array(t[f]).tobytes() == np.array(best[f]).tobytes(), (name, f)
        assert np.float32(t["roll"]).tobytes() == np.float32(best["roll"]).tobytes()
    eng.close()


def test_every_roll_record_is_a_candidate(data_dir, surrogate):
    eng = _engine(data_dir, surrogate, max_points=1 << 18)
    for name in ("pcd2", "pcd3", "pcd12"):
        xyz = capi.load_pcd(os.path.join(data_dir, name + ".pcd"))
        gi = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44)
        rec = eng.score_rolls([xyz], [gi], 0, 12)[0]
        top = eng.top_grasps(k=1024, roll_window=0)[0]
        by = {(t["best_roll"], t["best_row"], t["best_col"]): t for t in top}
        for r in range(12):
            if rec["vote"][r] < 71:
                continue
            t = by[(r, int(rec["row"][r]), int(rec["col"][r]))]
            assert t["best_vote"] == rec["vote"][r] and np.float32(t["h_locmax"]) == rec["h_locmax"][r]
            rp, _ = eng.roll_pose(gi, rec, r)
            for f in POSE:
                assert tuple(t[f]) == tuple(rp[f]), (name, r, f)
            assert (t["roll"], t["rolls_done"], t["n_evals"]) == (rp["roll"], rp["rolls_done"], rp["n_evals"])
            assert t["eval"] == rec["vote"][r] - 20
    eng.close()


def test_plateaus(data_dir, tmp_path):
    """rho = -1e4: every masked cell is labelled 1 (wide equal-vote runs: tie order and in-roll suppression); rho = +1e4: none"""
    xyz = capi.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    gi = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44)
    for rho, label in ((-1e4, 1), (1e4, -1)):
        path = str(tmp_path / ("plateau%d.model" % (rho > 0)))
        models.write_random_model(path, 256, rho=rho, seed=3)
        eng = _engine(data_dir, path, max_points=1 << 18)
        rec = eng.score_rolls([xyz], [gi], 0, 12)
        for r in range(12):
            lab = eng.debug(capi.DBG_LABELS, 0, r)
            mask = eng.debug(capi.DBG_MASK, 0, r)
            assert mask.any() and (lab[mask != 0] == label).all()
        for params in (dict(k=64), dict(k=64, cell_radius=0), dict(k=16, cell_radius=3, min_vote=1)):
            got = _check(eng, [gi], rec, params, "plateau")
            if label < 0:
                assert got == [[]]
        eng.close()


def test_depth_rerun_gives_the_same_result(data_dir, surrogate, monkeypatch):
    xyz = capi.load_pcd(os.path.join(data_dir, "pcd3.pcd"))
    gi = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44)
    eng = _engine(data_dir, surrogate, testing=True, max_points=1 << 18)
    eng.score_rolls([xyz], [gi], 0, 12)
    params = [dict(k=64, roll_window=6, min_dist_m=0.2), dict(k=8), dict(k=200, cell_radius=1)]
    ref = [eng.top_grasps(**p) for p in params]
    monkeypatch.setenv("HAF_TOP_DEPTH", "1")
    assert [eng.top_grasps(**p) for p in params] == ref
    eng.close()


def test_batch_subrange_determinism_and_state(data_dir, surrogate):
    names = ["pcd%d" % i for i in range(1, 9)]
    clouds = [capi.load_pcd(os.path.join(data_dir, n + ".pcd")) for n in names]
    inputs = [capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44) for _ in names]
    inputs[6] = capi.default_input(grasp_area_center=(0.30, 0.46, 0.0))
    eng = _engine(data_dir, surrogate, n_rolls=20, roll_step_deg=9, max_clouds=8, max_points=1 << 20)
    eng.score_batch(clouds, inputs)
    batch = eng.top_grasps(k=16)
    assert len(batch) == 8
    for b in range(8):
        eng.score(clouds[b], inputs[b])
        assert eng.top_grasps(k=16) == [batch[b]], b
    # a roll sub-range carries global roll indices
    rec = eng.score_rolls(clouds[:2], inputs[:2], 7, 6)
    got = _check(eng, inputs[:2], rec, dict(k=40), "subrange", roll_first=7)
    assert all(7 <= t["best_roll"] < 13 for c in got for t in c) and any(got)
    # two calls: identical; records, grids and counters unchanged
    grids = [eng.roll_grid(c, r)[0] for c in range(2) for r in range(7, 13)]
    counts = eng.last_counts()
    again = eng.top_grasps(k=40)
    assert again == got
    assert [eng.roll_grid(c, r)[0].tobytes() for c in range(2) for r in range(7, 13)] == [g.tobytes() for g in grids]
    assert eng.last_counts() == counts
    # a following request gives what a fresh engine gives
    after = eng.score(clouds[2], inputs[2])
    fresh = _engine(data_dir, surrogate, n_rolls=20, roll_step_deg=9, max_clouds=8, max_points=1 << 20)
    assert fresh.score(clouds[2], inputs[2]) == after
    assert fresh.top_grasps(k=16) == eng.top_grasps(k=16)
    fresh.close()
    eng.close()


def test_error_paths(data_dir, surrogate, golden_dir, tmp_path):
    xyz = capi.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    gi = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44)
    eng = _engine(data_dir, surrogate, max_clouds=2, max_points=1 << 18)
    with pytest.raises(capi.HafError) as ei:
        eng.top_grasps()
    assert ei.value.code == capi.HAF_E_ARG and "no scored batch" in str(ei.value)
    eng.score(xyz, gi)
    for bad, word in ((dict(k=0), "k "), (dict(k=1025), "k "), (dict(min_vote=0), "min_vote"), (dict(cell_radius=-1), "cell_radius"),
                      (dict(roll_window=-1), "roll_window"), (dict(min_dist_m=-0.1), "min_dist_m"), (dict(min_dist_m=float("nan")), "min_dist_m")):
        with pytest.raises(capi.HafError) as ei:
            eng.top_grasps(**bad)
        assert ei.value.code == capi.HAF_E_ARG and word in str(ei.value), bad
    # a cloud with a negative budget next to a normal one: no candidates for it
    neg = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=44, max_calculation_time=-1.0)
    eng.score_batch([xyz, xyz], [gi, neg])
    got = eng.top_grasps(k=8)
    assert len(got) == 2 and len(got[0]) > 0 and got[1] == []
    eng.close()
    # probability mode
    f, r = _files(data_dir)
    import json
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as fh:
        pj = json.load(fh)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    prob = capi.Engine(f, r, mp, flags=capi.FLAG_PROBABILITY, max_points=1 << 18)
    prob.score(xyz, gi)
    with pytest.raises(capi.HafError) as ei:
        prob.top_grasps()
    assert ei.value.code == capi.HAF_E_ARG and "PROBABILITY" in str(ei.value)
    prob.close()


def test_server_and_cli(data_dir, surrogate, tmp_path):
    import subprocess
    from haf_grasping_amd import server
    f, r = _files(data_dir)
    xyz = capi.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    srv = server.CalcGraspPointsServer(f, r, surrogate)
    goal = server.GraspInputMsg(input_pc=xyz, grasp_area_length_x=32, grasp_area_length_y=44)
    res = srv.execute(goal)
    top = srv.top_grasps(k=5, min_vote=1)
    assert top and top[0].hypothesis_string() == res.hypothesis_string()
    cli = os.path.join(os.path.dirname(capi.__file__), "haf_grasp_cli")
    base = [cli, "--features", f, "--range", r, "--model", surrogate, "--search-size", "18", "30"]
    plain = subprocess.run(base + [os.path.join(data_dir, "pcd2.pcd")], capture_output=True, text=True, check=True).stdout
    withk = subprocess.run(base + ["--top-k", "5", "--top-radius", "7", "--top-rolls", "1", "--top-dist", "0.02",
                                   os.path.join(data_dir, "pcd2.pcd")], capture_output=True, text=True, check=True).stdout
    assert withk.startswith(plain)
    extra = withk[len(plain):].splitlines()
    want = srv.top_grasps(k=5)
    assert len(extra) == len(want) > 0
    assert all(l.startswith("top %d " % (i + 1)) for i, l in enumerate(extra))
    if want[0].eval == res.eval:                     # rank 1 is the goal's own result when its vote reaches min_vote
        assert extra[0] == "top 1 " + plain.splitlines()[-1]
    srv.close()
