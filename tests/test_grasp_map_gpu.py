"""Per-pixel grasp maps on the MI355X (include/hafgrasp.h: haf_grasp_map, haf_cell_pose, haf_grasp_map_best; csrc/graspmap.hip).
The device map against haf_grasp_map_ref on the engine's own roll grids and against the numpy mirror on the CPU oracle's transforms and
vote grids, every pixel of all three images; state preservation; haf_cell_pose against haf_top_grasps and haf_score; the masked best
against the key-order argmax over the returned map; the engine-side refusals; the CLI.  Every comparison is an equality.
Testing build throughout; the guard zones around every device buffer are checked after each test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import models
import pcdio
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import compare_full, oracle_input
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, _files, device_copy, kernel_cases, make_engine, render_depth, snapshot
from test_grasp_map_cpu import scene_frames
from test_views_gpu import CAM_A, CAM_B

pytestmark = pytest.mark.gpu

H = W = 56
POSE = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector")


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(scope="module")
def orc(data_dir, surrogate):
    f, r = _files(data_dir)
    return O.Oracle(f, r, surrogate)


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")          # every map call checks the guard zones itself, too
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


def oracle_transforms(cfg_kw, in_kw, roll_first, count):
    """the CPU oracle's own 4x4 roll transforms (hafo_transform): [count, 16] float32"""
    ocfg = O.make_cfg(**{k: v for k, v in cfg_kw.items() if k in ("n_rolls", "roll_step_deg")}, H=cfg_kw.get("grid_h", 56), W=cfg_kw.get("grid_w", 56))
    oin = oracle_input(in_kw)
    out = np.zeros((count, 16), np.float32)
    for r in range(count):
        O.lib().hafo_transform(C.byref(ocfg), C.byref(oin), roll_first + r, 0, out[r].ctypes.data)
    return out


def engine_grids(eng, request, roll_first, count):
    return np.stack([eng.roll_grid(request, roll_first + r)[0] for r in range(count)])


def device_images(n, misalign=0):
    """three device buffers for packed images of n pixels, `misalign` elements past a 256-byte boundary -> (dict of pointers, reader)"""
    import torch
    tv = torch.full((n + 16,), 12345, dtype=torch.int16, device="cuda")
    tr = torch.full((n + 16,), 12345, dtype=torch.int16, device="cuda")
    tc = torch.full((n + 16,), 12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = dict(vote=tv.data_ptr() + 2 * misalign, roll=tr.data_ptr() + 2 * misalign, cell=tc.data_ptr() + 4 * misalign)

    def read(shape):
        torch.cuda.synchronize()
        out = {}
        for k, t in (("vote", tv), ("roll", tr), ("cell", tc)):
            a = t.cpu().numpy()
            assert (a[:misalign] == 12345).all() and (a[misalign + n:] == 12345).all(), k      # nothing outside the image
            out[k] = a[misalign:misalign + n].reshape(shape)
        return out
    return ptr, read


def check_map(eng, request, inp, roll_first, count, host_frame, img, want_ms, want_grids, name, use=None, device_out=None):
    """haf_grasp_map == haf_grasp_map_ref on the engine's grids == the mirror on (want_ms, want_grids) -> the map"""
    got = eng.grasp_map(request, use if use is not None else host_frame)
    ref = capi.grasp_map_ref(eng.cfg, inp, roll_first, engine_grids(eng, request, roll_first, count), host_frame)
    for k in ("vote", "roll", "cell"):
        bad = np.flatnonzero(got[k].reshape(-1) != ref[k].reshape(-1))
        assert bad.size == 0, (name, k, bad.size, bad[:5], got[k].reshape(-1)[bad[:5]], ref[k].reshape(-1)[bad[:5]])
    want = gm.mirror_map(want_ms, want_grids, roll_first, fc.mirror_points(host_frame, img), eng.cfg.grid_h, eng.cfg.grid_w)
    gm.assert_map_equal(got, want, name)
    if device_out is not None:
        n = host_frame.width * host_frame.height
        ptr, read = device_images(n, device_out)
        assert eng.grasp_map(request, use if use is not None else host_frame, device_out=ptr) is None
        dev = read((host_frame.height, host_frame.width))
        for k in ("vote", "roll", "cell"):
            assert (dev[k] == got[k]).all(), (name, "device outputs", k)
    return got


def test_map_equals_host_definition_and_oracle_in_every_pixel(data_dir, surrogate, orc, table1):
    """table1 at C3 (56 x 56, 20 rolls), scored as a cloud and pinned to the oracle by compare_full.  Then every frame of kernel_cases()
    (all kinds and shapes, padded rows, 640 x 480 one element off a 16-byte boundary, widths 1..17) and the golden scene's own frames
    (grasp-map CPU suite), host- and device-resident, host and device outputs (aligned and one element off): the device map equals
    haf_grasp_map_ref on the engine's haf_get_roll_grid grids and the numpy mirror on the oracle's M and graspseval.  Mapping a frame that
    was never scored is the normal case here: none of them was."""
    eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    got, want = compare_full(eng, orc, table1, C3_CFG, C3_IN)
    assert got["n_evals"] >= 20000 and got["eval"] > 50
    ms = oracle_transforms(C3_CFG, C3_IN, 0, 20)
    assert (ms.view(np.uint32) == want["M"].view(np.uint32)).all()
    seen, kinds, with_cell = 0, 0, 0
    for k, (name, frame, img) in enumerate(scene_frames(table1) + kernel_cases()):
        host = check_map(eng, 0, inp, 0, 20, frame, img, want["M"], want["graspseval"], name + "/host", device_out=k % 2)
        dev = check_map(eng, 0, inp, 0, 20, frame, img, want["M"], want["graspseval"], name + "/device", use=device_copy(frame, img), device_out=(k + 1) % 2)
        assert all((host[f] == dev[f]).all() for f in ("vote", "roll", "cell"))
        seen += 1
        kinds |= 1 << frame.kind
        with_cell += int((host["roll"] >= 0).sum())
        for keep in ("vote", "roll", "cell"):                                    # any output may be left out
            part = eng.grasp_map(0, frame, want=(keep,))
            assert list(part) == [keep] and (part[keep] == host[keep]).all(), (name, keep)
    assert seen >= 10 + 28 + 2 + 51 and kinds == 7 and with_cell >= 300000
    eng.close()


def test_big_grid_subrange_batch_and_unscored_camera(data_dir, surrogate, orc, tmp_path, table1):
    """(a) a 512 x 512 / 36-roll engine on the synthetic C5 cloud, random 256-SV model: the map of a rendered view against
    haf_grasp_map_ref and against the mirror on the ORACLE's transforms (hafo_transform) and the engine's vote grids -- the CPU oracle
    cannot score 9.4 M evaluations in a test's time; the engine's grids at this size are pinned to it elsewhere (test_engine_gpu);
    (b) a haf_score_rolls sub-range: global roll indices 7..12; (c) a batch of three requests with different inputs, mapped one after
    another, one of them with a negative budget (no roll ran: HAF_MAP_NO_CELL everywhere); (d) after haf_score_frames on camera A's
    image, the map of camera B's image, which was never scored."""
    path = str(tmp_path / "rand256.model")
    models.write_random_model(path, 256, seed=4, balanced=True)
    xyz = models.synthetic_cloud(grid=512, k=2, seed=0)
    big_cfg = dict(grid_h=512, grid_w=512, n_rolls=36, roll_step_deg=5)
    big_in = dict(grasp_area_length_x=512, grasp_area_length_y=512)
    cam = np.array([1, 0, 0, 0.0, 0, -1, 0, 0.0, 0, 0, -1, 4.0], np.float32)     # straight down from 4 m: the whole 5 m grid is far wider than the view
    depth = render_depth(xyz, cam)
    frame = capi.depth_frame(depth, sensor_to_base=cam, **K525)
    eng = make_engine(data_dir, path, max_points=1 << 20, **big_cfg)
    inp = capi.default_input(**big_in)
    out = eng.score(xyz, inp)
    assert out["n_evals"] > 1000000
    grids = engine_grids(eng, 0, 0, 36)
    big = check_map(eng, 0, inp, 0, 36, frame, depth, oracle_transforms(big_cfg, big_in, 0, 36), grids, "c5", device_out=0)
    assert (big["roll"] >= 0).sum() >= 100000 and (big["vote"] > 0).any()    # (217 044 pixels of the view carry a depth; roll 0's grid holds them all)
    check_map(eng, 0, inp, 0, 36, frame, depth, oracle_transforms(big_cfg, big_in, 0, 36), grids, "c5/device", use=device_copy(frame, depth))
    eng.close()

    eng = make_engine(data_dir, surrogate, max_clouds=3, max_points=3 * 640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    scene = orc.run(table1, O.make_cfg(**C3_CFG), oracle_input(C3_IN))
    da, db = render_depth(table1, CAM_A), render_depth(table1, CAM_B)
    fa, fb = capi.depth_frame(da, sensor_to_base=CAM_A, **K525), capi.depth_frame(db, sensor_to_base=CAM_B, **K525)
    # (b)
    eng.score_rolls([table1], [inp], 7, 6)
    sub = check_map(eng, 0, inp, 7, 6, fa, da, scene["M"][7:13], scene["graspseval"][7:13], "subrange", device_out=1)
    assert set(np.unique(sub["roll"])) <= set(range(7, 13)) | {-1} and (sub["roll"] >= 7).sum() >= 10000
    # (c)
    ins = [C3_IN, dict(C3_IN, approach_vector=(0.1, -0.1, 1.0), gripper_opening_width=2), dict(C3_IN, grasp_area_center=(0.10, 0.20, 0.0))]
    inputs = [capi.default_input(**kw) for kw in ins]
    eng.score_batch([table1] * 3, inputs)
    maps = []
    for b in range(3):
        want = scene if b == 0 else orc.run(table1, O.make_cfg(**C3_CFG), oracle_input(ins[b]))
        maps.append(check_map(eng, b, inputs[b], 0, 20, fa, da, want["M"], want["graspseval"], "batch %d" % b, use=device_copy(fa, da) if b == 1 else None))
        assert (maps[b]["vote"] > 0).sum() >= 3000, b
    assert any((maps[0][k] != maps[b][k]).any() for b in (1, 2) for k in ("vote", "roll", "cell"))
    neg = capi.default_input(max_calculation_time=-1.0, **C3_IN)
    eng.score_batch([table1, table1], [neg, inp])
    none = eng.grasp_map(0, fa)
    assert (none["vote"] == gm.NO_CELL).all() and (none["roll"] == -1).all() and (none["cell"] == -1).all()
    check_map(eng, 1, inp, 0, 20, fa, da, scene["M"], scene["graspseval"], "next to a negative budget")
    with pytest.raises(capi.HafError) as ei:
        eng.cell_pose(0, 0, 10, 10)
    assert ei.value.code == capi.HAF_E_ARG
    # (d)
    pts = capi.frame_points(fa)
    got = eng.score_frames([fa], [inp])[0]
    want = orc.run(pts, O.make_cfg(**C3_CFG), oracle_input(C3_IN))
    assert got["n_evals"] == want["n_evals"] >= 20000 and got["best_vote"] == want["top"]
    other = check_map(eng, 0, inp, 0, 20, fb, db, want["M"], want["graspseval"], "unscored camera", device_out=0)
    own = check_map(eng, 0, inp, 0, 20, fa, da, want["M"], want["graspseval"], "scored camera")
    assert (other["vote"] > 0).sum() >= 3000 and (own["vote"] > 0).sum() >= 3000 and own["vote"].max() == want["top"]
    eng.close()


def full_state(eng, out, n_clouds=1):
    s = snapshot(eng, out, n_clouds)
    s["prestage"], s["strict"], s["stage_ms"] = eng.last_prestage(), eng.last_strict_host(), eng.stage_ms()
    for b in range(n_clouds):
        s["points", b] = eng.debug_points(b).tobytes()
        for r in range(eng.cfg.n_rolls):
            s["dbg", b, r] = tuple(eng.debug(w, b, r).tobytes() for w in (capi.DBG_INTEGRAL, capi.DBG_MASK, capi.DBG_LABELS, capi.DBG_DECISION))
    return s


def test_map_calls_leave_the_last_batch_as_it_was(data_dir, surrogate, table1):
    """haf_top_grasps, haf_get_roll_grid, haf_last_* and haf_debug_fetch* return after map, cell-pose and masked-best calls -- host
    frames of every kind (their pixels are staged), device frames, host and device outputs -- what they returned before; the next
    request gives what it gives on a fresh engine"""
    da = render_depth(table1, CAM_A)
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    inp = capi.default_input(**C3_IN)
    for how in ("frames", "cloud"):
        eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
        out = eng.score_frames([fa], [inp])[0] if how == "frames" else eng.score(capi.view_points([fa]), inp)
        before = full_state(eng, out)
        for k, (name, frame, img) in enumerate(scene_frames(table1)[:7]):
            eng.grasp_map(0, frame)
            ptr, keep = device_images(frame.width * frame.height)
            eng.grasp_map(0, device_copy(frame, img), device_out=ptr)
            keep((frame.height, frame.width))
            assert eng.best_in_mask(0, frame, None, 1) is not None or k == 6          # (the single pixel need not carry a positive vote)
        eng.cell_pose(0, 3, 20, 30)
        after = full_state(eng, out)
        assert before.keys() == after.keys()
        for k in before:
            assert before[k] == after[k], (how, k)
        nxt = eng.score(table1, inp)
        fresh = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
        assert fresh.score(table1, inp) == nxt and fresh.top_grasps(k=16) == eng.top_grasps(k=16)
        fresh.close()
        eng.close()


def test_cell_pose_reproduces_top_grasps_and_the_best_grasp(data_dir, surrogate, orc, table1):
    """At the (roll, row, col) of each of the first 8 haf_top_grasps candidates haf_cell_pose gives that candidate's grasp and h_locmax
    exactly (run_length is 0: a cell is not a run); at rank 1 that is haf_score's output, which compare_full pins to the oracle.  Any
    other cell: the vote of the roll grid at the cell, eval = vote - 20."""
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=1 << 18, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    best, want = compare_full(eng, orc, table1, C3_CFG, C3_IN)
    top = eng.top_grasps(k=8)[0]
    assert len(top) == 8
    for rank, t in enumerate(top):
        c = eng.cell_pose(0, t["best_roll"], t["best_row"], t["best_col"])
        assert c["run_length"] == 0
        for f in t:
            if f != "run_length":
                assert np.array(c[f]).tobytes() == np.array(t[f]).tobytes(), (rank, f, c[f], t[f])
    first = eng.cell_pose(0, best["best_roll"], best["best_row"], best["best_col"])
    for f in POSE + ("roll", "eval", "best_row", "best_col", "best_roll", "best_vote"):       # (rolls_done and n_evals are the roll's own)
        assert np.array(first[f]).tobytes() == np.array(best[f]).tobytes(), (f, first[f], best[f])
    assert (first["eval"], first["best_row"], first["best_col"], first["best_roll"]) == (want["eval"], want["row"], want["col"], want["roll_idx"])
    rng = np.random.default_rng(5)
    for _ in range(16):
        roll, row, col = int(rng.integers(0, 20)), int(rng.integers(0, H)), int(rng.integers(0, W))
        c = eng.cell_pose(0, roll, row, col)
        vote = int(want["graspseval"][roll][row, col])
        assert (c["best_vote"], c["eval"], c["best_row"], c["best_col"], c["best_roll"], c["rolls_done"]) == (vote, vote - 20, row, col, roll, roll + 1)
    # the second request of a batch, on a roll sub-range
    rec = eng.score_rolls([table1, table1], [inp, inp], 7, 6)
    for b in range(2):
        for t in eng.top_grasps(k=4)[b]:
            c = eng.cell_pose(b, t["best_roll"], t["best_row"], t["best_col"])
            assert all(np.array(c[f]).tobytes() == np.array(t[f]).tobytes() for f in t if f != "run_length")
    eng.close()


def test_masked_best_is_the_key_order_argmax(data_dir, surrogate, table1):
    """haf_grasp_map_best == the argmax in key order (vote descending, roll, v, u ascending) computed in numpy over the returned map:
    no mask, a rectangle, a mask that selects nothing, a mask around the second-best object, a padded mask, min_vote above and at the
    best vote; its pose is haf_cell_pose of that pixel's (roll, cell)"""
    da = render_depth(table1, CAM_A)
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    eng.score_frames([fa], [inp])
    m = eng.grasp_map(0, fa)
    vote, roll, cell = m["vote"], m["roll"], m["cell"]
    assert (vote > 0).sum() >= 3000
    bu, bv = gm.key_argmax(vote, roll, None, 1)
    rect = np.zeros((480, 640), np.uint8)
    rect[100:300, 200:500] = 1
    # the second-best object: the best pixel further than 60 pixels from the best one, and a disc around it
    vv, uu = np.mgrid[0:480, 0:640]
    far = ((uu - bu) ** 2 + (vv - bv) ** 2 > 60 ** 2).astype(np.uint8)
    su, sv = gm.key_argmax(vote, roll, far, 1)
    second = (((uu - su) ** 2 + (vv - sv) ** 2 <= 25 ** 2) * 255).astype(np.uint8)
    assert second[bv, bu] == 0
    nothing = np.zeros((480, 640), np.uint8)
    holes = (da == 0).astype(np.uint8)                                       # only pixels without a cell
    wide = np.zeros((480, 700), np.uint8)
    wide[:, :640] = rect
    top = int(vote.max())
    cases = [("none", None, 1), ("rect", rect, 1), ("nothing", nothing, 1), ("second", second, 1), ("holes", holes, -40000), ("padded", wide[:, :640], 1),
             ("min_vote at the best", None, top), ("min_vote above the best", None, top + 1), ("negative votes too", rect, -100)]
    found = 0
    for name, mask, min_vote in cases:
        want = gm.key_argmax(vote, roll, mask, min_vote)
        got = eng.best_in_mask(0, fa, mask, min_vote)
        if want is None:
            assert got is None, name
            continue
        found += 1
        c, u, v = got
        assert (u, v) == want, (name, (u, v), want)
        assert (c["best_vote"], c["best_roll"], c["best_row"] * W + c["best_col"]) == (int(vote[v, u]), int(roll[v, u]), int(cell[v, u])), name
        assert c == eng.cell_pose(0, int(roll[v, u]), int(cell[v, u]) // W, int(cell[v, u]) % W), name
        # ... and the same from a device-resident frame
        assert eng.best_in_mask(0, device_copy(fa, da), mask, min_vote) == got, name
    assert found == 6 and eng.best_in_mask(0, fa, nothing) is None and eng.best_in_mask(0, fa, holes, -40000) is None
    eng.close()


def test_engine_side_refusals_leave_the_engine_as_it_was(data_dir, surrogate, golden_dir, tmp_path, table1):
    """Every refusal of haf_grasp_map, haf_cell_pose and haf_grasp_map_best returns its code and a text, writes nothing, and leaves the
    last-batch state and the next map untouched"""
    import json
    L = capi.testlib()
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    da = render_depth(table1, CAM_A)[:40, :64].copy()
    da[da == 0] = 900
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=4096)
    h = eng._h
    inp = capi.default_input(**C3_IN)
    n = 40 * 64
    vote, roll, cell = np.full(n, 7, np.int16), np.full(n, 7, np.int16), np.full(n, 7, np.int32)
    cand, u, v, found = capi.GraspCandidate(), C.c_int32(-5), C.c_int32(-5), C.c_int32(-5)

    def map_rc(request=0, frame=fa, on_device=0):
        return L.haf_grasp_map(h, request, C.byref(frame) if frame else None, vote.ctypes.data, roll.ctypes.data, cell.ctypes.data, on_device)

    def best_rc(request=0, frame=fa, mask=None, stride=0, out=cand, fnd=found):
        return L.haf_grasp_map_best(h, request, C.byref(frame) if frame else None, mask, stride, 1, C.byref(out) if out else None, C.byref(u), C.byref(v),
                                    C.byref(fnd) if fnd else None)

    def pose_rc(request=0, r=0, row=10, col=10, out=cand):
        return L.haf_cell_pose(h, request, r, row, col, C.byref(out) if out else None)

    def untouched():
        return (vote == 7).all() and (roll == 7).all() and (cell == 7).all() and (u.value, v.value, found.value) == (-5, -5, -5)
    for rc in (map_rc(), best_rc(), pose_rc()):                               # no scored batch
        assert rc == A and b"no scored batch" in L.haf_last_error(h)
    assert L.haf_grasp_map(None, 0, C.byref(fa), None, None, None, 0) == A and L.haf_cell_pose(None, 0, 0, 0, 0, C.byref(cand)) == A
    assert L.haf_grasp_map_best(None, 0, C.byref(fa), None, 0, 1, C.byref(cand), None, None, C.byref(found)) == A
    small = np.ascontiguousarray(table1[::30])                                # (max_points = 4096)
    out = eng.score(small, inp)
    ref_state = snapshot(eng, out)
    ref_map = eng.grasp_map(0, fa)
    mask = np.ones((40, 64), np.uint8)
    big = capi.depth_frame(np.ones((65, 64), np.uint16), **K525)               # 4160 pixels > max_points
    checks = [(map_rc(request=1), A), (map_rc(request=-1), A), (map_rc(frame=None), A), (map_rc(on_device=2), A), (map_rc(on_device=-1), A),
              (map_rc(frame=big), CAP), (best_rc(request=1), A), (best_rc(frame=None), A), (best_rc(out=None), A), (best_rc(fnd=None), A),
              (best_rc(frame=big), CAP), (best_rc(mask=mask.ctypes.data, stride=63), A),
              (pose_rc(request=1), A), (pose_rc(request=-1), A), (pose_rc(r=-1), A), (pose_rc(r=12), A), (pose_rc(row=-1), A), (pose_rc(row=56), A),
              (pose_rc(col=-1), A), (pose_rc(col=56), A), (pose_rc(out=None), A)]
    for i, (rc, code) in enumerate(checks):
        assert rc == code and L.haf_last_error(h), (i, rc, code)
    for name, frame, code, _ in fc.refusal_frames():
        assert map_rc(frame=frame) == code and best_rc(frame=frame) == code, name
        assert L.haf_last_error(h), name
    assert untouched()
    assert snapshot(eng, out) == ref_state
    again = eng.grasp_map(0, fa)
    assert all((again[k] == ref_map[k]).all() for k in ref_map)
    # a roll outside a scored sub-range
    eng.score_rolls([small], [inp], 4, 3)
    assert pose_rc(r=3) == A and pose_rc(r=7) == A and pose_rc(r=4) == capi.HAF_OK and pose_rc(r=6) == capi.HAF_OK
    eng.close()
    # probability mode: fp32 votes, no map
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as fh:
        pj = json.load(fh)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    prob = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=1 << 18)
    prob.score(table1, inp)
    for call in (lambda: prob.grasp_map(0, fa), lambda: prob.cell_pose(0, 0, 10, 10), lambda: prob.best_in_mask(0, fa)):
        with pytest.raises(capi.HafError) as ei:
            call()
        assert ei.value.code == A and "PROBABILITY" in str(ei.value)
    prob.close()


def read_pgm16(path):
    with open(path, "rb") as f:
        data = f.read()
    magic, w, h, maxval = data.split(None, 4)[:4]
    assert magic == b"P5" and int(maxval) == 65535
    body = data[len(data) - 2 * int(w) * int(h):]
    return np.frombuffer(body, ">u2").reshape(int(h), int(w)).astype(np.int64) - 32768


def test_cli_writes_the_maps_and_prints_the_masked_best(data_dir, surrogate, tmp_path, table1):
    """haf_grasp_cli --depth ... --map-out PREFIX --mask FILE.pgm: the two 16-bit PGMs decode (sample - 32768) to the images
    haf_grasp_map returns for the same goal, and the "mask" line is haf_grasp_map_best's pixel and hypothesis; also through the Python
    mirror of the action server"""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    da = render_depth(table1, CAM_A)
    pa, pm, prefix = str(tmp_path / "a.pgm"), str(tmp_path / "mask.pgm"), str(tmp_path / "map")
    fc.write_pgm16(pa, da)
    mask = np.zeros((480, 640), np.uint8)
    mask[150:330, 220:420] = 200
    with open(pm, "wb") as f:
        f.write(b"P5\n# an instance mask\n640 480\n255\n" + mask.tobytes())
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % v for v in CAM_A]
    plain = subprocess.run(common, check=True, capture_output=True, text=True).stdout
    run = subprocess.run(common + ["--map-out", prefix, "--mask", pm], check=True, capture_output=True, text=True).stdout
    assert run.startswith(plain)
    extra = run[len(plain):].splitlines()
    assert len(extra) == 1 and extra[0].startswith("mask ")
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    frame = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    res = srv.execute_frame(goal, frame)
    assert int(plain.splitlines()[-1].split()[0]) == res.eval > 50
    maps = srv.grasp_map(frame)
    assert (maps["vote"] > 0).sum() >= 3000
    assert (read_pgm16(prefix + ".vote.pgm") == maps["vote"]).all() and (read_pgm16(prefix + ".roll.pgm") == maps["roll"]).all()
    msg, u, v = srv.best_in_mask(frame, mask)
    assert mask[v, u] and (u, v) == gm.key_argmax(maps["vote"], maps["roll"], mask, 1)
    assert [int(t) for t in extra[0].split()[1:4]] == [u, v, msg.eval]
    cand, cu, cv = srv.engine.best_in_mask(0, frame, mask)
    line = [float(t) for t in extra[0].split()[4:13]]                        # grasp points 1 and 2, approach vector: "%g" text
    np.testing.assert_allclose(line, list(cand["grasp_point1"]) + list(cand["grasp_point2"]) + list(cand["approach_vector"]), rtol=1e-5, atol=1e-6)
    empty = str(tmp_path / "empty.pgm")
    with open(empty, "wb") as f:
        f.write(b"P5 640 480 255\n" + bytes(640 * 480))
    run = subprocess.run(common + ["--mask", empty], check=True, capture_output=True, text=True).stdout
    assert run == plain + "mask none\n"
    assert srv.best_in_mask(frame, np.zeros((480, 640), np.uint8)) is None
    # a map without a depth image is a usage error
    assert subprocess.run([cli, "--features", f_, "--range", r_, "--model", surrogate, "--map-out", prefix, os.path.join(data_dir, "pcd2.pcd")],
                          capture_output=True, text=True).returncode == 2
    srv.close()
