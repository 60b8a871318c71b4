"""haf_score_frames_roi on the MI355X (include/hafgrasp.h; csrc/roi.hip, the ROI forms in prestages.hip and vote.hip): scoring only the
cells near the cells of the masked pixels.  At C3 against the CPU oracle -- evaluated cells, labels, vote grids, records, output -- for
every mask kind and every residence of frame and mask; on larger grids (both branches of k_vote_cells) against the engine's own full
request; a batch against its requests one by one; the last-batch state behind an ROI call and the next plain call; the refusals; the
CLI.  Every comparison is an equality.  Testing build throughout; the guard zones around every device buffer are checked after every
request and after each test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import models
import pcdio
import roi_cases as rc
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import oracle_input
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, _files, device_copy, make_engine, render_depth, snapshot
from test_grasp_map_gpu import full_state
from test_views_gpu import CAM_A, CAM_B

pytestmark = pytest.mark.gpu

H = W = 56


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(scope="module")
def orc(data_dir, surrogate):
    f, r = _files(data_dir)
    return O.Oracle(f, r, surrogate)


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


@pytest.fixture(scope="module")
def cam_a(table1):
    """table1 rendered from CAM_A: (frame, image, words of its pixels' points)"""
    da = render_depth(table1, CAM_A)
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    return fa, da, fc.mirror_points(fa, da)


@pytest.fixture(scope="module")
def c3_full(orc, cam_a):
    """the CPU oracle's full request on cam_a's points at C3; computed once, never written"""
    return orc.run(capi.frame_points(cam_a[0]), O.make_cfg(**C3_CFG), oracle_input(C3_IN))


def device_mask(mask, pad=3):
    """the mask in device memory, its rows `pad` bytes apart from packed and the padding NOT zero -> ((pointer, stride), keep-alive)"""
    import torch
    h, w = mask.shape
    wide = np.full((h, w + pad), 9, np.uint8)
    wide[:, :w] = mask
    dev = torch.from_numpy(wide).cuda()
    torch.cuda.synchronize()
    return (dev.data_ptr(), w + pad), dev


def strip(d):
    return {k: v for k, v in d.items() if k != "n_rechecked"}      # (counted per batch, and by whichever tier decided)


def expected(eng, inp, Ms, words, mask, full_mask, full_labels, full_votes, heights):
    """The definition, from the FULL request's grids: -> (S, E, labels, votes, records, output) of the ROI request"""
    R, Hh, Ww = full_votes.shape
    S = rc.mirror_roi(Ms, words, mask, Hh, Ww)
    E = rc.dilate(S) & (full_mask != 0)
    labels = np.where(E, full_labels, -1).astype(np.int8)
    votes = np.where(S, full_votes, 0).astype(np.float32)
    rec = np.zeros(R, capi.ROLL_RECORD_DTYPE)
    for r in range(R):
        vote, row, col, hl = rc.mirror_record(votes[r], heights[r])
        rec[r] = (vote, row, col, hl, int(E[r].sum()))
    return S, E, labels, votes, rec, eng.finalize(inp, rec)


def check_roi_state(eng, request, got, want, name):
    """the last batch of `eng` against expected()'s tuple: DBG_MASK, DBG_LABELS, the roll grids (votes and evaluated cells), the output"""
    S, E, labels, votes, rec, out = want
    for r in range(votes.shape[0]):
        assert (eng.debug(capi.DBG_MASK, request, r) == E[r]).all(), (name, "mask", r)
        lab = eng.debug(capi.DBG_LABELS, request, r)
        assert (lab == labels[r]).all(), (name, "labels", r, int((lab != labels[r]).sum()))
        ev, m = eng.roll_grid(request, r)
        assert (ev == votes[r]).all(), (name, "votes", r, int((ev != votes[r]).sum()))
        assert (m == E[r]).all(), (name, "roll grid mask", r)
    assert strip(got) == strip(out), (name, got, out)
    assert got["n_evals"] == int(E.sum()) or int(got["rolls_done"]) < votes.shape[0], (name, got["n_evals"], int(E.sum()))


def test_roi_equals_the_oracle_restricted_to_the_mask_at_c3(data_dir, surrogate, cam_a, c3_full):
    """56 x 56, 20 rolls, surrogate model, table1 rendered from CAM_A.  For every mask kind (a rectangle over one object, ~200 scattered
    pixels, all ones, all zeros, only invalid pixels, one pixel, the rectangle with a padded stride), the frame and the mask each host- and
    device-resident: the evaluated cells are E_r, the labels the oracle's on E_r and -1 elsewhere, the roll grid the oracle's votes on S_r
    and 0 elsewhere, the output haf_finalize of the mirror's records, n_evals the sum of |E_r|.
    The rectangle (roi_cases.C3_RECT), on the oracle's grids: 3 800 ROI cells, 6 368 of 31 093 evaluations, best vote 93."""
    fa, da, words = cam_a
    full = c3_full
    eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    dev_frame = device_copy(fa, da)
    seen = {}
    for name, mask in rc.masks(words, 480, 640, rect=rc.C3_RECT):
        want = expected(eng, inp, full["M"], words, mask, full["mask"], full["labels"], full["graspseval"], full["heights"])
        S, E = want[0], want[1]
        dm, keep = device_mask(mask)
        for how, frame, m in (("host/host", fa, mask), ("host/device", fa, dm), ("device/host", dev_frame, mask), ("device/device", dev_frame, dm)):
            got = eng.score_frames_roi([frame], [m], [inp])[0]
            check_roi_state(eng, 0, got, want, name + " " + how)
            assert got["n_evals"] == int(E.sum()) == eng.last_counts()["n_evals"], (name, how)
        seen[name] = (int(S.sum()), int(E.sum()), int(want[3].max()), got["eval"])
    print(seen, "full n_evals", full["n_evals"])
    assert 0 < seen["rect"][1] < full["n_evals"] / 2 and seen["rect"][2] > 0
    assert seen["rect_padded"] == seen["rect"] and seen["rect"][3] == seen["rect"][2] - 20
    # every pixel masked: S_r is every cell that holds a point.  Still not the full request: a cell of the search area whose nearest
    # point lies 3 or 4 rows away is evaluated there (the 9 x 9 box test) but not here (30 649 of 31 093 on the oracle's grids)
    assert full["n_evals"] / 2 < seen["ones"][1] <= full["n_evals"] and 0 < seen["ones"][2] <= full["top"]
    assert 0 < seen["scattered"][0] <= 20 * 200 and 0 < seen["one_pixel"][0] <= 20 and seen["one_pixel"][1] <= 20 * 29
    # an empty ROI is the reference's "nothing found"
    for name in ("zeros", "invalid_only"):
        assert seen[name] == (0, 0, 0, -20), (name, seen[name])
    eng.close()


@pytest.mark.parametrize("grid", [160, 131], ids=["160_quad_vote", "131_scalar_vote"])
def test_larger_grids_equal_the_full_request_restricted_to_the_mask(data_dir, tmp_path, grid):
    """160 x 160 and 131 x 131 (both above the one-workgroup vote; the first takes the quad branch of k_vote_cells, the second the scalar
    one; 131 also has rows of three 64-bit ROI words with a partial last one), 8 rolls, a random 64-SV model, a 640 x 480 frame of the
    synthetic cloud (307 200 points: the bucket-sorted binning runs).  Labels, votes, records and output of the ROI request are as defined
    from the grids and heights of the engine's own full haf_score_frames, which the other suites pin to the oracle."""
    model = models.write_random_model(str(tmp_path / "m64.model"), 64, seed=5, balanced=True)
    cfg_kw = dict(grid_h=grid, grid_w=grid, n_rolls=8, roll_step_deg=20)
    in_kw = dict(grasp_area_length_x=grid, grasp_area_length_y=grid)
    xyz = models.synthetic_cloud(grid=grid, k=3, seed=2)
    cam = np.array([1, 0, 0, 0.0, 0, -1, 0, 0.0, 0, 0, -1, 1.5], np.float32)
    depth = render_depth(xyz, cam)
    frame = capi.depth_frame(depth, sensor_to_base=cam, **K525)
    words = fc.mirror_points(frame, depth)
    eng = make_engine(data_dir, model, max_points=640 * 480, **cfg_kw)
    inp = capi.default_input(**in_kw)
    full_out = eng.score_frames([frame], [inp])[0]
    before = snapshot(eng, full_out)
    R = 8
    fm = np.stack([eng.debug(capi.DBG_MASK, 0, r) for r in range(R)])
    fl = np.stack([eng.debug(capi.DBG_LABELS, 0, r) for r in range(R)])
    fh = np.stack([eng.debug(capi.DBG_HEIGHTS, 0, r) for r in range(R)])
    fv = np.stack([eng.roll_grid(0, r)[0] for r in range(R)])
    assert full_out["n_evals"] >= 8 * 10000 and (fv > 0).any() and (fl == 1).any()
    # the rectangle: 160 x 120 pixels around the best pixel of the full request's grasp map, so that a grasp lies under it
    full_map = eng.grasp_map(0, frame)
    bu, bv = gm.key_argmax(full_map["vote"], full_map["roll"], None, 1)
    rect = (max(0, bv - 60), min(480, bv + 60), max(0, bu - 80), min(640, bu + 80))
    Ms = rc.oracle_transforms(cfg_kw, in_kw, 0, R)
    dev_frame = device_copy(frame, depth)
    seen = {}
    for k, (name, mask) in enumerate(rc.masks(words, 480, 640, rect=rect)):
        want = expected(eng, inp, Ms, words, mask, fm, fl, fv, fh)
        dm, keep = device_mask(mask)
        got = eng.score_frames_roi([dev_frame if k % 2 else frame], [dm if k % 3 == 0 else mask], [inp])[0]
        check_roi_state(eng, 0, got, want, "%d %s" % (grid, name))
        seen[name] = (int(want[0].sum()), int(want[1].sum()), int(want[3].max()))
    print(grid, seen, "full n_evals", full_out["n_evals"])
    assert 0 < seen["rect"][1] < full_out["n_evals"] / 2 and seen["rect"][2] == int(full_map["vote"].max()) > 0 and seen["scattered"][1] > 0
    assert full_out["n_evals"] / 2 < seen["ones"][1] <= full_out["n_evals"] and seen["zeros"] == (0, 0, 0)
    # the full request afterwards is what it was
    again = eng.score_frames([frame], [inp])[0]
    after = snapshot(eng, again)
    assert before.keys() == after.keys()
    for key in before:
        assert before[key] == after[key], key
    eng.close()


def test_batch_equals_its_requests_one_by_one(data_dir, surrogate, table1, cam_a):
    """Three requests in one call -- different frames (a U16 image, an F32 crop with limits, a device-resident image from another camera),
    different masks (host, device, host with a padded stride) and different inputs, one of them with a negative budget -- equal the three
    requests one by one in output and in every grid"""
    fa, da, words = cam_a
    db = render_depth(table1, CAM_B)
    metres = da.astype(np.float32) * np.float32(0.001)
    crop = metres[60:440, 40:600]
    fcrop = capi.depth_frame(crop, fx=525.0, fy=525.0, cx=319.5 - 40, cy=239.5 - 60, sensor_to_base=CAM_A, min_depth=0.3, max_depth=1.5)
    fb = capi.depth_frame(db, sensor_to_base=CAM_B, **K525)
    frames = [fa, fcrop, device_copy(fb, db)]
    ma = dict(rc.masks(words, 480, 640, rect=rc.C3_RECT))
    mcrop = dict(rc.masks(fc.mirror_points(fcrop, crop), 380, 560))
    mb = dict(rc.masks(fc.mirror_points(fb, db), 480, 640))
    dm, keep = device_mask(mcrop["scattered"])
    masks = [ma["rect"], dm, mb["rect_padded"]]
    inputs = [capi.default_input(**C3_IN), capi.default_input(max_calculation_time=-1.0, **C3_IN),
              capi.default_input(**dict(C3_IN, approach_vector=(0.1, -0.1, 1.0), gripper_opening_width=2))]
    eng = make_engine(data_dir, surrogate, max_clouds=3, max_points=3 * 640 * 480, **C3_CFG)
    outs = eng.score_frames_roi(frames, masks, inputs)
    batch = snapshot(eng, None, 3)
    labels = [[eng.debug(capi.DBG_LABELS, b, r).tobytes() for r in range(20)] for b in range(3)]
    assert outs[0]["eval"] > -20 and outs[0]["n_evals"] > 0 and outs[1]["rolls_done"] == 0 and outs[1]["n_evals"] == 0 and outs[2]["n_evals"] > 0
    assert strip(outs[1]) == strip(eng.score_frames([frames[1]], [inputs[1]])[0])      # no roll ran: the reference's untouched overall best
    for b in range(3):
        o = eng.score_frames_roi([frames[b]], [masks[b]], [inputs[b]])[0]
        assert strip(o) == strip(outs[b]), b
        if b == 1:
            continue                                      # (alone, a request with a negative budget scores nothing: no last batch)
        single = snapshot(eng, None)
        for r in range(20):
            assert single["grid", 0, r] == batch["grid", b, r], (b, r)
            assert eng.debug(capi.DBG_LABELS, 0, r).tobytes() == labels[b][r], (b, r)
        assert single["top"][0] == batch["top"][b], b
    eng.close()


def test_state_behind_an_roi_call_and_the_next_plain_call(data_dir, surrogate, cam_a):
    """After an ROI call the last-batch state is the ROI request's: the best vote over its rolls is the maximum of the FULL request's
    grasp map over the masked pixels, haf_top_grasps' rank 1 is the output, haf_cell_pose of the winner its pose, haf_grasp_map_best
    under the same mask finds that vote.  A plain haf_score_frames afterwards reproduces the state it left before the ROI call exactly,
    haf_last_tiers and haf_screen_form included."""
    fa, da, words = cam_a
    mask = dict(rc.masks(words, 480, 640, rect=rc.C3_RECT))["rect"]
    eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    full_out = eng.score_frames([fa], [inp])[0]
    before = full_state(eng, full_out)
    form = (eng.screen_form(), eng.screen_state())
    full_map = eng.grasp_map(0, fa)
    best_full = int(full_map["vote"][mask != 0].max())
    assert 0 < best_full < full_out["best_vote"]                           # (the overall best grasp lies outside the rectangle)
    for m in (mask, device_mask(mask)[0]):
        out = eng.score_frames_roi([fa], [m], [inp])[0]
        grids = np.stack([eng.roll_grid(0, r)[0] for r in range(20)])
        assert int(grids.max()) == best_full == out["best_vote"] and out["eval"] == best_full - 20
        top = eng.top_grasps(k=4)[0]
        for f in ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector", "roll", "eval", "best_row", "best_col", "best_roll", "best_vote"):
            assert np.array(top[0][f]).tobytes() == np.array(out[f]).tobytes(), f
        pose = eng.cell_pose(0, out["best_roll"], out["best_row"], out["best_col"])
        for f in ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector", "roll", "eval", "best_vote"):
            assert np.array(pose[f]).tobytes() == np.array(out[f]).tobytes(), f
        roi_map = eng.grasp_map(0, fa)
        assert int(roi_map["vote"][mask != 0].max()) == best_full and int(roi_map["vote"].max()) == best_full
        hit = eng.best_in_mask(0, fa, mask)
        assert hit is not None and hit[0]["best_vote"] == best_full and mask[hit[2], hit[1]]
        assert (eng.screen_form(), eng.screen_state()) == form
        assert eng.stage_ms()["mask"] > 0.0
    again = eng.score_frames([fa], [inp])[0]
    after = full_state(eng, again)
    assert before.keys() == after.keys()
    for k in before:
        if k != "stage_ms":
            assert before[k] == after[k], k
    assert (eng.screen_form(), eng.screen_state()) == form
    eng.close()


def test_screening_list_overflow_is_served_without_touching_the_screening_form(data_dir, surrogate, cam_a, c3_full, monkeypatch):
    """An ROI request whose screening pass leaves more undecided than the refinement list holds (a 256-entry list and a 50 x wider
    screening band, testing build) is decided by the three-pass kernel for this call: the labels, votes and output are the definition's,
    the overflow is counted, and the engine's choice of the screening form is what it was -- an ROI request never re-chooses it."""
    for k, v in dict(HAF_FLAG0_CAP="256", HAF_GUARD0_REL="50", HAF_NO_DIRECT="1", HAF_NO_CALIBRATE="1").items():
        monkeypatch.setenv(k, v)
    fa, da, words = cam_a
    mask = dict(rc.masks(words, 480, 640, rect=rc.C3_RECT))["rect"]
    eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    form = (eng.screen_form(), eng.screen_state())
    assert form[1]["active"]
    want = expected(eng, inp, c3_full["M"], words, mask, c3_full["mask"], c3_full["labels"], c3_full["graspseval"], c3_full["heights"])
    for m in (mask, device_mask(mask)[0]):
        seen = eng.overflow_stats()["screening_list_overflows"]
        got = eng.score_frames_roi([fa], [m], [inp])[0]
        assert eng.overflow_stats()["screening_list_overflows"] == seen + 1
        check_roi_state(eng, 0, got, want, "overflow")
        assert (eng.screen_form(), eng.screen_state()) == form
    eng.close()


def test_refusals_leave_the_engine_as_it_was(data_dir, surrogate, golden_dir, tmp_path, table1):
    """Every refusal of haf_score_frames_roi returns its code and a text that names the request, before any device work: the last-batch
    state stays what it was.  An engine created with HAF_FLAG_PROBABILITY is refused."""
    import json
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=4096)
    L, h = eng._L, eng._h
    inp = capi.default_input()
    rng = np.random.default_rng(4)
    img = fc.u16_image(rng, 61, 5)
    good = capi.depth_frame(img, sensor_to_base=np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0.9], np.float32), **fc._intrinsics(rng, 61, 5))
    mask = np.ones((5, 61), np.uint8)
    out0 = eng.score_frames([good], [inp])[0]
    ref = full_state(eng, out0)

    def roi(m=mask.ctypes.data, stride=61, on_device=0):
        return capi.Roi(m, stride, on_device)

    def refused(n, frames, rois, inputs, out, code, names=True):
        rc_ = L.haf_score_frames_roi(h, n, frames, rois, inputs, out)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc_ == code and "haf_score_frames_roi" in text, (rc_, code, text)
        now = full_state(eng, out0)
        assert all(now[k] == ref[k] for k in ref if k != "stage_ms")
        return text

    two, gi, out = (capi.Frame * 2)(good, good), (capi.GraspInput * 2)(inp, inp), (capi.GraspOutput * 2)()
    rr = (capi.Roi * 2)(roi(), roi())
    for args in ((1, None, rr, gi, out), (1, two, None, gi, out), (1, two, rr, None, out), (1, two, rr, gi, None), (0, two, rr, gi, out), (-3, two, rr, gi, out)):
        refused(*args, A)
    assert L.haf_score_frames_roi(None, 1, two, rr, gi, out) == A
    for bad in (roi(m=None), roi(stride=60), roi(stride=0), roi(on_device=2), roi(on_device=-1)):
        assert "request 0" in refused(1, two, (capi.Roi * 2)(bad, roi()), gi, out, A)
        assert "request 1" in refused(2, two, (capi.Roi * 2)(roi(), bad), gi, out, A)      # checked before request 0 is touched
    three = (capi.Frame * 3)(good, good, good)
    assert "max_clouds" in refused(3, three, (capi.Roi * 3)(roi(), roi(), roi()), (capi.GraspInput * 3)(inp, inp, inp), (capi.GraspOutput * 3)(), CAP)
    big = np.ones((64, 65), np.uint16)
    assert "max_points" in refused(1, (capi.Frame * 1)(capi.depth_frame(big, **K525)), rr, gi, out, CAP)
    half = capi.depth_frame(np.ones((42, 50), np.uint16), **K525)
    assert "max_points" in refused(2, (capi.Frame * 2)(half, half), rr, gi, out, CAP)
    for name, frame, code, _ in fc.refusal_frames():
        assert "request 0" in refused(1, (capi.Frame * 1)(frame), rr, gi, out, code), name
        assert "request 1" in refused(2, (capi.Frame * 2)(good, frame), rr, gi, out, code), name
    # ... and the valid call is served
    got = eng.score_frames_roi([good], [mask], [inp])[0]
    assert got["n_evals"] <= out0["n_evals"]
    eng.close()
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as fh:
        pj = json.load(fh)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    prob = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=4096)
    with pytest.raises(capi.HafError) as ei:
        prob.score_frames_roi([good], [mask], [inp])
    assert ei.value.code == A and "PROBABILITY" in str(ei.value)
    prob.close()


def test_cli_roi_mask_prints_the_grasp_of_the_roi_request(data_dir, surrogate, tmp_path, cam_a):
    """haf_grasp_cli --depth ... --roi-mask FILE.pgm prints the grasp Engine.score_frames_roi returns for the same goal, and --top-k works
    behind it on the restricted request; also through the Python mirror of the action server (execute_frame(roi_mask=))"""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    fa, da, words = cam_a
    pa, pm = str(tmp_path / "a.pgm"), str(tmp_path / "roi.pgm")
    fc.write_pgm16(pa, da)
    mask = dict(rc.masks(words, 480, 640, rect=rc.C3_RECT))["rect"] * np.uint8(200)
    with open(pm, "wb") as f:
        f.write(b"P5\n# an instance mask\n640 480\n255\n" + mask.tobytes())
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % v for v in CAM_A]
    plain = subprocess.run(common, check=True, capture_output=True, text=True).stdout.splitlines()
    run = subprocess.run(common + ["--roi-mask", pm, "--top-k", "2"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(plain) == 1 and len(run) in (2, 3) and run[1].startswith("top 1 ") and run[1][len("top 1 "):] == run[0]
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    res = srv.execute_frame(goal, fa, roi_mask=mask)
    out = srv.engine.score_frames_roi([fa], [mask], [goal.to_c()])[0]
    assert int(run[0].split()[0]) == res.eval == out["eval"] > -20 and int(plain[0].split()[0]) > res.eval
    line = [float(t) for t in run[0].split()[1:10]]                          # grasp points 1 and 2, approach vector: "%g" text
    np.testing.assert_allclose(line, list(out["grasp_point1"]) + list(out["grasp_point2"]) + list(out["approach_vector"]), rtol=1e-5, atol=1e-6)
    srv.close()
    # two views and an ROI mask: a usage error
    assert subprocess.run(common + ["--depth", pa, "--roi-mask", pm], capture_output=True, text=True).returncode == 2
