"""haf_fit_openings on the MI355X (include/hafgrasp.h; csrc/opening.hip): the kernels against haf_fit_openings_ref in EVERY word of every
row, in order, n_found, info and every histogram word, on every case of opening_cases -- host and device-resident frames of all three
kinds, host and device masks, 1 to 257 grasps on 1 to 2211 pixels; consecutive calls on the reused block and scratch, with and without
the histograms; one call on a caller's stream with stream-ordered inputs; the engine's state; the refusals; the Python server and the
command line.  Every comparison is an equality.  Testing build, the guard zones checked inside every call and after every test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clearance_cases as cc
import frame_cases as fc
import opening_cases as oc
import stream_cases as sc
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, device_copy, make_engine
from test_grasp_map_gpu import full_state
from test_plane_cpu import table1_frame
from test_plane_gpu import device_mask
from test_views_gpu import CAM_A
from test_opening_cpu import BY_NAME, CASES, every_refusal, ref_of       # (builds the cases: after the modules above)

pytestmark = pytest.mark.gpu

OPEN_LINE = r"^open (\d+) (-?\d+) opening (\S+) shift (\S+) between (\d+) hits (\d+) sym (\S+)$"


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")          # every call checks the guard zones itself, too
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def eng(data_dir, surrogate):
    e = make_engine(data_dir, surrogate, max_points=640 * 480)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table1(data_dir):
    return table1_frame(data_dir)


def fit(e, case, frame=None, mask=None, hist=True):
    name, f, image, kw, pkw, grasps, m = case
    return e.fit_openings(frame if frame is not None else f, grasps, capi.gripper(**kw), capi.opening_params(**pkw), mask if mask is not None else m,
                          hist=hist)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_the_host_definition_word_for_word(eng, case):
    name, frame, image, kw, pkw, grasps, mask = case
    want = ref_of(case)
    dev = device_copy(frame, image)
    keep, dmask = device_mask(mask) if mask is not None else (None, None)
    for fr, m, where in ((frame, mask, "host frame, host mask"), (dev, dmask, "device frame, device mask"), (frame, dmask, "host frame, device mask"),
                         (dev, mask, "device frame, host mask")):
        oc.same(fit(eng, case, fr, m), want, (name, where))
        if mask is None and fr is dev:
            break


def test_consecutive_calls_reuse_the_block_and_the_scratch(eng):
    """the histograms of a call are cleared wherever they lie -- in the block when they are asked for, in the scratch when not --: 257
    grasps, then 1 on another frame, then 65 with a mask, and once more around without the histograms"""
    names = ("cloud1025_grasps257", "block_default", "boxes_masked_f32_pad5", "only_void", "carry_600_600", "cloud257_grasps65", "cloud1_grasps1")
    for hist in (True, False, True):
        for name in names:
            got, want = fit(eng, BY_NAME[name], hist=hist), ref_of(BY_NAME[name])
            assert len(got) == (4 if hist else 3)
            oc.same(got + (() if hist else (want[3], )), want, (name, hist))
    assert ref_of(BY_NAME["cloud1025_grasps257"])[0]["n_finger_slab"].sum() > 0


def test_one_call_on_a_callers_stream_with_stream_ordered_inputs(data_dir, surrogate):
    """the engine on a torch stream; the frame and the mask are zeros until a copy that waits behind a delay on that stream (stream_cases:
    a call that ran on any other stream would read the zeros and find nothing between any fingers)"""
    import torch
    s = sc.scene()
    frame, image = s["frames"]["u16"]
    g, p = capi.gripper(), capi.opening_params(max_hits=3, max_shift=0.01)
    want = capi.fit_openings_ref(frame, s["grasps"], g, p, s["mask_any"], hist=True)
    assert 0 < len(want[1]) and want[3].sum() > 0             # the late inputs can change the result: an all-zero frame counts nothing
    S = torch.cuda.Stream()
    cycles, _ = sc.calibrate_sleep(torch, S)
    e = make_engine(data_dir, surrogate, **sc.ENGINE_KW)
    own = e.get_stream()
    e.set_stream(S.cuda_stream)
    d = sc.Late(torch, S, cycles)
    dframe, dmask = d.frame(frame, image), d.rows(s["mask_any"])
    with d:
        got = e.fit_openings(dframe, s["grasps"], g, p, dmask, hist=True)
    oc.same(got, want, "frame and mask late")
    assert e.get_stream() == S.cuda_stream
    e.set_stream(own)
    oc.same(e.fit_openings(frame, s["grasps"], g, p, s["mask_any"], hist=True), want, "back on the engine's own stream")
    e.close()


def test_candidates_of_a_scored_frame_and_the_last_batch(data_dir, surrogate, table1):
    """score_frames -> top_grasps(k=32) -> fit_openings on the rendered table1 frame at C3: equal to the reference on the same dicts; the
    last batch's state is what it was, a second top_grasps gives the same candidates; a candidate array goes in by its stride"""
    fa, da = table1
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    g, p = capi.gripper(), capi.opening_params(max_shift=0.01, max_hits=2)
    one = [cc.grasp_of((0.13, 0.25, 0.05), (0, 0, 1), (1, 0, 0))]
    oc.same(e.fit_openings(fa, one, g, p, hist=True), capi.fit_openings_ref(fa, one, g, p, hist=True), "before any request")
    out = e.score_frames([fa], [capi.default_input(**C3_IN)])[0]
    cands = e.top_grasps(k=32)[0]
    assert len(cands) >= 2
    before = full_state(e, out)
    want = capi.fit_openings_ref(fa, cands, g, p, hist=True)
    assert (want[0]["n_finger_slab"] > 0).sum() >= len(cands) // 2       # a grasp point lies within a centimetre of the scene's surface
    oc.same(e.fit_openings(fa, cands, g, p, hist=True), want, "host frame")
    oc.same(e.fit_openings(device_copy(fa, da), cands, g, p, hist=True), want, "device frame")
    mask = (da > 0).astype(np.uint8)
    mask[:, :300] = 0
    oc.same(e.fit_openings(fa, cands, g, p, mask, hist=True), capi.fit_openings_ref(fa, cands, g, p, mask, hist=True), "masked")
    arr = (capi.GraspCandidate * len(cands))()
    for c, d in zip(arr, cands):
        for f in cc.POSE_FIELDS:
            setattr(c.grasp, f, (C.c_double * 3)(*d[f]))
    oc.same(e.fit_openings(fa, arr, g, p, hist=True), want, "a haf_grasp_candidate array")
    after = full_state(e, out)
    assert before.keys() == after.keys()
    for k in before:
        assert before[k] == after[k], k
    assert e.top_grasps(k=32)[0] == cands
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code, writes nothing and leaves the engine usable; the text names the call"""
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    case = BY_NAME["boxes_u16_pad3"]
    every_refusal(lambda *a: L.haf_fit_openings(h, *a), False)
    assert (L.haf_last_error(h) or b"").decode().startswith("haf_fit_openings: ")
    arr, n, stride = capi._grasp_array(case[5])
    out = np.zeros(n, capi.OPENING_DTYPE)
    args = (C.byref(capi.gripper()), C.byref(capi.opening_params()), n, arr, stride, out.ctypes.data, None, None, None, None)
    assert L.haf_fit_openings(None, C.byref(case[1]), None, *args) == capi.HAF_E_ARG
    big = capi.depth_frame(np.ones((64, 65), np.uint16), 525.0, 525.0, 32.0, 32.0)             # 4160 pixels > max_points
    assert L.haf_fit_openings(h, C.byref(big), None, *args) == capi.HAF_E_CAPACITY
    assert "max_points" in (L.haf_last_error(h) or b"").decode() and not out.tobytes().strip(b"\0")
    oc.same(fit(e, case), ref_of(case), "after the refusals")
    e.close()


def test_server_chain_on_the_small_boxes_frame(data_dir, surrogate):
    """CalcGraspPointsServer.fitted_grasps() on object_cases' 160 x 120 boxes frame == the candidates whose row says found == 1, in rank
    order, each with its opening applied; free_grasps and top_grasps answer as before"""
    import object_cases as obj
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import _files
    s = sc.scene()
    frame, image = s["frames"]["u16"]
    f_, r_ = _files(data_dir)
    srv = CalcGraspPointsServer(f_, r_, surrogate, **sc.ENGINE_KW)
    srv.execute_frame(GraspInputMsg(**obj.input_kw(s["inputs"][0])), frame)
    ranked = srv.top_grasps(k=16, min_vote=1)
    cands = srv.engine.top_grasps(k=16, min_vote=1)[0]
    free_before = srv.free_grasps(frame, k=16, min_vote=1)
    assert len(cands) >= 2
    n_found = 0
    for p in (None, capi.opening_params(max_shift=0.01, max_hits=4)):
        rows, order, info = capi.fit_openings_ref(frame, cands, None, p)
        got = srv.fitted_grasps(frame, k=16, params=p, min_vote=1)
        assert [c.tobytes() for _, c in got] == [rows[i].tobytes() for i in order]
        for (msg, _), i in zip(got, order):
            applied = capi.apply_opening(cands[i], rows[i])
            assert (msg.graspPoint1, msg.graspPoint2, msg.averagedGraspPoint) == \
                   (applied["grasp_point1"], applied["grasp_point2"], applied["averaged_grasp_point"])
            assert (msg.eval, msg.approachVector, msg.roll) == (ranked[i].eval, ranked[i].approachVector, ranked[i].roll)
        n_found += len(got)
    assert n_found >= 1
    assert srv.top_grasps(k=16, min_vote=1) == ranked
    again = srv.free_grasps(frame, k=16, min_vote=1)
    assert [(m, c.tobytes()) for m, c in again] == [(m, c.tobytes()) for m, c in free_before]
    srv.close()


def test_cli_reports_the_openings(data_dir, surrogate, tmp_path, table1):
    """haf_grasp_cli --top-k --gripper --fit-opening prints the binding's rows behind the unchanged top and clear lines"""
    import subprocess
    from test_frames_gpu import _files
    fa, da = table1
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pa = str(tmp_path / "a.pgm")
    fc.write_pgm16(pa, da)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--top-k", "32", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + \
             ["%.9g" % x for x in CAM_A] + ["--gripper", "default"]
    plain = subprocess.run(common, check=True, capture_output=True, text=True).stdout
    assert "open " not in plain
    lines = subprocess.run(common + ["--fit-opening", "0.01,0.08,0.01"], check=True, capture_output=True, text=True).stdout.splitlines()
    opened = [l for l in lines if l.startswith("open ")]
    assert [l for l in lines if not l.startswith("open ")] == plain.splitlines()                   # no other line changes
    assert len(opened) == sum(l.startswith("top ") for l in lines) >= 2 and lines[-len(opened):] == opened
    e = make_engine(data_dir, surrogate, max_points=1 << 22, **C3_CFG)
    e.score_frames([fa], [capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))])
    cands = e.top_grasps(k=32)[0]
    rows, _, _ = e.fit_openings(fa, cands, capi.gripper(), capi.opening_params(min_opening=0.01, max_opening=0.08, max_shift=0.01))
    e.close()
    assert len(cands) == len(opened)
    for rank, (line, r) in enumerate(zip(opened, rows)):
        assert re.match(OPEN_LINE, line), line
        want = "open %d %d opening %s shift %s between %d hits %d sym %s" % (
            rank + 1, r["found"], "%.9g" % r["opening_m"], "%.9g" % r["shift_m"], r["n_between"], r["n_finger"].sum() + r["n_palm"],
            "%.9g" % r["sym_opening_m"])
        assert line == want, (line, want)
