"""haf_check_grasps on the MI355X (include/hafgrasp.h; csrc/clearance.hip): the kernels against haf_check_grasps_ref in EVERY word of
every row, in order and n_free, on every case of clearance_cases -- host and device-resident frames of all three kinds, host and device
masks, 1 to 257 grasps on 1 to 1073 pixels; consecutive calls on the reused scratch; the rendered table1 scene behind haf_score_frames
and haf_top_grasps; the engine's state; the refusals; the Python server and the command line.  Every comparison is an equality.  Testing
build, the guard zones checked inside every call and after every test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clearance_cases as cc
import frame_cases as fc
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, device_copy, make_engine
from test_grasp_map_gpu import full_state
from test_plane_cpu import table1_frame
from test_plane_gpu import device_mask
from test_views_gpu import CAM_A
from test_clearance_cpu import CASES, every_refusal, ref_of       # (builds the cases: after the modules above)

pytestmark = pytest.mark.gpu

CLEAR_LINE = r"^clear (\d+) (-?\d+) fingers (\d+) (\d+) palm (\d+) between (\d+) width (\S+) offset (\S+) top (\S+)$"


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


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_the_host_definition_word_for_word(eng, case):
    name, frame, image, kw, grasps, mask = case
    g = capi.gripper(**kw)
    want = ref_of(case)
    dev = device_copy(frame, image)
    keep, dmask = device_mask(mask) if mask is not None else (None, None)
    for fr, m, where in ((frame, mask, "host frame, host mask"), (dev, dmask, "device frame, device mask"), (frame, dmask, "host frame, device mask"),
                         (dev, mask, "device frame, host mask")):
        cc.same(eng.check_grasps(fr, grasps, g, m), want, (name, where))
        if mask is None and fr is dev:
            break


def test_consecutive_calls_reuse_the_scratch(eng):
    """the rows of a call are cleared: 257 grasps, then 1 on another frame, then 65 with a mask -- and once more around"""
    by_name = {c[0]: c for c in CASES}
    for name in ("cloud1025_grasps257", "u16_37x29_grasps1", "boxes_masked_f32_pad5", "only_void", "cloud513_grasps65", "cloud1_grasps1"):
        _, frame, image, kw, grasps, mask = by_name[name]
        cc.same(eng.check_grasps(frame, grasps, capi.gripper(**kw), mask), ref_of(by_name[name]), name)
    assert ref_of(by_name["cloud1025_grasps257"])[0]["n_near"].sum() > 0 and ref_of(by_name["u16_37x29_grasps1"])[0]["n_near"].sum() > 0


def test_candidates_of_a_scored_frame_and_the_last_batch(data_dir, surrogate, table1):
    """score_frames -> top_grasps(k=32) -> check_grasps on the rendered table1 frame at C3: equal to the reference on the same dicts; the
    last batch's state is what it was, a second top_grasps gives the same candidates; a candidate array goes in by its stride"""
    fa, da = table1
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    g = capi.gripper()
    fresh = e.check_grasps(fa, [cc.grasp_of((0.13, 0.25, 0.05), (0, 0, 1), (1, 0, 0))], g)       # a fresh engine, before any request
    cc.same(fresh, capi.check_grasps_ref(fa, [cc.grasp_of((0.13, 0.25, 0.05), (0, 0, 1), (1, 0, 0))], g), "before any request")
    out = e.score_frames([fa], [capi.default_input(**C3_IN)])[0]
    cands = e.top_grasps(k=32)[0]
    assert len(cands) >= 2
    before = full_state(e, out)
    want = capi.check_grasps_ref(fa, cands, g)
    assert want[0]["n_near"].sum() > 0 and (want[0]["n_near"] > 0).all()      # a grasp point lies within a centimetre of the scene's surface
    cc.same(e.check_grasps(fa, cands, g), want, "host frame")
    cc.same(e.check_grasps(device_copy(fa, da), cands, g), want, "device frame")
    mask = (da > 0).astype(np.uint8)
    mask[:, :300] = 0
    cc.same(e.check_grasps(fa, cands, capi.gripper(opening=0.05, max_hits=5), mask), capi.check_grasps_ref(fa, cands, capi.gripper(opening=0.05, max_hits=5), mask), "masked")
    arr = (capi.GraspCandidate * len(cands))()
    for c, d in zip(arr, cands):
        for f in cc.POSE_FIELDS:
            setattr(c.grasp, f, (C.c_double * 3)(*d[f]))
    cc.same(e.check_grasps(fa, arr, g), want, "a haf_grasp_candidate array")
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
    case = next(c for c in CASES if c[0] == "boxes_u16_pad3")
    name, frame, image, kw, grasps, mask = case
    every_refusal(lambda *a: L.haf_check_grasps(h, *a), False)
    assert (L.haf_last_error(h) or b"").decode().startswith("haf_check_grasps: ")
    arr, n, stride = capi._grasp_array(grasps)
    out = np.zeros(n, capi.CLEARANCE_DTYPE)
    assert L.haf_check_grasps(None, C.byref(frame), None, C.byref(capi.gripper()), n, arr, stride, out.ctypes.data, None, None) == capi.HAF_E_ARG
    big = capi.depth_frame(np.ones((64, 65), np.uint16), 525.0, 525.0, 32.0, 32.0)             # 4160 pixels > max_points
    assert L.haf_check_grasps(h, C.byref(big), None, C.byref(capi.gripper()), n, arr, stride, out.ctypes.data, None, None) == capi.HAF_E_CAPACITY
    assert "max_points" in (L.haf_last_error(h) or b"").decode() and not out.tobytes().strip(b"\0")
    cc.same(e.check_grasps(frame, grasps, capi.gripper(**kw), mask), ref_of(case), "after the refusals")
    e.close()


def test_server_and_cli_report_the_clearance(data_dir, surrogate, tmp_path, table1):
    """CalcGraspPointsServer.free_grasps() == the candidates whose row says free == 1, in rank order; haf_grasp_cli --top-k --gripper prints
    the binding's rows behind the unchanged top lines, on a --depth frame and on a .pcd"""
    import subprocess
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import TABLE1, _files
    fa, da = table1
    f_, r_ = _files(data_dir)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    srv.execute_frame(goal, fa)
    ranked = srv.top_grasps(k=32)
    cands = srv.engine.top_grasps(k=32)[0]
    wide = capi.gripper(opening=0.12, max_hits=2)
    for g in (None, wide):
        rows, order = capi.check_grasps_ref(fa, cands, g)
        got = srv.free_grasps(fa, k=32, gripper=g)
        assert [m for m, _ in got] == [ranked[i] for i in np.flatnonzero(rows["free"] == 1)]
        assert [c.tobytes() for _, c in got] == [rows[i].tobytes() for i in order]
    assert srv.top_grasps(k=32) == ranked
    srv.close()
    # the command line
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pa = str(tmp_path / "a.pgm")
    fc.write_pgm16(pa, da)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--top-k", "32"]
    depth = ["--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % x for x in CAM_A]
    pcd = os.path.join(data_dir, TABLE1 + ".pcd")
    cloud = capi.cloud_frame(np.ascontiguousarray(capi.load_pcd(pcd)[:, :3], np.float32))
    inp = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
    for source, scene, spec, g in ((depth, fa, "default", capi.gripper()),
                                   ([pcd], cloud, "0.12,0.01,0.02,0.03,0.06,0.12,0.04,0.04", capi.gripper(opening=0.12))):
        plain = subprocess.run(common + source, check=True, capture_output=True, text=True).stdout
        assert "clear" not in plain
        lines = subprocess.run(common + ["--gripper", spec] + source, check=True, capture_output=True, text=True).stdout.splitlines()
        clear = [l for l in lines if l.startswith("clear ")]
        assert [l for l in lines if not l.startswith("clear ")] == plain.splitlines()              # no other line changes
        assert len(clear) == sum(l.startswith("top ") for l in lines) >= 2 and lines[-len(clear):] == clear
        # (the poses in the hypothesis strings are rounded: the rows to compare with come from the binding's own candidates)
        e = make_engine(data_dir, surrogate, max_points=1 << 22, **C3_CFG)
        if scene is fa:
            e.score_frames([fa], [inp])
        else:
            e.score(capi.load_pcd(pcd), inp)
        cands = e.top_grasps(k=32)[0]
        rows, _ = e.check_grasps(scene, cands, g)
        e.close()
        assert len(cands) == len(clear)
        for rank, (line, r) in enumerate(zip(clear, rows)):
            assert re.match(CLEAR_LINE, line), line
            want = "clear %d %d fingers %d %d palm %d between %d width %s offset %s top %s" % (
                rank + 1, r["free"], r["n_finger"][0], r["n_finger"][1], r["n_palm"], r["n_between"], "%.9g" % r["width_m"], "%.9g" % r["offset_m"],
                "%.9g" % r["top_m"])
            assert line == want, (line, want)
