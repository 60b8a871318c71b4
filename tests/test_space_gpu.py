"""haf_check_space on the MI355X (include/hafgrasp.h; csrc/space.hip): the kernel against haf_check_space_ref in EVERY word of every row,
in order, n_clear, info and every state byte, on every case of space_cases -- host and device-resident views of both depth kinds, mixed
in one call, 1 to 8 views, 1 to 257 grasps, 1 to 65536 samples; one call on a caller's stream with stream-ordered views; the engine's
state; the refusals; the Python server and the command line.  Every comparison is an equality.  Testing build, the guard zones checked
inside every call and after every test."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import clearance_cases as cc
import frame_cases as fc
import models
import space_cases as spc
import stream_cases as stc
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, device_copy, make_engine
from test_grasp_map_gpu import full_state
from test_plane_cpu import table1_frame
from test_views_gpu import CAM_A
from test_space_cpu import CASES                 # (builds the cases: after the modules above)

pytestmark = pytest.mark.gpu

SPACE_LINE = r"^space (\d+) (-?\d+) hit (\d+) hidden (\d+) unseen (\d+) free (\d+) between-hit (\d+)$"
REF = {}


def ref_of(case):
    """haf_check_space_ref's answer, computed once per case, shared and never changed"""
    if case["name"] not in REF:
        REF[case["name"]] = spc.run(capi.check_space_ref, case)
    return REF[case["name"]]


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


def check(e, case, views, states=True):
    return e.check_space(views, spc.grasp_arg(case), capi.gripper(**case["gripper"]), capi.space_params(**case["params"]), states=states)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_host_definition_word_for_word(eng, case):
    want = ref_of(case)
    host = [f for f, _ in case["views"]]
    dev = [device_copy(f, img) for f, img in case["views"]]
    spc.same(check(eng, case, host), want, (case["name"], "host views"))
    spc.same(check(eng, case, dev), want, (case["name"], "device views"))
    mixed = [d if k % 2 == 0 else h for k, (h, d) in enumerate(zip(host, dev))]
    if len(host) > 1:
        spc.same(check(eng, case, mixed), want, (case["name"], "device and host views in one call"))
    got = check(eng, case, mixed, states=False)           # without states: the same rows, nothing in the scratch
    assert len(got) == 3 and got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() and got[2] == want[2]


def test_one_call_on_a_callers_stream_with_stream_ordered_views(eng):
    """the engine on a caller's stream; both views are zeros until a copy that waits behind a delay on that stream (stream_cases: a call
    that ran on any other stream would read the zeros and see nothing anywhere)"""
    import torch
    s = stc.scene()
    views = [s["frames"]["u16"], s["frames"]["f32"]]
    g, p = capi.gripper(), capi.space_params(sample_step=0.01, max_unknown=10)
    want = capi.check_space_ref([f for f, _ in views], s["grasps"], g, p, states=True)
    assert want[0]["n"][:, :, spc.UNSEEN + 1:].sum() > 0          # the late views can change the result: all-zero views leave every sample UNSEEN
    # The caller's stream is HIP's default stream, stream_cases' mode "null": the engine leaves its own stream for it, and the delay and
    # the late copies go to torch's default stream, which is that stream.  No stream is created here.  A torch.cuda.Stream() is taken
    # from torch's pool and never given back: it would change which pool stream, and with it which hardware queue, every later stream
    # test of the process gets (test_streams_gpu.py's control test needs its torch stream and an engine's own on different queues)
    S = torch.cuda.default_stream()
    cycles, _ = stc.calibrate_sleep(torch, S)
    e = eng                                               # (the module's engine: no engine and no stream of this test's own)
    own = e.get_stream()
    assert own != 0
    e.set_stream(0)
    try:
        d = stc.Late(torch, S, cycles)
        late = [d.frame(f, img) for f, img in views]
        with d:
            got = e.check_space(late, s["grasps"], g, p, states=True)
        spc.same(got, want, "both views late")
        assert e.get_stream() == 0
    finally:
        e.set_stream(own)
    assert e.get_stream() == own
    spc.same(e.check_space([f for f, _ in views], s["grasps"], g, p, states=True), want, "back on the engine's own stream")


def test_candidates_of_a_scored_frame_and_the_last_batch(data_dir, surrogate, golden_dir, tmp_path):
    """before any request; score_frames -> top_grasps(k=32) -> check_space on the rendered table1 frame at C3: equal to the reference on
    the same dicts; the last batch's state is what it was, a second top_grasps gives the same candidates; a candidate array goes in by its
    stride; an engine with HAF_FLAG_PROBABILITY serves the call"""
    fa, da = table1_frame(data_dir)
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    p = capi.space_params(sample_step=0.008, max_unknown=20, max_hit=5)
    one = [cc.grasp_of((0.13, 0.25, 0.05), (0, 0, 1), (1, 0, 0))]
    first = capi.check_space_ref([fa], one, None, p, states=True)
    spc.same(e.check_space([fa], one, None, p, states=True), first, "before any request")
    out = e.score_frames([fa], [capi.default_input(**C3_IN)])[0]
    cands = e.top_grasps(k=32)[0]
    assert len(cands) >= 2
    before = full_state(e, out)
    want = capi.check_space_ref([fa], cands, None, p, states=True)
    assert want[0]["n"][:, :, spc.HIT].sum() > 0 and want[0]["n"][:, :, spc.FREE].sum() > 0
    spc.same(e.check_space([fa], cands, None, p, states=True), want, "host view")
    spc.same(e.check_space([device_copy(fa, da), fa], cands, None, p, states=True), capi.check_space_ref([fa, fa], cands, None, p, states=True),
             "the view twice, device and host")
    arr = (capi.GraspCandidate * len(cands))()
    for c, d in zip(arr, cands):
        for f in cc.POSE_FIELDS:
            setattr(c.grasp, f, (C.c_double * 3)(*d[f]))
    spc.same(e.check_space([fa], arr, None, p, states=True), want, "a haf_grasp_candidate array")
    after = full_state(e, out)
    assert before.keys() == after.keys()
    for k in before:
        assert before[k] == after[k], k
    assert e.top_grasps(k=32)[0] == cands
    e.close()
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    e = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=640 * 480)
    spc.same(e.check_space([fa], one, None, p, states=True), first, "HAF_FLAG_PROBABILITY")
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code, writes nothing and leaves the engine usable; the text names the call"""
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    rng = np.random.default_rng(5)
    view = spc.scene_view("u16", 8, 6, spc.IDENTITY, rng)
    arr, n, stride = capi._grasp_array([spc.EXACT_GRASP])
    out = np.zeros(n, capi.SPACE_DTYPE)

    def call(views, n_views=None, grip=None, params=None, handle=h):
        frames = (capi.Frame * len(views))(*views)
        return L.haf_check_space(handle, frames, len(views) if n_views is None else n_views, C.byref(grip or capi.gripper()),
                                 C.byref(params or capi.space_params()), n, arr, stride, out.ctypes.data, None, None, None, None)

    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    assert call([view[0]], handle=None) == A
    assert call([view[0]], n_views=0) == A and (L.haf_last_error(h) or b"").decode().startswith("haf_check_space: ")
    assert call([view[0]], params=capi.space_params(sample_step=2.0)) == A
    assert call([view[0], capi.xyz_frame(np.zeros((6, 8, 3), np.float32))]) == A and b"view 1" in L.haf_last_error(h)
    assert call([view[0]], grip=capi.gripper(**spc.OVER_CAP), params=capi.space_params(sample_step=spc.STEP)) == A
    big = capi.depth_frame(np.ones((64, 65), np.uint16), 525.0, 525.0, 32.0, 32.0)             # 4160 pixels > max_points
    assert call([view[0], big]) == CAP and b"max_points" in L.haf_last_error(h)
    half = capi.depth_frame(np.ones((64, 40), np.uint16), 525.0, 525.0, 20.0, 32.0)            # 2560 pixels: two host views do not fit
    assert call([half, half]) == CAP and b"max_points" in L.haf_last_error(h)
    assert call([half, device_copy(half, np.ones((64, 40), np.uint16))]) == capi.HAF_OK        # a device-resident view is read in place
    out[:] = 0
    assert call([half, half]) == CAP and not out.tobytes().strip(b"\0")
    case = next(c for c in CASES if c["name"] == "views_2")
    spc.same(check(e, case, [f for f, _ in case["views"]]), ref_of(case), "after the refusals")
    e.close()


def test_server_on_the_occluded_finger_scene(data_dir, surrogate):
    """CalcGraspPointsServer.seen_free_grasps() on the box scene, scored from the front camera: the candidates whose row says clear == 1,
    in rank order, each with its own message, for one view and for two and for three sets of thresholds -- the defaults, 40 unknown
    samples allowed, and thresholds that admit every pose; the second view can only turn unknown samples into seen ones; free_grasps
    and top_grasps answer as before"""
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import _files
    front, back, grasp = spc.occluded_scene()
    f_, r_ = _files(data_dir)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=2 * 160 * 120, **C3_CFG)
    # the pose the CPU suite examines, through the engine: hidden behind the box with one view, clear with two
    rows, order, _ = srv.engine.check_space([front[0]], [grasp])
    assert rows["n"][0][spc.FINGER0][spc.HIDDEN] > 0 and order.tolist() == []
    assert srv.engine.check_space([front[0], back[0]], [grasp])[1].tolist() == [0]
    srv.execute_frame(GraspInputMsg(grasp_area_center=(0.0, 0.0, 0.0), grasp_area_length_x=30, grasp_area_length_y=30), front[0])
    ranked = srv.top_grasps(k=16, min_vote=1)
    cands = srv.engine.top_grasps(k=16, min_vote=1)[0]
    assert len(cands) >= 2 and len(ranked) == len(cands)
    free_before = srv.free_grasps(front[0], k=16, min_vote=1)
    wide = capi.space_params(max_hit=10 ** 6, max_unknown=10 ** 6, min_between_hit=0)
    n_pairs = 0
    for p in (None, capi.space_params(max_unknown=40), wide):
        unknown = []
        for views in ([front[0]], [front[0], back[0]]):
            got = srv.seen_free_grasps(views, k=16, params=p, min_vote=1)
            rows, order, _ = capi.check_space_ref(views, cands, None, p)
            assert [c.tobytes() for _, c in got] == [rows[i].tobytes() for i in order]
            assert len(got) == len(order)
            for (msg, _), i in zip(got, order):
                assert (msg.eval, msg.graspPoint1, msg.graspPoint2, msg.averagedGraspPoint, msg.approachVector, msg.roll) == \
                       (ranked[i].eval, ranked[i].graspPoint1, ranked[i].graspPoint2, ranked[i].averagedGraspPoint, ranked[i].approachVector, ranked[i].roll)
            if p is wide:                                 # thresholds that refuse nothing: every pose that is not void comes back, in rank order
                assert order.tolist() == np.flatnonzero(rows["clear"] != -1).tolist() and len(got) >= 2
            else:
                n_pairs += len(got)
            unknown.append(rows["n"][:, 1:, :spc.FREE].sum(axis=(1, 2)))
        assert (unknown[1] <= unknown[0]).all()
    assert n_pairs >= 1                                   # some candidate is seen free under thresholds that can refuse
    assert srv.top_grasps(k=16, min_vote=1) == ranked
    again = srv.free_grasps(front[0], k=16, min_vote=1)
    assert [(m, c.tobytes()) for m, c in again] == [(m, c.tobytes()) for m, c in free_before]
    srv.close()


def test_cli_reports_the_seen_space(data_dir, surrogate, tmp_path):
    """haf_grasp_cli --top-k --gripper --check-space prints the binding's rows behind the unchanged top and clear lines, for one --depth
    view and for two, which all go to haf_check_space; the clear candidates' hypothesis strings, hafshim::seen_free_hypotheses', go to
    stderr and are the `top` lines' of the same ranks"""
    import subprocess
    import pcdio
    from test_frames_gpu import _files
    from test_views_gpu import CAM_B, TABLE1, two_cameras
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    frames = two_cameras(pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd")))
    paths = [str(tmp_path / "a.pgm"), str(tmp_path / "b.pgm")]
    for path, f in zip(paths, frames):
        fc.write_pgm16(path, f._keep)
    poses = [["%.9g" % x for x in CAM_A], ["%.9g" % x for x in CAM_B]]
    goal = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
    params = capi.space_params(sample_step=0.008, tol_abs=0.004, tol_rel=0.002, max_hit=100000, max_unknown=100000)
    n_clear = 0
    for n_views in (1, 2):
        common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
                  "--search-size", "42", "42", "--top-k", "32", "--intrinsics", "525", "525", "319.5", "239.5"]
        for k in range(n_views):
            common += ["--depth", paths[k], "--sensor-pose"] + poses[k]
        common += ["--gripper", "default"]
        plain = subprocess.run(common, check=True, capture_output=True, text=True)
        assert "space " not in plain.stdout and "seen free" not in plain.stderr
        run = subprocess.run(common + ["--check-space", "0.008,0.004,0.002,100000,100000"], check=True, capture_output=True, text=True)
        lines = run.stdout.splitlines()
        seen = [l for l in lines if l.startswith("space ")]
        assert [l for l in lines if not l.startswith("space ")] == plain.stdout.splitlines()       # no other line changes
        tops = [l.split(" ", 2)[2] for l in lines if l.startswith("top ")]
        assert len(seen) == len(tops) >= 2 and lines[-len(seen):] == seen
        e = make_engine(data_dir, surrogate, max_points=1 << 22, **C3_CFG)
        if n_views == 1:
            e.score_frames(frames[:1], [goal])
        else:
            e.score_views([frames], [goal])
        cands = e.top_grasps(k=32)[0]
        rows, order, _ = e.check_space(frames[:n_views], cands, capi.gripper(), params)
        e.close()
        assert len(cands) == len(seen)
        for rank, (line, r) in enumerate(zip(seen, rows)):
            assert re.match(SPACE_LINE, line), line
            n = r["n"][1:].sum(axis=0)
            want = "space %d %d hit %d hidden %d unseen %d free %d between-hit %d" % (rank + 1, r["clear"], n[spc.HIT], n[spc.HIDDEN], n[spc.UNSEEN],
                                                                                     n[spc.FREE], r["n"][spc.BETWEEN][spc.HIT])
            assert line == want, (line, want)
        free = [l.split(": seen free: ", 1)[1] for l in run.stderr.splitlines() if ": seen free: " in l]
        assert free == [tops[i] for i in order], (free, order)
        n_clear += len(order)
    assert n_clear >= 1                                   # the shim's strings were compared for at least one candidate
