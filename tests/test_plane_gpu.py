"""haf_fit_plane on the MI355X (include/hafgrasp.h; csrc/plane.hip): the kernels against haf_fit_plane_ref in EVERY word -- hypothesis
words, counts, the winner, the ten moments, the plane's bits, rms, found and stats -- on every case of plane_cases: host and
device-resident frames of all three kinds, host and device masks, n_hyp 1 / 64 / 65 / 1024, consecutive calls on the reused scratch; the
rendered table1 scene and the composition with haf_filter_depth, haf_segment_frame, haf_score_frames_roi and haf_grasp_map_labels; the
engine's state; the refusals; the Python server and the command line.  Every comparison is an equality.  Testing build, the guard zones
checked inside every call and after every test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_cases as fc
import plane_cases as pc
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, K525, assert_same, device_copy, make_engine, snapshot
from test_grasp_map_gpu import engine_grids, full_state
from test_plane_cpu import PLANE_LINE, check_table1_fit, plane_refusals, table1_frame, untouched_result
from test_views_gpu import CAM_A

pytestmark = pytest.mark.gpu

CASES = pc.small_cases()
SEGMENT_OVER_FIT = dict(min_height=0.03, max_gap=0.02, min_pixels=50, max_labels=255)


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")          # every fit checks the guard zones itself, too
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


def device_mask(mask):
    """a host mask (rows may be padded) -> (tensor to keep, (pointer, row stride)): the same bytes, padding included, on the device"""
    import torch
    stride = mask.strides[0]
    span = (mask.shape[0] - 1) * stride + mask.shape[1]
    t = torch.from_numpy(np.frombuffer(C.string_at(mask.ctypes.data, span), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr(), stride)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_the_host_definition_word_for_word(eng, case):
    name, frame, image, kw, mask = case
    p = capi.plane_params(**kw)
    want = capi.fit_plane_ref(frame, p, mask, debug=True)
    dev = device_copy(frame, image)
    keep, dmask = device_mask(mask) if mask is not None else (None, None)
    for fr, m, where in ((frame, mask, "host frame, host mask"), (dev, dmask, "device frame, device mask"), (frame, dmask, "host frame, device mask"),
                         (dev, mask, "device frame, host mask")):
        pc.same(eng.fit_plane(fr, p, m, debug=True), want, (name, where))
        if mask is None and fr is dev:
            break
    plain = eng.fit_plane(frame, p, mask)                 # counts and hyps are optional
    assert plain["plane"].tobytes() == want["plane"].tobytes() and plain["stats"] == want["stats"] and plain["rms"] == want["rms"]


def test_consecutive_calls_reuse_the_scratch(eng):
    """the counts, the moments and the counters of a call are cleared: 1024 hypotheses, then 64 on another frame, then 65 with a mask"""
    by_name = {c[0]: c for c in CASES}
    for name in ("boxes_f32_67x33_hyp1024", "boxes_u16_130x17_hyp64", "boxes_masked_xyz_67x33", "usable0_67x33", "holes_u16_67x33", "boxes_u16_67x33_hyp1"):
        _, frame, image, kw, mask = by_name[name]
        p = capi.plane_params(**kw)
        pc.same(eng.fit_plane(frame, p, mask, debug=True), capi.fit_plane_ref(frame, p, mask, debug=True), name)


def test_a_frame_of_more_blocks_than_the_hypothesis_kernel_stages(data_dir, surrogate):
    """2049 x 2048 pixels are 4 099 blocks of 1 024, over the 4 096 prefix words k_plane_hyp keeps in LDS: its searches then read the
    prefix sums from memory.  A tilted plane with a hole of many whole blocks and a ragged last block; 16 hypotheses keep the host
    reference at a fraction of a second"""
    w, h = 2049, 2048
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    z = np.round(1500.0 + 0.05 * u + 0.03 * v).astype(np.uint16)
    z.reshape(-1)[100000:900000] = 0
    z[::7, ::5] = 0
    frame = capi.depth_frame(z, 1000.0, 1000.0, 1024.0, 1023.5, sensor_to_base=CAM_A)
    p = capi.plane_params(n_hyp=16, seed=21)
    want = capi.fit_plane_ref(frame, p, debug=True)
    assert want["found"] and want["stats"][1] > 3000000 and want["n_inliers"] > want["stats"][1] // 2
    e = make_engine(data_dir, surrogate, max_points=w * h)
    pc.same(e.fit_plane(frame, p, debug=True), want, "host frame")
    pc.same(e.fit_plane(device_copy(frame, z), p, debug=True), want, "device frame")
    e.close()


def test_table1_and_the_segmentation_over_the_fitted_plane(eng, table1):
    """640 x 480, 300 blocks: the device equals the reference at the defaults and with 1024 hypotheses; haf_segment_frame over the fitted
    plane equals haf_segment_ref over the reference's fitted plane"""
    fa, da = table1
    want = capi.fit_plane_ref(fa, None, debug=True)
    check_table1_fit(want)
    dev = device_copy(fa, da)
    pc.same(eng.fit_plane(fa, None, debug=True), want, "host")
    pc.same(eng.fit_plane(dev, None, debug=True), want, "device")
    p = capi.plane_params(n_hyp=1024, seed=99, up=[0, 0, 1], max_tilt=0.3)
    pc.same(eng.fit_plane(dev, p, debug=True), capi.fit_plane_ref(fa, p, debug=True), "1024 hypotheses")
    got = eng.fit_plane(fa)
    sp_ref, sp_dev = (capi.segment_params(plane=f["plane"], **SEGMENT_OVER_FIT) for f in (want, got))
    ref_seg = capi.segment_ref(fa, sp_ref)
    assert len(ref_seg[1]) >= 2                              # objects stand on the fitted plane: the test is not vacuous
    seg = eng.segment(fa, sp_dev)
    assert (seg[0] == ref_seg[0]).all() and seg[1].tobytes() == ref_seg[1].tobytes() and seg[2] == ref_seg[2]


def test_the_whole_chain_equals_the_chain_of_host_definitions(data_dir, surrogate, table1):
    """filter -> fit -> segment -> ROI score -> best per label, every image staying on the device, against the same chain fed from
    haf_filter_depth_ref, haf_fit_plane_ref and haf_segment_ref"""
    fa, da = table1
    fp = capi.depth_filter()
    filtered, _ = capi.filter_depth_ref([fa], fp)
    f_host = capi.depth_frame(filtered, sensor_to_base=CAM_A, **K525)
    fit_ref = capi.fit_plane_ref(f_host, None, debug=True)
    assert fit_ref["found"]
    labels_ref, infos_ref, stats_ref = capi.segment_ref(f_host, capi.segment_params(plane=fit_ref["plane"], **SEGMENT_OVER_FIT))
    n = len(infos_ref)
    assert n >= 2
    e = make_engine(data_dir, surrogate, max_points=1 << 20, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    f_dev, _ = e.filter_depth([fa], fp)
    assert f_dev.on_device == 1
    fit = e.fit_plane(f_dev, None, debug=True)
    pc.same(fit, fit_ref, "filtered frame")
    img, infos, stats = e.segment(f_dev, capi.segment_params(plane=fit["plane"], **SEGMENT_OVER_FIT), device_out=True)
    assert infos.tobytes() == infos_ref.tobytes() and stats == stats_ref
    a = snapshot(e, e.score_frames_roi([f_dev], [(img.data, img.row_stride_bytes)], [inp])[0])
    got = e.best_per_label(0, f_dev, img, n_labels=n)
    b = snapshot(e, e.score_frames_roi([f_host], [(labels_ref != 0).astype(np.uint8)], [inp])[0])
    assert_same(a, b)
    want = capi.label_best_ref(e.cfg, inp, 0, engine_grids(e, 0, 0, 20), f_host, labels_ref, n_labels=n)
    assert all((got["picks"][f] == want["picks"][f]).all() for f in capi.LABEL_PICK_DTYPE.names) and got["order"] == want["order"]
    assert len(got["order"]) >= 2
    e.close()


def test_fit_leaves_the_last_batch_alone_and_needs_none(data_dir, golden_dir, surrogate, tmp_path, table1):
    import json
    import models
    fa, da = table1
    want = capi.fit_plane_ref(fa, None, debug=True)
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    pc.same(e.fit_plane(fa, None, debug=True), want, "a fresh engine, before any request")
    inp = capi.default_input(**C3_IN)
    out = e.score_frames([fa], [inp])[0]
    before, map_before = full_state(e, out), e.grasp_map(0, fa)
    xyz = capi.xyz_frame(np.ascontiguousarray(capi.frame_points(capi.depth_frame(da, **K525)).reshape(480, 640, 3)), sensor_to_base=CAM_A)
    mask = (da > 0).astype(np.uint8)
    for frame, kw in ((fa, {}), (device_copy(fa, da), dict(mask=mask)), (xyz, dict(params=capi.plane_params(n_hyp=1024))), (fa, dict(debug=True))):
        e.fit_plane(frame, **kw)
    after = full_state(e, out)
    assert before.keys() == after.keys()
    for k in before:
        assert before[k] == after[k], k
    map_after = e.grasp_map(0, fa)
    assert all((map_before[k] == map_after[k]).all() for k in map_before)
    e.close()
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    e = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=640 * 480)
    pc.same(e.fit_plane(fa, None, debug=True), want, "HAF_FLAG_PROBABILITY")
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code and a text that names the call, writes nothing and leaves the engine usable"""
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    _, frame, image, kw, _ = next(c for c in CASES if c[0] == "boxes_u16_67x33_hyp64")
    p = capi.plane_params(**kw)
    want = capi.fit_plane_ref(frame, p, debug=True)
    mask = np.ones((33, 67), np.uint8)

    def refused(fr, params, code, roi=None, with_out=True):
        res, counts, hyps = untouched_result(), np.full(capi.MAX_PLANE_HYP, -7, np.int32), np.full((capi.MAX_PLANE_HYP, 4), -7, np.float32)
        rc = L.haf_fit_plane(h, C.byref(fr) if fr is not None else None, C.byref(roi) if roi is not None else None,
                             C.byref(params) if params is not None else None, C.byref(res) if with_out else None, counts.ctypes.data, hyps.ctypes.data)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text.startswith("haf_fit_plane: "), (rc, code, text)
        assert bytes(res) == bytes(untouched_result()) and (counts == -7).all() and (hyps == -7).all()
        pc.same(e.fit_plane(frame, p, debug=True), want, text)
        return text

    for name, over in plane_refusals():
        refused(frame, capi.plane_params(**dict(kw, **over)), A)
    for name, fr, code, _ in fc.refusal_frames():
        refused(fr, p, code)
    refused(None, p, A)
    refused(frame, None, A)
    refused(frame, p, A, with_out=False)
    assert L.haf_fit_plane(None, C.byref(frame), None, C.byref(p), C.byref(capi.PlaneResult()), None, None) == A
    refused(frame, p, A, roi=capi.Roi(mask.ctypes.data, 66, 0))
    refused(frame, p, A, roi=capi.Roi(mask.ctypes.data, 67, 2))
    refused(frame, p, A, roi=capi.Roi(mask.ctypes.data, 67, -1))
    big = capi.depth_frame(np.ones((64, 65), np.uint16), **K525)             # 4160 pixels > max_points
    assert "max_points" in refused(big, p, CAP)
    e.close()


def test_server_and_cli_fit_the_plane(data_dir, surrogate, tmp_path, table1):
    """CalcGraspPointsServer.execute_frame_segmented(plane="fit") == the same call with the reference's fitted plane in its parameters;
    without the keyword nothing changes; haf_grasp_cli --segment --plane fit prints the reference's plane and segments over it"""
    import subprocess
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import _files
    fa, da = table1
    f_, r_ = _files(data_dir)
    fit_ref = capi.fit_plane_ref(fa)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    base = capi.segment_params(**SEGMENT_OVER_FIT)
    want = srv.execute_frame_segmented(goal, fa, capi.segment_params(plane=fit_ref["plane"], **SEGMENT_OVER_FIT))
    want_infos = srv.last_segment_infos.tobytes()
    assert srv.last_plane_fit is None and len(want[1]) >= 2
    got = srv.execute_frame_segmented(goal, fa, base, plane="fit")
    assert got == want and srv.last_segment_infos.tobytes() == want_infos
    assert srv.last_plane_fit["found"] and srv.last_plane_fit["plane"].tobytes() == fit_ref["plane"].tobytes()
    assert list(base.plane) == [0.0, 0.0, 1.0, 0.0]                           # the caller's parameters are not written
    tight = capi.plane_params(min_inliers=1 << 20)                            # nothing can be found: the plane of the parameters stays
    assert srv.execute_frame_segmented(goal, fa, base, plane=tight) == srv.execute_frame_segmented(goal, fa, base)
    with pytest.raises(ValueError):
        srv.execute_frame_segmented(goal, fa, base, plane="level")
    srv.close()
    # the command line
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pa, pl, pm = str(tmp_path / "a.pgm"), str(tmp_path / "labels.pgm"), str(tmp_path / "mask.pgm")
    fc.write_pgm16(pa, da)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % x for x in CAM_A]
    seg = ["--segment", "0.03,0,0.02,50"]
    run = subprocess.run(common + seg + ["--plane", "fit", "--labels-out", pl], check=True, capture_output=True, text=True)
    m = re.match(PLANE_LINE, run.stdout.splitlines()[0])
    assert m, run.stdout[:200]
    assert np.array([float(m.group(k)) for k in range(1, 5)], np.float32).tobytes() == fit_ref["plane"].tobytes()
    assert int(m.group(5)) == fit_ref["n_inliers"] and abs(float(m.group(6)) - fit_ref["rms"]) <= 1e-5 * fit_ref["rms"]
    with open(pl, "rb") as f:
        raw = f.read()
    head = b"P5\n640 480\n255\n"
    ref_labels = capi.segment_ref(fa, capi.segment_params(plane=fit_ref["plane"], **SEGMENT_OVER_FIT))[0]
    assert raw.startswith(head) and (np.frombuffer(raw[len(head):], np.uint8).reshape(480, 640) == ref_labels).all()
    typed = subprocess.run(common + seg + ["--plane"] + ["%.9g" % x for x in fit_ref["plane"]], check=True, capture_output=True, text=True)
    assert run.stdout.split("\n", 1)[1] == typed.stdout                       # the same objects as with the plane typed by hand
    mask = np.zeros((480, 640), np.uint8)
    mask[:, :320] = 1
    with open(pm, "wb") as f:
        f.write(b"P5\n640 480\n255\n" + mask.tobytes())
    p2 = capi.plane_params(tol=0.004, n_hyp=128)
    half = capi.fit_plane_ref(fa, p2, mask)
    run2 = subprocess.run(common + seg + ["--plane", "fit,0.004,128", "--plane-mask", pm], check=True, capture_output=True, text=True)
    m2 = re.match(PLANE_LINE, run2.stdout.splitlines()[0])
    assert half["found"] and m2 and int(m2.group(5)) == half["n_inliers"]
    assert np.array([float(m2.group(k)) for k in range(1, 5)], np.float32).tobytes() == half["plane"].tobytes()
