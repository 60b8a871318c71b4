"""haf_measure_labels on the MI355X (include/hafgrasp.h; csrc/labelshape.hip): the kernel against haf_measure_labels_ref in EVERY word of
every entry on every case of shape_cases -- host and device-resident frames of all three kinds crossed with host and device label images,
one label, 4096 labels with 64 of them in every wave, labels that alternate inside a lane's group, a label split over far-apart
workgroups, empty labels, values above n_labels, consecutive calls on the reused table; the composition with haf_segment_frame on the
rendered table1 scene; the engine's state; the refusals; the per-object flow of the Python server against the one-request flow and
against single requests; the command line.  Every comparison is an equality.  Testing build, the guard zones checked inside every call
and after every test."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import shape_cases as sc
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, K525, _files, device_copy, make_engine
from test_grasp_map_gpu import full_state
from test_label_shape_cpu import OBJECT_LINE, SHAPE_LINE, shape_refusals, untouched_shapes
from test_plane_cpu import table1_frame
from test_views_gpu import CAM_A

pytestmark = pytest.mark.gpu

CASES = sc.small_cases()
BY_NAME = {c[0]: c for c in CASES}
SEGMENT_OVER_FIT = dict(min_height=0.03, max_gap=0.02, min_pixels=50, max_labels=255)
# the goal of the flow test: its 56 cm grid spans y in [0.17, 0.73], the table's objects lie at y in [0.02, 0.38]: seven of the eleven
# (label 11 at (0.27, 0.07) among them) are outside the one request's grid
FAR_GOAL = dict(grasp_area_center=(0.06, 0.45, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
OUTSIDE_LABEL = 11


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


def device_labels(labels):
    """a host label image (rows may be padded) -> a capi.LabelImage of the same bytes, padding included, on the device"""
    import torch
    stride = labels.strides[0] if labels.shape[0] > 1 else labels.shape[1] * labels.itemsize
    span = (labels.shape[0] - 1) * stride + labels.shape[1] * labels.itemsize
    t = torch.from_numpy(np.frombuffer(C.string_at(labels.ctypes.data, span), np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    img = capi.LabelImage(t.data_ptr(), labels.itemsize, 1, stride)
    img._keep = t
    return img


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_host_definition_word_for_word(eng, case):
    name, frame, image, labels, n_labels, plane = case
    want = capi.measure_labels_ref(frame, labels, n_labels, plane)
    dev, dlab = device_copy(frame, image), device_labels(labels)
    for fr, lab, where in ((frame, labels, "host frame, host labels"), (dev, dlab, "device frame, device labels"),
                           (frame, dlab, "host frame, device labels"), (dev, labels, "device frame, host labels")):
        sc.same(eng.measure_labels(fr, lab, n_labels, plane), want, (name, where))
    other = None if plane is not None else sc.TABLE_PLANE          # each case with a plane and without
    sc.same(eng.measure_labels(dev, dlab, n_labels, other), capi.measure_labels_ref(frame, labels, n_labels, other), (name, "the other plane"))


def test_consecutive_calls_with_fewer_labels_reuse_the_table(eng):
    """4096 rows, then 256, then 5, then 1 on other frames: a row of an earlier call must not survive into a later one"""
    for name in ("distinct_u16_130x33", "n256_f32_130x33", "above_xyz_64x16", "one_u16_17x5", "distinct_xyz_130x33", "alternate_f32_8x1"):
        _, frame, image, labels, n_labels, plane = BY_NAME[name]
        sc.same(eng.measure_labels(frame, labels, n_labels, plane), capi.measure_labels_ref(frame, labels, n_labels, plane), name)
    _, frame, image, labels, _, plane = BY_NAME["distinct_u16_130x33"]
    for n in (4096, 300, 17):                                           # the same image under a shrinking n_labels
        sc.same(eng.measure_labels(frame, labels, n, plane), capi.measure_labels_ref(frame, labels, n, plane), n)


def test_composition_with_the_segmenter_on_table1(eng, table1):
    """haf_segment_frame into the engine's image, haf_measure_labels on that device image: the shapes of the reference on the downloaded
    image, and n_pixels of every label is haf_segment_info's"""
    fa, da = table1
    fit = capi.fit_plane_ref(fa)
    sp = capi.segment_params(plane=fit["plane"], **SEGMENT_OVER_FIT)
    ref_labels, ref_infos, _ = capi.segment_ref(fa, sp)
    n = len(ref_infos)
    assert n >= 2
    plane = list(sp.plane)
    want = capi.measure_labels_ref(fa, ref_labels, n, plane)
    for frame in (fa, device_copy(fa, da)):
        img, infos, _ = eng.segment(frame, sp, device_out=True)
        assert img.on_device == 1 and infos.tobytes() == ref_infos.tobytes()
        got = eng.measure_labels(frame, img, n, plane)
        sc.same(got, want, "table1")
        assert (got["n_pixels"] == infos["n_pixels"]).all() and got["found"].all()
    labels16 = eng.segment(fa, capi.segment_params(plane=fit["plane"], **dict(SEGMENT_OVER_FIT, max_labels=4096)), np.uint16)[0]
    sc.same(eng.measure_labels(fa, labels16, n, plane), want, "uint16 image")
    sc.same(want, sc.mirror_measure(fa, da, ref_labels, n, plane), "mirror")
    assert (want["height"] > 0.03).all() and (want["height"] < 0.3).all() and (want["narrow_width"] <= want["long_width"] * 1.05).all()


def test_measuring_leaves_the_last_batch_alone_and_needs_none(data_dir, golden_dir, surrogate, tmp_path, table1):
    import json
    import models
    fa, da = table1
    _, frame, image, labels, n_labels, plane = BY_NAME["n255_f32_130x33"]
    want = capi.measure_labels_ref(frame, labels, n_labels, plane)
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    sc.same(e.measure_labels(frame, labels, n_labels, plane), want, "a fresh engine, before any request")
    inp = capi.default_input(**C3_IN)
    out = e.score_frames([fa], [inp])[0]
    before, map_before = full_state(e, out), e.grasp_map(0, fa)
    lab = (da > 0).astype(np.uint8)
    for name in ("n255_f32_130x33", "distinct_xyz_130x33", "one_u16_64x16"):
        _, fr, im, lb, nl, pl = BY_NAME[name]
        e.measure_labels(fr, lb, nl, pl)
        e.measure_labels(device_copy(fr, im), device_labels(lb), nl, pl)
    e.measure_labels(fa, lab, 1, [0, 0, 1, 0])
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
    sc.same(e.measure_labels(frame, labels, n_labels, plane), want, "HAF_FLAG_PROBABILITY")
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code and a text that names the call, writes nothing and leaves the engine usable"""
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    _, frame, image, labels, n_labels, plane = BY_NAME["alternate_u16_17x5"]
    labels = np.ascontiguousarray(labels)
    want = capi.measure_labels_ref(frame, labels, n_labels, plane)
    for name, fr, img, nl, pl, with_out, code in shape_refusals(frame, labels):
        shapes = untouched_shapes()
        keep = np.asarray(pl, np.float32) if pl is not None else None
        rc = L.haf_measure_labels(h, C.byref(fr) if fr is not None else None, C.byref(img) if img is not None else None, nl,
                                  keep.ctypes.data if keep is not None else None, shapes.ctypes.data if with_out else None)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text.startswith("haf_measure_labels: "), (name, rc, code, text)
        assert shapes.tobytes() == untouched_shapes().tobytes(), name
        sc.same(e.measure_labels(frame, labels, n_labels, plane), want, name)
    img, _ = capi.label_image(labels, frame, 2)
    assert L.haf_measure_labels(None, C.byref(frame), C.byref(img), 2, None, untouched_shapes().ctypes.data) == capi.HAF_E_ARG
    big = capi.depth_frame(np.ones((64, 65), np.uint16), **K525)             # 4160 pixels > max_points
    shapes = untouched_shapes()
    big_img, _ = capi.label_image(np.ones((64, 65), np.uint8), big, 1)
    assert L.haf_measure_labels(h, C.byref(big), C.byref(big_img), 1, None, shapes.ctypes.data) == capi.HAF_E_CAPACITY
    assert "max_points" in L.haf_last_error(h).decode() and shapes.tobytes() == untouched_shapes().tobytes()
    e.close()


def goal_of(inp):
    from haf_grasping_amd import GraspInputMsg
    return GraspInputMsg(grasp_area_center=tuple(inp.grasp_area_center), grasp_area_length_x=inp.grasp_area_length_x,
                         grasp_area_length_y=inp.grasp_area_length_y)


def test_a_request_per_object_reaches_what_one_request_cannot(data_dir, surrogate, tmp_path, table1):
    """CalcGraspPointsServer.execute_frame_per_object on table1 with a goal whose grid leaves objects out.  First, on the CPU: the
    oracle's grids for label 11's own window give that label a pixel with a vote >= min_vote (haf_label_best_ref on them).  Then:
    execute_frame_segmented with the goal has no entry for the label, the per-object flow has one, and every grasp of the flow is what
    ONE request centred on that object gives -- execute_frame(goal_b, frame, roi_mask=image), then best_per_object -- field for field.
    The command line prints the same objects."""
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from oracle import oracle as O
    from test_engine_gpu import oracle_input
    fa, da = table1
    f_, r_ = _files(data_dir)
    fit = capi.fit_plane_ref(fa)
    sp = capi.segment_params(plane=fit["plane"], **SEGMENT_OVER_FIT)
    ref_labels, ref_infos, _ = capi.segment_ref(fa, sp)
    n = len(ref_infos)
    ref_shapes = capi.measure_labels_ref(fa, ref_labels, n, list(sp.plane))
    assert n >= OUTSIDE_LABEL and ref_shapes["box_max"][OUTSIDE_LABEL - 1][1] < 0.45 - 0.28       # the whole object is off the goal's grid
    cfg = capi.default_config(grid_h=56, grid_w=56, **C3_CFG)
    base = capi.default_input(**FAR_GOAL)
    own, fits = capi.object_input(cfg, base, ref_shapes[OUTSIDE_LABEL - 1], 4)
    pts = capi.frame_points(fa)
    orc = O.Oracle(f_, r_, surrogate)
    own_kw = dict(grasp_area_center=tuple(own.grasp_area_center), grasp_area_length_x=own.grasp_area_length_x, grasp_area_length_y=own.grasp_area_length_y)
    grids = orc.run(pts[np.isfinite(pts).all(axis=1)], O.make_cfg(H=56, W=56, **C3_CFG), oracle_input(own_kw))["graspseval"]
    cpu = capi.label_best_ref(cfg, own, 0, grids, fa, ref_labels, n_labels=n, min_vote=1)
    assert fits and cpu["picks"]["found"][OUTSIDE_LABEL - 1] and cpu["picks"]["vote"][OUTSIDE_LABEL - 1] >= 1

    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 22, max_clouds=4, **C3_CFG)
    goal = GraspInputMsg(**FAR_GOAL)
    _, one_request = srv.execute_frame_segmented(goal, fa, sp)
    assert OUTSIDE_LABEL not in [o[0] for o in one_request]
    flow = srv.execute_frame_per_object(goal, fa, sp)
    sc.same(srv.last_shapes, ref_shapes, "last_shapes")
    by_label = {o[0]: o for o in flow}
    assert OUTSIDE_LABEL in by_label and len(flow) > len(one_request) and len(flow) > 4            # more than one chunk of max_clouds
    assert (by_label[OUTSIDE_LABEL][2], by_label[OUTSIDE_LABEL][3]) == (cpu["picks"]["u"][OUTSIDE_LABEL - 1], cpu["picks"]["v"][OUTSIDE_LABEL - 1])
    keys = []
    img, _, _ = srv.engine.segment(fa, sp, device_out=True)
    for label, msg, u, v, shape, fit_flag in flow:
        inp, want_fits = capi.object_input(cfg, base, ref_shapes[label - 1], 4)
        srv.execute_frame(goal_of(inp), fa, roi_mask=(img.data, img.row_stride_bytes))
        single = {o[0]: o for o in srv.best_per_object(fa, img, min_vote=1, n_labels=n)}
        assert single[label] == (label, msg, u, v), label
        assert fit_flag == want_fits and shape == capi.shape_to_dict(ref_shapes[label - 1])
        pick = srv.engine.best_per_label(0, fa, img, n_labels=n)["picks"][label - 1]
        keys.append((-int(pick["vote"]), int(pick["roll"]), v * 640 + u))
    assert keys == sorted(keys)                                            # best first, in haf_grasp_map_labels' order
    via_fit = srv.execute_frame_per_object(goal, fa, capi.segment_params(**SEGMENT_OVER_FIT), plane="fit")
    assert via_fit == flow and srv.last_plane_fit["found"]
    assert srv.execute_frame_per_object(goal, fa, capi.segment_params(plane=fit["plane"], **dict(SEGMENT_OVER_FIT, min_height=5.0))) == []

    # the command line: the same objects, best first, and the shapes of a label file
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pa, pl = str(tmp_path / "a.pgm"), str(tmp_path / "labels.pgm")
    fc.write_pgm16(pa, da)
    with open(pl, "wb") as f:
        f.write(b"P5\n640 480\n255\n" + ref_labels.tobytes())
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.06", "0.45", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % x for x in CAM_A]
    run = subprocess.run(common + ["--segment", "0.03,0,0.02,50", "--plane", "fit", "--per-object", "4"], check=True, capture_output=True, text=True)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("object ")]
    assert len(lines) == len(flow) and len(run.stdout.splitlines()) == len(lines) + 1          # the plane line, then the objects
    for line, (label, msg, u, v, shape, _) in zip(lines, flow):
        m = re.match(OBJECT_LINE, line)
        assert m and [int(m.group(k)) for k in (1, 2, 3)] == [label, u, v], line
        t = m.group(4).split()
        assert int(t[0]) == msg.eval
        np.testing.assert_allclose([float(x) for x in t[1:10]], list(msg.graspPoint1) + list(msg.graspPoint2) + list(msg.approachVector), rtol=1e-5, atol=1e-6)
        assert np.float32(m.group(5)) == np.float32(shape["narrow_width"]) and int(m.group(6)) == 15 * shape["narrow_dir"]
        assert np.float32(m.group(7)) == np.float32(shape["height"])
    plane = ["%.9g" % x for x in sp.plane]
    run = subprocess.run(common + ["--labels", pl, "--measure", "--plane"] + plane, check=True, capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert len(lines) == n
    for l, line in enumerate(lines):
        m = re.match(SHAPE_LINE, line)
        s = ref_shapes[l]
        assert m and [int(m.group(k)) for k in (1, 2, 3, 4)] == [l + 1, s["found"], s["n_pixels"], s["n_points"]], line
        got = np.array([m.group(k) for k in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17, 18)], np.float32)
        want = np.concatenate([s["centroid"], s["box_min"], s["box_max"], [s["narrow_width"], s["long_width"], s["diameter"], s["height"]]])
        assert got.tobytes() == want.astype(np.float32).tobytes() and int(m.group(16)) == 15 * s["narrow_dir"], line
    srv.close()
