"""haf_segment_frame on the MI355X (include/hafgrasp.h; csrc/segment.hip): the kernels against haf_segment_ref word for word -- labels,
infos, n_labels and stats -- on every case of segment_cases: host and device-resident frames of all three kinds, uint8 and uint16, into
host memory, into the caller's padded device image and into the engine's own; the ties, the caps, one 640 x 480; the composition with
haf_filter_depth, haf_score_frames_roi and haf_grasp_map_labels on the rendered table1 scene; the engine's state; the refusals; the
Python server and the command line (haf_grasp_cli creates an engine, so its --segment / --labels-out round trip lives here).  Every
comparison is an equality.  Testing build, the guard zones checked inside every call and after every test."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import frame_cases as fc
import pcdio
import segment_cases as sc
from haf_grasping_amd import capi
from test_depth_filter_gpu import SENTINEL, device_image, fetch, rows_of
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, assert_same, device_copy, make_engine, render_depth, snapshot
from test_grasp_map_gpu import engine_grids, full_state
from test_segment_cpu import segment_refusals
from test_views_gpu import CAM_A

pytestmark = pytest.mark.gpu

# the rendered table1 scene under CAM_A: the table's surface lies below z = 0.025 m of the base frame, the objects above it
TABLE1_PARAMS = dict(plane=[0, 0, 1, 0], min_height=0.03, max_gap=0.02, min_pixels=50, max_labels=255)


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")          # every segment call checks the guard zones itself, too
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def eng(data_dir, surrogate):
    e = make_engine(data_dir, surrogate, max_points=640 * 480)
    yield e
    e.close()


def image_of(img, frame, dtype):
    """a LabelImage in device memory -> (labels [height, width], the padding bytes between its rows)"""
    e = np.dtype(dtype).itemsize
    assert img.on_device == 1 and img.elem_bytes == e
    shape = types.SimpleNamespace(height=frame.height, width=frame.width, row_stride_bytes=img.row_stride_bytes)
    return rows_of(fetch(img.data, (frame.height - 1) * img.row_stride_bytes + frame.width * e), shape, dtype)


def segment_into(eng, frame, p, dtype, mode, name):
    """one call into one kind of output -> (labels, infos, stats), the untouched bytes around a caller's image checked"""
    h, w = frame.height, frame.width
    if mode == "host":
        wide = np.full((h, w + 2), 0x5A, dtype)
        labels, infos, stats = eng.segment(frame, p, dtype, host_out=wide[:, :w])
        assert labels.ctypes.data == wide.ctypes.data and (wide[:, w:] == 0x5A).all(), (name, mode)
        return np.ascontiguousarray(labels), infos, stats
    if mode == "device":
        keep, ptr, stride, nbytes = device_image(frame, dtype)
        img, infos, stats = eng.segment(frame, p, dtype, device_out=(ptr, stride))
        assert img.data == ptr and img.row_stride_bytes == stride
        labels, pad = image_of(img, frame, dtype)
        assert (pad == SENTINEL).all(), (name, mode)
        whole = keep.cpu().numpy()
        off = ptr - keep.data_ptr()
        assert (whole[:off] == SENTINEL).all() and (whole[off + nbytes:] == SENTINEL).all(), (name, mode)
        return labels, infos, stats
    img, infos, stats = eng.segment(frame, p, dtype, device_out=True)
    assert img.row_stride_bytes == w * np.dtype(dtype).itemsize
    return image_of(img, frame, dtype)[0], infos, stats


MODES = ("host", "device", "engine")
DTYPES = (np.uint8, np.uint16)


def check(eng, frame, image, p, name, combos):
    """combos: (source, mode, dtype) triples; every one == haf_segment_ref"""
    want = {dt: capi.segment_ref(frame, p, dt) for dt in {c[2] for c in combos}}
    dev = device_copy(frame, image) if any(c[0] == "device" for c in combos) else None
    for source, mode, dtype in combos:
        got = segment_into(eng, dev if source == "device" else frame, p, dtype, mode, name)
        w = want[dtype]
        bad = np.flatnonzero(got[0].reshape(-1) != w[0].reshape(-1))
        assert bad.size == 0 and got[2] == w[2] and len(got[1]) == len(w[1]), (name, source, mode, dtype.__name__, bad[:5], got[2], w[2])
        assert got[1].tobytes() == w[1].tobytes(), (name, source, mode, got[1][:3], w[1][:3])


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernels_equal_the_host_definition_word_for_word(eng, kind, shape):
    """every pattern and pose of this kind (one instance of the tile kernel) on this shape: a host and a device-resident frame each into
    one kind of output and one element size per case, all twelve combinations within any six consecutive cases; the first random case
    into all of them"""
    cases = [c for c in sc.small_cases([shape]) if "_%s_" % kind in c[0]]
    assert len(cases) >= 12
    for j, (name, frame, image, kw) in enumerate(cases):
        p = capi.segment_params(**kw)
        combos = [(src, MODES[(i + j) % 3], DTYPES[(i + j // 3) % 2]) for i, src in enumerate(("host", "device"))]
        if j == 0:
            assert name.startswith("random")
            combos = [(s, m, d) for s in ("host", "device") for m in MODES for d in DTYPES]
        check(eng, frame, image, p, name, combos)


def test_ties_and_caps(eng):
    for name, frame, image, kw, want in sc.tie_cases():
        p = capi.segment_params(**kw)
        assert (capi.segment_ref(frame, p)[0] == want).all(), name
        check(eng, frame, image, p, name, [("host", "host", np.uint8), ("device", "engine", np.uint16)])
    for name, frame, image, kw, dtype, n_labels, passing in sc.checker_cap_cases():
        p = capi.segment_params(**kw)
        labels, infos, stats = eng.segment(frame, p, dtype)
        assert len(infos) == n_labels and stats[3] == passing and int(labels.max()) == n_labels, (name, stats)
        check(eng, frame, image, p, name, [("host", "engine", dtype), ("device", "device", dtype)])


@pytest.mark.parametrize("case", [0, 1], ids=["all_foreground", "random_tilted"])
def test_vga(eng, case):
    """the one 640 x 480: one component of 307 200 pixels through all 1 200 tiles; ragged components that cross many seams"""
    name, frame, image, kw = sc.vga_cases()[case]
    p = capi.segment_params(**kw)
    want = capi.segment_ref(frame, p, np.uint16)
    if case == 0:
        assert want[2] == [307200, 307200, 1, 1] and want[1]["n_pixels"][0] == 307200
    else:
        assert want[2][3] > 200 and want[2][2] > want[2][3]
    check(eng, frame, image, p, name, [("host", "host", np.uint16), ("device", "engine", np.uint8), ("host", "device", np.uint16)])


@pytest.fixture(scope="module")
def table1_frame(data_dir):
    da = render_depth(pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd")), CAM_A)
    return capi.depth_frame(da, sensor_to_base=CAM_A, **K525), da


def test_segmented_image_composes_with_roi_scoring_and_the_label_map(data_dir, surrogate, table1_frame):
    """segment into the engine's device image; haf_score_frames_roi under that image as the device mask == under the host mask
    segment_ref != 0; haf_grasp_map_labels on the same device image afterwards == haf_label_best_ref on segment_ref's labels"""
    fa, da = table1_frame
    p = capi.segment_params(**TABLE1_PARAMS)
    ref_labels, ref_infos, ref_stats = capi.segment_ref(fa, p)
    n = len(ref_infos)
    assert n >= 2 and ref_stats[3] == n and (ref_infos["n_pixels"] >= 50).all()      # (13 objects: the test is not vacuous)
    e = make_engine(data_dir, surrogate, max_points=1 << 20, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    img, infos, stats = e.segment(fa, p, device_out=True)
    assert infos.tobytes() == ref_infos.tobytes() and stats == ref_stats
    a_out = e.score_frames_roi([fa], [(img.data, img.row_stride_bytes)], [inp])[0]
    a = snapshot(e, a_out)
    got = e.best_per_label(0, fa, img, n_labels=n)           # the engine's image is still there, behind a scoring call
    assert (image_of(img, fa, np.uint8)[0] == ref_labels).all()
    want = capi.label_best_ref(e.cfg, inp, 0, engine_grids(e, 0, 0, 20), fa, ref_labels, n_labels=n)
    assert all((got["picks"][f] == want["picks"][f]).all() for f in capi.LABEL_PICK_DTYPE.names) and got["order"] == want["order"]
    assert len(got["order"]) >= 2 and a_out["n_evals"] > 0
    b = snapshot(e, e.score_frames_roi([fa], [(ref_labels != 0).astype(np.uint8)], [inp])[0])
    assert_same(a, b)
    host = e.best_per_label(0, fa, ref_labels, n_labels=n)
    assert (host["picks"] == got["picks"]).all() and host["order"] == got["order"] and host["poses"] == got["poses"]
    e.close()


def test_filtered_frame_segments_like_the_host_filtered_one(data_dir, surrogate, table1_frame):
    """haf_filter_depth's engine image goes straight into haf_segment_frame: the labels of haf_segment_ref on haf_filter_depth_ref's image"""
    fa, da = table1_frame
    fp = capi.depth_filter()
    filtered, _ = capi.filter_depth_ref([fa], fp)
    p = capi.segment_params(**TABLE1_PARAMS)
    want = capi.segment_ref(capi.depth_frame(filtered, sensor_to_base=CAM_A, **K525), p, np.uint16)
    assert len(want[1]) >= 2
    e = make_engine(data_dir, surrogate, max_points=1 << 20)
    frame, _ = e.filter_depth([fa], fp)
    assert frame.on_device == 1
    got = e.segment(frame, p, np.uint16)
    assert sc.same(got, want)
    img, infos, stats = e.segment(frame, p, np.uint16, device_out=True)
    assert (image_of(img, fa, np.uint16)[0] == want[0]).all() and infos.tobytes() == want[1].tobytes() and stats == want[2]
    e.close()


def test_segment_leaves_the_last_batch_alone_and_needs_none(data_dir, golden_dir, surrogate, tmp_path, table1_frame):
    import json
    import models
    fa, da = table1_frame
    p = capi.segment_params(**TABLE1_PARAMS)
    want = capi.segment_ref(fa, p)
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    assert sc.same(e.segment(fa, p), want)                   # a fresh engine, before any request
    inp = capi.default_input(**C3_IN)
    out = e.score_frames([fa], [inp])[0]
    before, map_before = full_state(e, out), e.grasp_map(0, fa)
    xyz = capi.xyz_frame(np.ascontiguousarray(capi.frame_points(capi.depth_frame(da, **K525)).reshape(480, 640, 3)), sensor_to_base=CAM_A)
    for frame, kw in ((fa, {}), (device_copy(fa, da), dict(device_out=True)), (xyz, dict(dtype=np.uint16)), (fa, dict(device_out=True))):
        e.segment(frame, p, **kw)
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
    assert sc.same(e.segment(fa, p), want)
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code and a text that names the call, writes nothing and leaves the engine usable: the next valid call
    gives the right image"""
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    frame, image, kw = sc.make_case("random", "u16", (61, 5), True)
    p = capi.segment_params(**kw)
    want = capi.segment_ref(frame, p)
    canvas = np.full((64, 80), 0x77, np.uint8)

    def refused(fr, params, code, out=canvas, elem=1, stride=80, on_device=0, n_ptr=True):
        info = np.full(8, -7, capi.SEGMENT_INFO_DTYPE)
        n, st, oi = C.c_int32(-7), (C.c_int64 * 4)(-7, -7, -7, -7), capi.LabelImage()
        rc = L.haf_segment_frame(h, C.byref(fr) if fr is not None else None, C.byref(params) if params is not None else None,
                                 out.ctypes.data if isinstance(out, np.ndarray) else out, elem, stride, on_device, C.byref(oi), info.ctypes.data,
                                 C.byref(n) if n_ptr else None, st)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text.startswith("haf_segment_frame: "), (rc, code, text)
        assert n.value == -7 and list(st) == [-7] * 4 and oi.data is None and (info["n_pixels"] == -7).all() and (canvas == 0x77).all()
        assert sc.same(e.segment(frame, p), want)
        return text

    for name, over, elem in segment_refusals():
        refused(frame, capi.segment_params(**dict(kw, **over)), A, elem=elem, stride=160)
    for name, fr, code, _ in fc.refusal_frames():
        refused(fr, p, code)
    refused(None, p, A)
    refused(frame, None, A)
    refused(frame, p, A, n_ptr=False)
    assert L.haf_segment_frame(None, C.byref(frame), C.byref(p), canvas.ctypes.data, 1, 80, 0, None, None, C.byref(C.c_int32()), None) == A
    refused(frame, p, A, on_device=2)
    refused(frame, p, A, on_device=-1)
    refused(frame, p, A, out=None)                                           # no host image
    refused(frame, p, A, stride=60)                                          # 61 labels need 61 bytes
    refused(frame, p, A, elem=2, stride=120)
    refused(frame, p, A, elem=2, stride=123)
    refused(frame, p, A, elem=2, out=canvas.ctypes.data + 1, stride=160)
    refused(frame, p, A, out=image.ctypes.data, stride=128)                  # labels is the frame
    big = capi.depth_frame(np.ones((64, 65), np.uint16), **K525)             # 4160 pixels > max_points
    assert "max_points" in refused(big, p, CAP)
    assert "max_points" in refused(big, p, CAP, out=None, on_device=1)
    e.close()


def test_server_and_cli_without_a_segmenter(data_dir, surrogate, tmp_path, table1_frame):
    """CalcGraspPointsServer.execute_frame_segmented == execute_frame_objects on segment_ref's labels; haf_grasp_cli --segment writes
    segment_ref's image (--labels-out, read back as an 8-bit PGM), prints the objects the Python path finds, and with --segment-roi the
    restricted request's result; the default plane passes through the goal's centre"""
    import subprocess
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import _files
    from test_labels_gpu import assert_object_lines, engine_objects
    fa, da = table1_frame
    f_, r_ = _files(data_dir)
    p = capi.segment_params(**TABLE1_PARAMS)
    ref_labels, ref_infos, ref_stats = capi.segment_ref(fa, p)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    want_res, want_objects = srv.execute_frame_objects(goal, fa, ref_labels)
    res, objects = srv.execute_frame_segmented(goal, fa, p)
    assert res == want_res and objects == want_objects and len(objects) >= 2
    assert srv.last_segment_stats == ref_stats and srv.last_segment_infos.tobytes() == ref_infos.tobytes()
    auto = srv.segment_params_from_goal(goal, min_height=0.03)                # the plane through the centre, normal (0, 0, 1): the same plane
    assert list(auto.plane) == [0.0, 0.0, 1.0, 0.0]
    assert srv.execute_frame_segmented(goal, fa, auto) == (res, objects)
    tilted = srv.segment_params_from_goal(GraspInputMsg(grasp_area_center=(0.1, 0.2, 0.3), approach_vector=(0.0, 3.0, 4.0)))
    np.testing.assert_allclose(list(tilted.plane), [0.0, 0.6, 0.8, -0.36], rtol=1e-6)
    # the command line
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pa, pl = str(tmp_path / "a.pgm"), str(tmp_path / "labels.pgm")
    fc.write_pgm16(pa, da)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % x for x in CAM_A]
    plain = subprocess.run(common, check=True, capture_output=True, text=True).stdout
    seg = ["--segment", "0.03,0,0.02,50"]
    run = subprocess.run(common + seg + ["--labels-out", pl], check=True, capture_output=True, text=True)
    with open(pl, "rb") as f:
        raw = f.read()
    head = b"P5\n640 480\n255\n"
    assert raw.startswith(head) and (np.frombuffer(raw[len(head):], np.uint8).reshape(480, 640) == ref_labels).all()
    assert "segmented: %d object(s); %d of %d pixels foreground, %d component(s), %d pass the size rule" % \
        (len(ref_infos), ref_stats[1], ref_stats[0], ref_stats[2], ref_stats[3]) in run.stderr
    assert run.stdout.startswith(plain)
    srv.execute_frame(goal, fa)
    assert_object_lines(run.stdout[len(plain):].splitlines(), engine_objects(srv.engine, fa, ref_labels), 1, "--segment")
    same_plane = subprocess.run(common + seg + ["--plane", "0", "0", "1", "0"], check=True, capture_output=True, text=True).stdout
    assert same_plane == run.stdout
    roi = subprocess.run(common + seg + ["--segment-roi"], check=True, capture_output=True, text=True).stdout.splitlines()
    srv.execute_frame_segmented(goal, fa, p)
    assert int([ln for ln in roi if not ln.startswith("object ")][-1].split()[0]) == res.eval
    assert_object_lines([ln for ln in roi if ln.startswith("object ")], engine_objects(srv.engine, fa, ref_labels), 1, "--segment-roi")
    srv.close()
    bad = subprocess.run(common + ["--segment", "0.03,0,-1,50"], capture_output=True, text=True)
    assert bad.returncode == 1 and "max_gap" in bad.stderr
    assert subprocess.run(common + ["--segment", "0.03,0"], capture_output=True, text=True).returncode == 2                 # usage
    assert subprocess.run(common + ["--segment-roi"], capture_output=True, text=True).returncode == 2
