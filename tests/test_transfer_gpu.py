"""haf_transfer_labels on the MI355X (include/hafgrasp.h; csrc/transfer.hip): the kernels against haf_transfer_labels_ref word for word --
labels, z-buffer and stats -- on every case of transfer_cases: frames of all three kinds, host and device-resident with groups that
are not 16-byte aligned, host and device-resident camera label images, uint8 and uint16 on both sides, into host memory, into the
caller's padded device image and into the engine's own; the contention shapes; the rendered table1 scene with the second camera's
labels; the composition with haf_measure_labels and haf_score_objects; the engine's state; the shared image; the refusals; the
labelled chain of the Python server.  Every comparison is an equality.  Testing build, the guard zones checked inside every call and
after every test."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_cases as fc
import pcdio
import transfer_cases as tc
from haf_grasping_amd import capi
from test_depth_filter_gpu import SENTINEL, device_image
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, device_copy, make_engine, render_depth
from test_grasp_map_gpu import full_state
from test_segment_gpu import image_of
from test_transfer_cpu import camera_with, out_dtypes, transfer_refusals
from test_views_gpu import CAM_A, CAM_B

pytestmark = pytest.mark.gpu

CASES = tc.cases()
MODES = ("host", "device", "engine")
TABLE1_KW = dict(plane=[0, 0, 1, 0], min_height=0.03)


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


def device_labels(labels):
    """a camera label image in device memory, its rows as far apart as on the host -> a tensor view label_image() takes"""
    import torch
    h, w = labels.shape
    stride = labels.strides[0] // labels.itemsize if h > 1 else w
    wide = np.zeros((h, stride), labels.dtype)
    wide[:, :w] = labels
    t = torch.from_numpy(wide.view(np.int16) if labels.dtype == np.uint16 else wide).cuda()
    torch.cuda.synchronize()
    return t[:, :w]


def transfer_into(eng, frame, cam, cam_labels, n, p, dtype, mode, name):
    """one call into one kind of output -> (labels, stats, zbuffer), the untouched bytes around a caller's image checked"""
    h, w = frame.height, frame.width
    if mode == "host":
        wide = np.full((h, w + 2), 0x5A, dtype)
        got = eng.transfer_labels(frame, cam, cam_labels, n, p, dtype, host_out=wide[:, :w], zbuffer=True)
        assert got[0].ctypes.data == wide.ctypes.data and (wide[:, w:] == 0x5A).all(), (name, mode)
        return (np.ascontiguousarray(got[0]),) + got[1:]
    if mode == "device":
        keep, ptr, stride, nbytes = device_image(frame, dtype)
        got = eng.transfer_labels(frame, cam, cam_labels, n, p, dtype, device_out=(ptr, stride), zbuffer=True)
        img = got[0]
        assert img.data == ptr and img.row_stride_bytes == stride
        labels, pad = image_of(img, frame, dtype)
        assert (pad == SENTINEL).all(), (name, mode)
        whole = keep.cpu().numpy()
        off = ptr - keep.data_ptr()
        assert (whole[:off] == SENTINEL).all() and (whole[off + nbytes:] == SENTINEL).all(), (name, mode)
        return (labels,) + got[1:]
    got = eng.transfer_labels(frame, cam, cam_labels, n, p, dtype, device_out=True, zbuffer=True)
    assert got[0].row_stride_bytes == w * np.dtype(dtype).itemsize
    return (image_of(got[0], frame, dtype)[0],) + got[1:]


def check(eng, case, combos):
    """combos: (frame source, label source, mode, dtype); every one == haf_transfer_labels_ref"""
    name, frame, image, cam, labels, n_labels, kw = case
    p = capi.transfer_params(**kw)
    want = {dt: capi.transfer_labels_ref(frame, cam, labels, n_labels, p, dt, zbuffer=True) for dt in {c[3] for c in combos}}
    dev = device_copy(frame, image) if any(c[0] == "device" for c in combos) else None
    dlab = device_labels(labels) if any(c[1] == "device" for c in combos) else None
    for fsrc, lsrc, mode, dtype in combos:
        got = transfer_into(eng, dev if fsrc == "device" else frame, cam, dlab if lsrc == "device" else labels, n_labels, p, dtype, mode, name)
        w = want[dtype]
        bad = np.flatnonzero(got[0].reshape(-1) != w[0].reshape(-1))
        assert bad.size == 0 and got[1] == w[1], (name, fsrc, lsrc, mode, dtype.__name__, bad[:5], got[1], w[1])
        assert tc.same(got, w), (name, fsrc, lsrc, mode)


def all_combos(n_labels):
    dts = out_dtypes(n_labels)
    return [(f, l, m, dts[(i + j + k) % len(dts)]) for i, f in enumerate(("host", "device")) for j, l in enumerate(("host", "device"))
            for k, m in enumerate(MODES)]


def combos_for(j, n_labels):
    dts = out_dtypes(n_labels)
    return [(f, ("host", "device")[(i + j) % 2], MODES[(i + j) % 3], dts[(i + j // 2) % len(dts)]) for i, f in enumerate(("host", "device"))]


@pytest.mark.parametrize("j", range(len(CASES)), ids=[c[0] for c in CASES])
def test_kernels_equal_the_host_definition(eng, j):
    """a host and a device-resident frame each into one kind of output per case; the kinds' cases, the hostile points and the contention
    shapes into every combination"""
    case = CASES[j]
    wide = case[0].startswith(("kind_", "hostile", "contention", "window"))
    check(eng, case, all_combos(case[5]) if wide else combos_for(j, case[5]))


@pytest.fixture(scope="module")
def table1(data_dir):
    """the rendered scene from the first camera, and an instance image in the SECOND camera's view: that view's own segmentation"""
    cloud = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    da, db = render_depth(cloud, CAM_A), render_depth(cloud, CAM_B)
    fa, fb = capi.depth_frame(da, sensor_to_base=CAM_A, **K525), capi.depth_frame(db, sensor_to_base=CAM_B, **K525)
    labels_b, infos, _ = capi.segment_ref(fb, capi.segment_params(**TABLE1_KW))
    assert len(infos) >= 2
    cam = capi.camera(640, 480, K525["fx"], K525["fy"], K525["cx"], K525["cy"], sensor_to_base=CAM_B)
    return fa, da, cam, labels_b, len(infos)


def test_rendered_table1_with_the_second_cameras_labels(eng, table1):
    fa, da, cam, labels_b, n = table1
    want = capi.transfer_labels_ref(fa, cam, labels_b, n, zbuffer=True)
    assert want[1][4] > 1000 and len(np.unique(want[0])) >= 3 and want[1][3] < want[1][2]      # objects arrive, and something is hidden
    case = ("table1_rendered", fa, da, cam, labels_b, n, {})
    check(eng, case, [("host", "host", "host", np.uint8), ("device", "device", "engine", np.uint16), ("host", "device", "device", np.uint8)])


def test_transfer_composes_with_measure_and_score_objects(data_dir, surrogate, table1):
    """transfer into the engine's image; haf_measure_labels and haf_score_objects on that image == the same calls on the reference's
    image uploaded by the caller, in every field"""
    import torch
    fa, da, cam, labels_b, n = table1
    ref, ref_stats = capi.transfer_labels_ref(fa, cam, labels_b, n)
    e = make_engine(data_dir, surrogate, max_points=1 << 20, max_clouds=4, **C3_CFG)
    img, stats = e.transfer_labels(fa, cam, labels_b, n, device_out=True)
    assert stats == ref_stats
    up = torch.from_numpy(ref).cuda()
    torch.cuda.synchronize()
    plane = TABLE1_KW["plane"]
    shapes = e.measure_labels(fa, img, n_labels=n, plane=plane)
    assert shapes.tobytes() == e.measure_labels(fa, up, n_labels=n, plane=plane).tobytes()
    assert shapes.tobytes() == capi.measure_labels_ref(fa, ref, n_labels=n, plane=plane).tobytes()
    base = capi.default_input(**C3_IN)
    todo = [(l + 1, capi.object_input(e.cfg, base, shapes[l], 4)[0]) for l in range(n) if shapes["found"][l]][:4]
    assert len(todo) >= 2
    a = e.score_objects(fa, img, n, [l for l, _ in todo], [i for _, i in todo])
    b = e.score_objects(fa, up, n, [l for l, _ in todo], [i for _, i in todo])
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3] and len(a[3]) >= 1
    assert (image_of(img, fa, np.uint8)[0] == ref).all()                      # the engine's image is still there, behind the scoring calls
    e.close()


def test_transfer_leaves_the_last_batch_alone_and_needs_none(data_dir, golden_dir, surrogate, tmp_path, table1):
    import json
    import models
    fa, da, cam, labels_b, n = table1
    want = capi.transfer_labels_ref(fa, cam, labels_b, n, zbuffer=True)
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    assert tc.same(e.transfer_labels(fa, cam, labels_b, n, zbuffer=True), want)              # a fresh engine, before any request
    out = e.score_frames([fa], [capi.default_input(**C3_IN)])[0]
    before, map_before = full_state(e, out), e.grasp_map(0, fa)
    for frame, lab, kw in ((fa, labels_b, {}), (device_copy(fa, da), device_labels(labels_b), dict(device_out=True)), (fa, labels_b, dict(dtype=np.uint16, zbuffer=True))):
        e.transfer_labels(frame, cam, lab, n, **kw)
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
    assert tc.same(e.transfer_labels(fa, cam, labels_b, n, zbuffer=True), want)
    e.close()


def test_the_engines_image_is_the_segmenters(eng, table1):
    """ONE image for the three calls: a segment() after a transfer replaces it, a transfer after a segment() replaces it; and the engine's
    image cannot be the camera's label image and the output at once"""
    fa, da, cam, labels_b, n = table1
    sp = capi.segment_params(**TABLE1_KW)
    seg_ref = capi.segment_ref(fa, sp)[0]
    tr_ref = capi.transfer_labels_ref(fa, cam, labels_b, n)[0]
    assert (seg_ref != tr_ref).any()
    img, _ = eng.transfer_labels(fa, cam, labels_b, n, device_out=True)
    assert (image_of(img, fa, np.uint8)[0] == tr_ref).all()
    seg, _, _ = eng.segment(fa, sp, device_out=True)
    assert seg.data == img.data and (image_of(seg, fa, np.uint8)[0] == seg_ref).all()
    img2, _ = eng.transfer_labels(fa, cam, labels_b, n, device_out=True)
    assert img2.data == seg.data and (image_of(img2, fa, np.uint8)[0] == tr_ref).all()
    cells, _, _ = eng.segment_cells(fa, capi.cell_segment_params(**TABLE1_KW), device_out=True)
    assert cells.data == img2.data
    # the engine's image as the camera's labels into a HOST output is fine; into the engine's image it is refused, and the image stays
    same_view = capi.camera(640, 480, K525["fx"], K525["fy"], K525["cx"], K525["cy"], sensor_to_base=CAM_A)
    img3, _ = eng.transfer_labels(fa, cam, labels_b, n, device_out=True)
    a = eng.transfer_labels(fa, same_view, img3, n)
    assert a[0].shape == (480, 640)
    with pytest.raises(capi.HafError) as err:
        eng.transfer_labels(fa, same_view, img3, n, device_out=True)
    assert err.value.code == capi.HAF_E_ARG and "own image" in str(err.value)
    assert (image_of(img3, fa, np.uint8)[0] == tr_ref).all()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code and a text that names the call, writes nothing and leaves the engine usable: the next valid call
    gives the right result"""
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    name, frame, image, cam, labels, n_labels, kw = tc.kind_cases()[0]       # a padded 23 x 11 frame into a padded 31 x 17 uint8 image
    p = capi.transfer_params(**kw)
    want = capi.transfer_labels_ref(frame, cam, labels, n_labels, p, zbuffer=True)
    img, n = capi.label_image(labels, cam, n_labels)
    canvas = np.full((72, 64), 0x77, np.uint8)
    zb = np.full((64, 65), -7, np.int32)

    def refused(code, fr=frame, c=cam, li=img, nl=n, par=p, out=canvas, elem=1, stride=64, on_device=0):
        st, oi = (C.c_int64 * 5)(*[-7] * 5), capi.LabelImage()
        rc = L.haf_transfer_labels(h, C.byref(fr) if fr is not None else None, C.byref(c) if c is not None else None,
                                   C.byref(li) if li is not None else None, nl, C.byref(par) if par is not None else None,
                                   out.ctypes.data if isinstance(out, np.ndarray) else out, elem, stride, on_device, C.byref(oi), zb.ctypes.data, st)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text.startswith("haf_transfer_labels: "), (rc, code, text)
        assert list(st) == [-7] * 5 and oi.data is None and (canvas == 0x77).all() and (zb == -7).all()
        assert tc.same(e.transfer_labels(frame, cam, labels, n_labels, p, zbuffer=True), want)
        return text

    for rname, cover, pover in transfer_refusals():
        refused(A, c=camera_with(cam, cover), par=capi.transfer_params(**dict(kw, **pover)))
    for rname, fr, code, _ in fc.refusal_frames():
        refused(code, fr=fr)
    refused(A, fr=None)
    refused(A, c=None)
    refused(A, li=None)
    refused(A, par=None)
    assert L.haf_transfer_labels(None, C.byref(frame), C.byref(cam), C.byref(img), n, C.byref(p), canvas.ctypes.data, 1, 64, 0, None, None, None) == A
    refused(A, on_device=2)
    refused(A, out=None)                                                     # no host image
    refused(A, elem=3)
    refused(A, stride=22)                                                    # 23 labels need 23 bytes
    refused(A, elem=2, stride=47)
    refused(A, elem=2, out=canvas.ctypes.data + 1, stride=64)
    refused(A, out=image.ctypes.data, stride=64)                             # labels is the frame
    for over in (dict(data=None), dict(elem_bytes=3), dict(on_device=2), dict(row_stride_bytes=30)):
        li = capi.LabelImage.from_buffer_copy(img)
        for k, v in over.items():
            setattr(li, k, v)
        refused(A, li=li)
    for nl in (0, -1, 4097, 256):
        refused(A, nl=nl)                                                    # (256: a uint8 output holds 255 labels)
    own = np.zeros((17, 64), np.uint8)
    li, _ = capi.label_image(own[:, :31], cam, n_labels)
    refused(A, li=li, out=own.ctypes.data + 8)                               # the camera's label image overlaps the output
    big = capi.depth_frame(np.ones((65, 64), np.uint16), **K525)             # 4160 pixels > max_points
    assert "max_points" in refused(CAP, fr=big)
    assert "max_points" in refused(CAP, fr=big, out=None, on_device=1)
    big_cam = camera_with(cam, dict(width=65, height=64))
    big_labels, _ = capi.label_image(np.zeros((64, 65), np.uint8), big_cam, n_labels)
    assert "max_points" in refused(CAP, c=big_cam, li=big_labels)
    e.close()


def test_the_labelled_chain_of_the_server(data_dir, surrogate, table1):
    """CalcGraspPointsServer.execute_frame_labelled on the rendered scene == execute_frame_per_object(fused=True)'s chain fed with the
    same labels by hand: haf_transfer_labels_ref, haf_measure_labels_ref, haf_object_input and haf_score_objects in chunks"""
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg, GraspOutputMsg
    from test_frames_gpu import _files
    fa, da, cam, labels_b, n = table1
    f_, r_ = _files(data_dir)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, max_clouds=2, **C3_CFG)
    plane = TABLE1_KW["plane"]
    got = srv.execute_frame_labelled(goal, fa, cam, labels_b, n_labels=n, plane=plane, margin_cells=4)
    labels, stats = capi.transfer_labels_ref(fa, cam, labels_b, n)
    assert srv.last_transfer_stats == stats
    shapes = capi.measure_labels_ref(fa, labels, n_labels=n, plane=plane)
    assert srv.last_shapes.tobytes() == shapes.tobytes()
    cfg, base = srv.engine.cfg, goal.to_c()
    todo = [(l + 1,) + capi.object_input(cfg, base, shapes[l], 4) for l in range(n) if shapes["found"][l]]
    assert len(todo) > 2                                                     # more than one chunk of max_clouds
    hits = []
    for c0 in range(0, len(todo), 2):
        part = todo[c0:c0 + 2]
        _, picks, poses, _ = srv.engine.score_objects(fa, labels, n, [l for l, _, _ in part], [i for _, i, _ in part], min_vote=1)
        for b, (l, _, fits) in enumerate(part):
            if picks["found"][b]:
                c = poses[b]
                msg = GraspOutputMsg(srv.base_frame_id, c["eval"], c["grasp_point1"], c["grasp_point2"], c["averaged_grasp_point"],
                                     c["approach_vector"], c["roll"])
                key = (-int(picks["vote"][b]), int(picks["roll"][b]), int(picks["v"][b]) * fa.width + int(picks["u"][b]))
                hits.append((key, (l, msg, int(picks["u"][b]), int(picks["v"][b]), capi.shape_to_dict(shapes[l - 1]), fits)))
    want = [hit for _, hit in sorted(hits, key=lambda kh: kh[0])]
    assert len(got) >= 2 and got == want
    for label, msg, u, v, shape, fits in got:
        assert labels[v, u] == label
    srv.close()


def test_the_command_line_transfers_in_front_of_measure_and_per_object(data_dir, surrogate, tmp_path, table1):
    """haf_grasp_cli --labels F.pgm --labels-camera ... --labels-pose ...: --labels-out is the reference's image, --measure prints the
    shapes of that image, --per-object --fused prints one line per object of execute_frame_labelled's list"""
    import subprocess
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import _files
    fa, da, cam, labels_b, n = table1
    f_, r_ = _files(data_dir)
    ref, _ = capi.transfer_labels_ref(fa, cam, labels_b, n)
    plane = TABLE1_KW["plane"]
    shapes = capi.measure_labels_ref(fa, ref, n_labels=n, plane=plane)
    pd, pl, po = str(tmp_path / "depth.pgm"), str(tmp_path / "cam_labels.pgm"), str(tmp_path / "labels.pgm")
    fc.write_pgm16(pd, da)
    with open(pl, "wb") as f:
        f.write(b"P5\n640 480\n255\n" + labels_b.tobytes())
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    head = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
            "--search-size", "42", "42", "--depth", pd, "--intrinsics", "525", "525", "319.5", "239.5", "--sensor-pose"] + ["%.9g" % x for x in CAM_A] + \
           ["--labels", pl, "--labels-camera", "525", "525", "319.5", "239.5", "--labels-pose"] + ["%.9g" % x for x in CAM_B] + ["--plane", "0", "0", "1", "0"]
    run = subprocess.run(head + ["--measure", "--labels-out", po], check=True, capture_output=True, text=True)
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("shape ")]
    assert len(lines) == n, (run.stdout, run.stderr)
    for l, t in enumerate(lines):
        assert [int(t[1]), int(t[3]), int(t[5]), int(t[7])] == [l + 1, shapes["found"][l], shapes["n_pixels"][l], shapes["n_points"][l]], t
    with open(po, "rb") as f:
        raw = f.read()
    assert raw.startswith(b"P5\n640 480\n255\n") and (np.frombuffer(raw[15:], np.uint8).reshape(480, 640) == ref).all()
    assert "labels transferred" in run.stderr
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, max_clouds=4, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    want = srv.execute_frame_labelled(goal, fa, cam, labels_b, n_labels=n, plane=plane, margin_cells=4)
    srv.close()
    run = subprocess.run(head + ["--per-object", "4", "--fused"], check=True, capture_output=True, text=True)
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("object ")]
    assert len(lines) == len(want) >= 2, (run.stdout, run.stderr)
    for t, (label, msg, u, v, shape, fits) in zip(lines, want):
        assert [int(x) for x in t[1:5]] == [label, u, v, msg.eval], t
    assert subprocess.run(head[:-5] + ["--transfer", "0.05,0.01"], capture_output=True, text=True).returncode == 2      # usage
