"""haf_segment_cells on the MI355X (include/hafgrasp.h; csrc/cellsegment.hip): the kernels against haf_segment_cells_ref word for word
-- labels, infos, cell_labels, n_labels and stats -- on every case of cell_segment_cases: grids around and beyond a 64 x 16 tile with
components through every kind of seam, N x 1 clouds and frames of all three kinds, host and device-resident, uint8 and uint16, into
host memory, into the caller's padded device image and into the engine's own; the rendered table1 scene on the default grid; scratch
that grows; the composition with haf_score_frames_roi and haf_grasp_map_labels; the engine's state; the refusals; the cloud chain of
the Python server.  Every comparison is an equality.  Testing build, the guard zones checked inside every call and after every test."""
import ctypes as C
import os

import numpy as np
import pytest

import cell_segment_cases as cc
import frame_cases as fc
import pcdio
from haf_grasping_amd import capi
from test_depth_filter_gpu import SENTINEL, device_image
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, assert_same, device_copy, make_engine, render_depth, snapshot
from test_grasp_map_gpu import engine_grids, full_state
from test_cell_segment_cpu import cell_refusals
from test_segment_gpu import image_of
from test_views_gpu import CAM_A

pytestmark = pytest.mark.gpu

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


def cells_into(eng, frame, p, dtype, mode, name, grid=True):
    """one call into one kind of output -> (labels, infos, stats, cell_labels), the untouched bytes around a caller's image checked"""
    h, w = frame.height, frame.width
    if mode == "host":
        wide = np.full((h, w + 2), 0x5A, dtype)
        got = eng.segment_cells(frame, p, dtype, host_out=wide[:, :w], cell_labels=grid)
        assert got[0].ctypes.data == wide.ctypes.data and (wide[:, w:] == 0x5A).all(), (name, mode)
        return (np.ascontiguousarray(got[0]),) + got[1:]
    if mode == "device":
        keep, ptr, stride, nbytes = device_image(frame, dtype)
        got = eng.segment_cells(frame, p, dtype, device_out=(ptr, stride), cell_labels=grid)
        img = got[0]
        assert img.data == ptr and img.row_stride_bytes == stride
        labels, pad = image_of(img, frame, dtype)
        assert (pad == SENTINEL).all(), (name, mode)
        whole = keep.cpu().numpy()
        off = ptr - keep.data_ptr()
        assert (whole[:off] == SENTINEL).all() and (whole[off + nbytes:] == SENTINEL).all(), (name, mode)
        return (labels,) + got[1:]
    got = eng.segment_cells(frame, p, dtype, device_out=True, cell_labels=grid)
    assert got[0].row_stride_bytes == w * np.dtype(dtype).itemsize
    return (image_of(got[0], frame, dtype)[0],) + got[1:]


MODES = ("host", "device", "engine")
DTYPES = (np.uint8, np.uint16)


def check(eng, frame, image, p, name, combos):
    """combos: (source, mode, dtype) triples; every one == haf_segment_cells_ref"""
    want = {dt: capi.segment_cells_ref(frame, p, dt, cell_labels=True) for dt in {c[2] for c in combos}}
    dev = device_copy(frame, image) if any(c[0] == "device" for c in combos) else None
    for k, (source, mode, dtype) in enumerate(combos):
        got = cells_into(eng, dev if source == "device" else frame, p, dtype, mode, name, grid=k % 2 == 0)
        w = want[dtype]
        bad = np.flatnonzero(got[0].reshape(-1) != w[0].reshape(-1))
        assert bad.size == 0 and got[2] == w[2] and len(got[1]) == len(w[1]), (name, source, mode, dtype.__name__, bad[:5], got[2], w[2])
        assert got[1].tobytes() == w[1].tobytes(), (name, source, mode, got[1][:3], w[1][:3])
        assert cc.same(got, w), (name, source, mode)      # (with the label grid when this combination asked for one)


def combos_for(j, p):
    dts = DTYPES if p.max_labels <= 255 else (np.uint16,)
    return [(src, MODES[(i + j) % 3], dts[(i + j // 3) % len(dts)]) for i, src in enumerate(("host", "device"))]


@pytest.mark.parametrize("grid", cc.GRIDS, ids=lambda g: "%dx%d" % g)
def test_kernels_equal_the_host_definition_on_every_grid(eng, grid):
    """every pattern on this grid as a shuffled N x 1 cloud: a host and a device-resident frame each into one kind of output and one
    element size per case; the first case into all of them"""
    cases = cc.grid_cases([grid])
    assert len(cases) >= 3
    for j, (name, frame, image, kw) in enumerate(cases):
        p = capi.cell_segment_params(**kw)
        combos = combos_for(j, p)
        if j == 0:
            combos = [(s, m, np.uint16) for s in ("host", "device") for m in MODES]
        check(eng, frame, image, p, name, combos)


def test_rules_frames_and_lines(eng):
    """the rules one at a time; frames of all three kinds under both poses, 13 x 7 and a padded 61 x 5; N x 1 with N = 1, 63, 65, 1000"""
    for j, (name, frame, image, kw, want) in enumerate(cc.rule_cases()):
        p = capi.cell_segment_params(**kw)
        ref = capi.segment_cells_ref(frame, p)
        assert (len(ref[1]), ref[2][4], ref[2][5]) == want, (name, ref[2])
        check(eng, frame, image, p, name, combos_for(j, p))
    for j, (name, frame, image, kw) in enumerate(cc.frame_cases() + cc.line_cases()):
        p = capi.cell_segment_params(**kw)
        check(eng, frame, image, p, name, combos_for(j, p))


@pytest.fixture(scope="module")
def table1(data_dir):
    cloud = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    da = render_depth(cloud, CAM_A)
    return np.ascontiguousarray(cloud[:, :3], np.float32), capi.depth_frame(da, sensor_to_base=CAM_A, **K525), da


def test_rendered_table1_on_the_default_grid(eng, table1):
    """the one 640 x 480: the rendered scene, host and device-resident, and the same pixels as an organised XYZ frame"""
    xyz, fa, da = table1
    p = capi.cell_segment_params(**TABLE1_KW)
    want = capi.segment_cells_ref(fa, p, cell_labels=True)
    assert len(want[1]) >= 2 and want[2][2] == 0
    check(eng, fa, da, p, "table1_rendered", [("host", "host", np.uint8), ("device", "engine", np.uint16), ("host", "device", np.uint16)])
    pts = np.ascontiguousarray(capi.frame_points(capi.depth_frame(da, **K525)).reshape(480, 640, 3))
    got = eng.segment_cells(capi.xyz_frame(pts, sensor_to_base=CAM_A), p, cell_labels=True)
    assert cc.same(got, want)


def test_scratch_grows_with_the_grid_and_with_the_frame(data_dir, surrogate, table1):
    """a fresh engine: a 64 x 64 grid, then 1024 x 1024, then 64 x 64 again; a small frame, the 640 x 480 one, the small one again"""
    xyz, fa, da = table1
    e = make_engine(data_dir, surrogate, max_points=640 * 480)
    name, frame, image, kw = cc.line_cases()[3]
    for nx in (64, 1024, 64):
        p = capi.cell_segment_params(**dict(kw, nx=nx, ny=nx, x0=-0.32 if nx == 64 else -5.12, y0=-0.32 if nx == 64 else -5.12, cell=0.01))
        want = capi.segment_cells_ref(frame, p, np.uint16, cell_labels=True)
        assert want[2][5] >= 2
        assert cc.same(e.segment_cells(frame, p, np.uint16, cell_labels=True), want), nx
    e.close()
    e = make_engine(data_dir, surrogate, max_points=640 * 480)
    small = cc.frame_cases()[0]
    for fr, pp in ((small[1], capi.cell_segment_params(**small[3])), (fa, capi.cell_segment_params(**TABLE1_KW)), (small[1], capi.cell_segment_params(**small[3]))):
        assert cc.same(e.segment_cells(fr, pp, cell_labels=True), capi.segment_cells_ref(fr, pp, cell_labels=True))
    e.close()


def test_cells_image_composes_with_roi_scoring_and_the_label_map(data_dir, surrogate, table1):
    """cells into the engine's device image; haf_score_frames_roi under that image as the device mask == under the host mask ref != 0;
    haf_grasp_map_labels on the same device image afterwards == haf_label_best_ref on the reference's labels"""
    xyz, fa, da = table1
    p = capi.cell_segment_params(**TABLE1_KW)
    ref_labels, ref_infos, ref_stats = capi.segment_cells_ref(fa, p)
    n = len(ref_infos)
    assert n >= 2 and ref_stats[5] == n
    e = make_engine(data_dir, surrogate, max_points=1 << 20, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    img, infos, stats = e.segment_cells(fa, p, device_out=True)
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
    # the engine's image is ONE image for both segmenters: the pixel segmenter's next call takes it over
    seg, _, _ = e.segment(fa, capi.segment_params(plane=[0, 0, 1, 0], min_height=0.03), device_out=True)
    assert seg.data == img.data
    e.close()


def test_cells_leave_the_last_batch_alone_and_need_none(data_dir, golden_dir, surrogate, tmp_path, table1):
    import json
    import models
    xyz, fa, da = table1
    p = capi.cell_segment_params(**TABLE1_KW)
    want = capi.segment_cells_ref(fa, p)
    cloud = capi.cloud_frame(xyz)
    want_cloud = capi.segment_cells_ref(cloud, p, np.uint16)
    e = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    assert cc.same(e.segment_cells(fa, p), want)             # a fresh engine, before any request
    inp = capi.default_input(**C3_IN)
    out = e.score_frames([fa], [inp])[0]
    before, map_before = full_state(e, out), e.grasp_map(0, fa)
    for frame, kw in ((fa, {}), (device_copy(fa, da), dict(device_out=True)), (cloud, dict(dtype=np.uint16)), (fa, dict(device_out=True, cell_labels=True))):
        got = e.segment_cells(frame, p, **kw)
        assert frame is not cloud or cc.same(got, want_cloud)
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
    assert cc.same(e.segment_cells(fa, p), want)
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code and a text that names the call, writes nothing and leaves the engine usable: the next valid call
    gives the right result"""
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    name, frame, image, kw = cc.frame_cases()[7]             # a padded 61 x 5 frame
    assert frame.width == 61
    p = capi.cell_segment_params(**kw)
    want = capi.segment_cells_ref(frame, p)
    canvas = np.full((64, 80), 0x77, np.uint8)
    grid = np.full((1024, 1024), 0x7777, np.uint16)

    def refused(fr, params, code, out=canvas, elem=1, stride=80, on_device=0, n_ptr=True):
        info = np.full(8, -7, capi.CELL_SEGMENT_INFO_DTYPE)
        n, st, oi = C.c_int32(-7), (C.c_int64 * 6)(*[-7] * 6), capi.LabelImage()
        rc = L.haf_segment_cells(h, C.byref(fr) if fr is not None else None, C.byref(params) if params is not None else None,
                                 out.ctypes.data if isinstance(out, np.ndarray) else out, elem, stride, on_device, C.byref(oi), grid.ctypes.data,
                                 info.ctypes.data, C.byref(n) if n_ptr else None, st)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text.startswith("haf_segment_cells: "), (rc, code, text)
        assert n.value == -7 and list(st) == [-7] * 6 and oi.data is None and (info["n_points"] == -7).all() and (canvas == 0x77).all()
        assert (grid == 0x7777).all()
        assert cc.same(e.segment_cells(frame, p), want)
        return text

    for rname, over, elem in cell_refusals():
        refused(frame, capi.cell_segment_params(**dict(kw, **over)), A, elem=elem, stride=160)
    for rname, fr, code, _ in fc.refusal_frames():
        refused(fr, p, code)
    refused(None, p, A)
    refused(frame, None, A)
    refused(frame, p, A, n_ptr=False)
    assert L.haf_segment_cells(None, C.byref(frame), C.byref(p), canvas.ctypes.data, 1, 80, 0, None, None, None, C.byref(C.c_int32()), None) == A
    refused(frame, p, A, on_device=2)
    refused(frame, p, A, out=None)                                           # no host image
    refused(frame, p, A, stride=60)                                          # 61 labels need 61 bytes
    refused(frame, p, A, elem=2, stride=123)
    refused(frame, p, A, elem=2, out=canvas.ctypes.data + 1, stride=160)
    refused(frame, p, A, out=image.ctypes.data, stride=128)                  # labels is the frame
    big = capi.depth_frame(np.ones((64, 65), np.uint16), **K525)             # 4160 pixels > max_points
    assert "max_points" in refused(big, p, CAP)
    assert "max_points" in refused(big, p, CAP, out=None, on_device=1)
    e.close()


def test_the_cloud_chain_of_the_server_and_the_command_line(data_dir, surrogate, tmp_path, table1):
    """CalcGraspPointsServer.execute_cloud_per_object on table1.pcd == the same chain assembled by hand from segment_cells_ref,
    measure_labels_ref, object_input and haf_score_objects; it finds at least two objects; the frame route with segmenter="cells" on
    the same N x 1 frame is the same list; haf_grasp_cli --segment-cells with the .pcd prints the same "object" lines and writes the
    reference's two label images"""
    import subprocess
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    from test_frames_gpu import _files
    xyz, fa, da = table1
    f_, r_ = _files(data_dir)
    p = capi.cell_segment_params(**TABLE1_KW)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, max_clouds=4, **C3_CFG)
    got = srv.execute_cloud_per_object(goal, xyz, p, margin_cells=4)
    frame = capi.cloud_frame(xyz)
    labels, infos, stats, grid = capi.segment_cells_ref(frame, p, cell_labels=True)
    n = len(infos)
    assert srv.last_segment_infos.tobytes() == infos.tobytes() and srv.last_segment_stats == stats
    shapes = capi.measure_labels_ref(frame, labels, n_labels=n, plane=list(p.plane))
    assert srv.last_shapes.tobytes() == shapes.tobytes()
    cfg, base = srv.engine.cfg, goal.to_c()
    todo = [(l + 1,) + capi.object_input(cfg, base, shapes[l], 4) for l in range(n) if shapes["found"][l]]
    assert len(todo) > 4                                                      # more than one chunk of max_clouds
    hits = []
    for c0 in range(0, len(todo), 4):
        part = todo[c0:c0 + 4]
        _, picks, poses, _ = srv.engine.score_objects(frame, labels, n, [l for l, _, _ in part], [i for _, i, _ in part], min_vote=1)
        for b, (l, _, fits) in enumerate(part):
            if picks["found"][b]:
                hits.append(((-int(picks["vote"][b]), int(picks["roll"][b]), int(picks["u"][b])), l, poses[b], int(picks["u"][b]), int(picks["v"][b]), fits))
    hits.sort(key=lambda t: t[0])
    assert len(got) == len(hits) >= 2
    for (label, msg, u, v, shape, fits), (_, l, c, pu, pv, pf) in zip(got, hits):
        assert (label, u, v, fits) == (l, pu, pv, pf) and v == 0 and labels[0, u] == label
        assert (msg.eval, msg.graspPoint1, msg.graspPoint2, msg.approachVector, msg.roll) == (c["eval"], c["grasp_point1"], c["grasp_point2"], c["approach_vector"], c["roll"])
        assert shape == capi.shape_to_dict(shapes[label - 1])
    assert srv.execute_frame_per_object(goal, frame, p, fused=True, segmenter="cells") == got
    # the calls around the segmenter on a long N x 1 frame: the plane fit and the shapes equal their host definitions there, too
    fit, fit_ref = srv.engine.fit_plane(frame), capi.fit_plane_ref(frame)
    assert fit["found"] and all(fit[k] == fit_ref[k] for k in ("found", "winner", "n_inliers", "stats")), (fit, fit_ref)
    assert fit["plane"].tobytes() == fit_ref["plane"].tobytes()
    assert srv.engine.measure_labels(frame, labels, n_labels=n, plane=list(p.plane)).tobytes() == shapes.tobytes()
    with pytest.raises(ValueError):
        srv.execute_frame_per_object(goal, frame, p, segmenter="voxels")
    srv.close()
    # the command line
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pl, pg = str(tmp_path / "labels.pgm"), str(tmp_path / "grid.pgm")
    cmd = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
           "--search-size", "42", "42", "--segment-cells", "0.03,0,0.01,50", "--plane", "0", "0", "1", "0", "--per-object", "4", "--fused",
           "--labels-out", pl, "--cell-labels-out", pg, os.path.join(data_dir, TABLE1 + ".pcd")]
    run = subprocess.run(cmd, check=True, capture_output=True, text=True)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("object ")]
    assert len(lines) == len(got), (run.stdout, run.stderr)
    for line, (label, msg, u, v, shape, fits) in zip(lines, got):
        t = line.split()
        assert [int(x) for x in t[1:5]] == [label, u, v, msg.eval], line
        np.testing.assert_allclose([float(x) for x in t[5:11]], list(msg.graspPoint1) + list(msg.graspPoint2), rtol=1e-5, atol=1e-6)
    for path, want in ((pl, labels), (pg, grid)):
        with open(path, "rb") as f:
            raw = f.read()
        head = b"P5\n%d %d\n255\n" % (want.shape[1], want.shape[0])
        assert raw.startswith(head) and (np.frombuffer(raw[len(head):], np.uint8).reshape(want.shape) == want).all(), path
    assert "segmented by cells: %d object(s)" % n in run.stderr
    assert subprocess.run(cmd[:-1] + ["--segment-cells", "0.03,0"] + cmd[-1:], capture_output=True, text=True).returncode == 2      # usage
    bad = subprocess.run([a if a != "0.03,0,0.01,50" else "0.03,0,5,50" for a in cmd], capture_output=True, text=True)
    assert bad.returncode == 1 and "cell" in bad.stderr
