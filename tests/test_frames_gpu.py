"""haf_score_frames on the MI355X (include/hafgrasp.h: haf_frame): the deprojection kernel against haf_frame_points bit for bit, the
frames path against the cloud path on the same engine and against the CPU oracle, batches, the bucket-sorted binning path, the
engine-side refusals and the CLI.  Testing build throughout; the guard zones around every device buffer are checked after each test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import models
import pcdio
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import compare_full

pytestmark = pytest.mark.gpu

TABLE1, TABLE3 = "table1_mult_obj_rcs_1428580506606673", "table3_mult_obj_rcs_1428581033679923"
K525 = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)
C3_CFG = dict(n_rolls=20, roll_step_deg=9)
C3_IN = dict(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
DOWN = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)          # camera z along -z of the base frame: looking straight down


def _files(data_dir):
    return os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(scope="module")
def orc(data_dir, surrogate):
    f, r = _files(data_dir)
    return O.Oracle(f, r, surrogate)


@pytest.fixture(autouse=True)
def _canaries():
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


def make_engine(data_dir, model, flags=0, **cfg):
    f, r = _files(data_dir)
    return capi.Engine(f, r, model, testing=True, flags=capi.FLAG_KEEP_DEBUG | capi.FLAG_PROFILE | flags, **cfg)


def pose(rot, t):
    return np.concatenate([np.asarray(rot, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(-1)


def tilt(ax, ay, az):
    ca, sa, cb, sb, cc, sc = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx @ DOWN


def render_depth(xyz, sensor_to_base, width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    """A pinhole camera's 16UC1 image of a base-frame cloud: every point into the camera frame (the inverse of sensor_to_base), onto
    its nearest pixel, the nearest depth per pixel, in millimetres."""
    m = np.asarray(sensor_to_base, np.float64).reshape(3, 4)
    pc = (np.asarray(xyz, np.float64) - m[:, 3]) @ m[:, :3]
    pc = pc[np.isfinite(pc).all(axis=1) & (pc[:, 2] > 0.05)]
    u = np.rint(fx * pc[:, 0] / pc[:, 2] + cx).astype(np.int64)
    v = np.rint(fy * pc[:, 1] / pc[:, 2] + cy).astype(np.int64)
    mm = np.rint(pc[:, 2] * 1000.0).astype(np.int64)
    ok = (u >= 0) & (u < width) & (v >= 0) & (v < height) & (mm > 0) & (mm < 65536)
    img = np.full(width * height, 65536, np.int64)
    np.minimum.at(img, v[ok] * width + u[ok], mm[ok])
    img[img == 65536] = 0
    return img.astype(np.uint16).reshape(height, width)


def snapshot(eng, out, n_clouds=1):
    """everything the last batch left behind that a caller can read"""
    R, snap = eng.cfg.n_rolls, dict(out=out, tiers=eng.last_counts(), exact=eng.last_exact_tiers(), top=eng.top_grasps(k=16) if not (eng.cfg.flags & capi.FLAG_PROBABILITY) else None)
    for b in range(n_clouds):
        for r in range(R):
            ev, mask = eng.roll_grid(b, r)
            snap["grid", b, r] = (ev.tobytes(), mask.tobytes(), eng.debug(capi.DBG_HEIGHTS, b, r).tobytes())
    return snap


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k


def device_copy(frame, image):
    """the frame's pixels in device memory at the same address modulo 16, rows and points as far apart as on the host"""
    import torch
    last = 12 if frame.kind == capi.FRAME_XYZ_F32 else image.itemsize
    elem = frame.point_stride_bytes if frame.kind == capi.FRAME_XYZ_F32 else image.itemsize
    span = (frame.height - 1) * frame.row_stride_bytes + (frame.width - 1) * elem + last
    off = frame.data % 16
    host = np.zeros(off + span + 16, np.uint8)
    host[off:off + span] = np.frombuffer(C.string_at(frame.data, span), np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    g = capi.Frame.from_buffer_copy(frame)
    g.data, g.on_device = dev.data_ptr() + off, 1
    g._keep = dev
    return g


def kernel_cases():
    """every case family of the CPU suite, 640 x 480 with the base offset by one element (rows not 16-byte aligned), widths 1..17"""
    out = list(fc.cases())
    rng = np.random.default_rng(77)
    for name, make in (("u16", fc.u16_image), ("f32", fc.f32_image)):
        flat = np.zeros(640 * 480 + 9, np.uint16 if name == "u16" else np.float32)
        base = (-flat.ctypes.data % 16) // flat.itemsize + 1                 # one element past a 16-byte boundary
        img = flat[base:base + 640 * 480].reshape(480, 640)
        img[:] = make(rng, 640, 480)
        assert img.ctypes.data % 16 == img.itemsize
        out.append(("%s_640x480_offset_by_one_element" % name, capi.depth_frame(img, sensor_to_base=fc.tilted_pose(rng), **fc._intrinsics(rng, 640, 480)), img))
    for w in range(1, 18):
        h, pad = 1 + w % 5, (w % 3)
        for name, img in (("u16", fc.u16_image(rng, w, h)), ("f32", fc.f32_image(rng, w, h)), ("xyz", fc.xyz_image(rng, w, h, 3 + w % 2))):
            img = fc.padded(img, pad) if pad else img
            fr = capi.xyz_frame(img, sensor_to_base=fc.tilted_pose(rng)) if name == "xyz" else \
                capi.depth_frame(img, sensor_to_base=fc.tilted_pose(rng), **fc._intrinsics(rng, w, h))
            out.append(("%s_width%d" % (name, w), fr, img))
    return out


def test_kernel_equals_host_definition_bit_for_bit(data_dir, surrogate):
    """haf_debug_fetch_points after haf_score_frames == haf_frame_points, every word, host and device-resident sources"""
    eng = make_engine(data_dir, surrogate, max_points=640 * 480)
    inp = capi.default_input()
    seen = 0
    for name, frame, image in kernel_cases():
        want = fc.words(capi.frame_points(frame))
        assert (want == fc.mirror_points(frame, image)).all(), name
        for where, fr in (("host", frame), ("device", device_copy(frame, image))):
            eng.score_frames([fr], [inp])
            got = fc.words(eng.debug_points(0))
            bad = np.flatnonzero((got != want).any(axis=1))
            assert got.shape == want.shape and bad.size == 0, (name, where, bad[:5], got[bad[:5]], want[bad[:5]])
            seen += 1
    assert seen >= 2 * (28 + 2 + 51)
    # a staged host cloud is fetched the same way; a device-resident xyz cloud is not the engine's to return
    import torch
    xyz = np.random.default_rng(3).uniform(-0.2, 0.2, (1000, 4)).astype(np.float32)
    eng.score(xyz, inp)
    assert (fc.words(eng.debug_points(0)) == fc.words(xyz[:, :3])).all()
    dev = torch.from_numpy(xyz).cuda()
    torch.cuda.synchronize()
    eng.score((dev.data_ptr(), 1000, 4), inp)
    with pytest.raises(capi.HafError) as ei:
        eng.debug_points(0, 1000)
    assert ei.value.code == capi.HAF_E_ARG
    eng.score(xyz, inp)
    for args in ((1, 1000), (-1, 1000), (0, 999)):
        with pytest.raises(capi.HafError):
            eng.debug_points(*args)
    eng.close()
    plain = capi.Engine(*_files(data_dir), surrogate, testing=True)          # without HAF_FLAG_KEEP_DEBUG
    plain.score(xyz, inp)
    with pytest.raises(capi.HafError, match="KEEP_DEBUG"):
        plain.debug_points(0)
    plain.close()


RENDERED = [pytest.param(TABLE1, (0.13, 0.2, 0.9), None, C3_CFG, C3_IN, 20000, id="table1_down"),
            pytest.param(TABLE3, (0.13, 0.2, 0.9), None, C3_CFG, C3_IN, 20000, id="table3_down"),
            pytest.param(TABLE1, (0.20, 0.13, 0.9), (0.21, -0.17, 0.6), C3_CFG, C3_IN, 20000, id="table1_tilted"),
            pytest.param("pcd2", (0.0, 0.0, 0.8), None, dict(n_rolls=12), dict(grasp_area_length_x=32, grasp_area_length_y=32), 3000, id="pcd2_down"),
            pytest.param("pcd2", (0.05, -0.04, 0.8), (-0.15, 0.2, -1.1), dict(n_rolls=12), dict(grasp_area_length_x=32, grasp_area_length_y=32),
                         3000, id="pcd2_tilted")]


# the straight-down renderings as the CPU oracle scores them: (n_evals, eval, (row, col, roll), rolls above the hypothesis threshold)
ORACLE_FIGURES = {(TABLE1, None): (31093, 81, (44, 19, 7), 17), (TABLE3, None): (24641, 103, (15, 34, 2), 20), ("pcd2", None): (3761, 103, (28, 24, 0), None)}


@pytest.mark.parametrize("name,cam,angles,cfg_kw,in_kw,min_evals", RENDERED)
def test_frames_path_equals_cloud_path_equals_oracle(data_dir, surrogate, orc, name, cam, angles, cfg_kw, in_kw, min_evals):
    """A depth frame rendered from a golden cloud (640 x 480, f = 525, c = (319.5, 239.5), nearest depth per pixel in millimetres):
    haf_score_frames(frame) leaves exactly what haf_score_batch(cloud = haf_frame_points(frame)) leaves on the same engine, and that is
    what the oracle computes from those points."""
    xyz = pcdio.load_pcd(os.path.join(data_dir, name + ".pcd"))
    s2b = pose(DOWN if angles is None else tilt(*angles), cam)
    depth = render_depth(xyz, s2b)
    frame = capi.depth_frame(depth, sensor_to_base=s2b, **K525)
    pts = capi.frame_points(frame)
    assert np.isfinite(pts).all(axis=1).sum() > 2000
    eng = make_engine(data_dir, surrogate, max_points=1 << 19, **cfg_kw)
    inp = capi.default_input(**in_kw)
    got, want = compare_full(eng, orc, pts, cfg_kw, in_kw)
    print("rendered %s: n_evals %d eval %d best (%d, %d, %d)" % (name, got["n_evals"], got["eval"], got["best_row"], got["best_col"], got["best_roll"]))
    assert got["n_evals"] >= min_evals and got["eval"] > 50                  # the comparison cannot pass on empty grids
    if (name, angles) in ORACLE_FIGURES:
        n_evals, ev, best, above = ORACLE_FIGURES[name, angles]
        assert (got["n_evals"], got["eval"], (got["best_row"], got["best_col"], got["best_roll"])) == (n_evals, ev, best)
        assert above is None or sum(v[2] > eng.cfg.graspval_th for v in want["roll_best"]) == above
    cloud = snapshot(eng, got)
    out = eng.score_frames([frame], [inp])[0]
    assert (fc.words(eng.debug_points(0)) == fc.words(pts)).all()
    frames = snapshot(eng, out)
    assert_same(frames, cloud)
    # ... and once more against the oracle's grids directly, as compare_full does for the cloud path
    for roll in range(want["rolls_done"]):
        assert (eng.debug(capi.DBG_LABELS, 0, roll) == want["labels"][roll]).all()
        assert (eng.roll_grid(0, roll)[0] == want["graspseval"][roll]).all()
    assert (out["eval"], out["best_row"], out["best_col"], out["best_roll"]) == (want["eval"], want["row"], want["col"], want["roll_idx"])
    np.testing.assert_allclose(out["averaged_grasp_point"], want["avg"], atol=1e-4)
    # the same request as an F32 image in metres (z = (float)d * 0.001f formed here, scale 1) and as the organised sensor-frame cloud
    # with the pose (the camera-frame points are those of the identity pose): the same points, so the same everything
    metres = depth.astype(np.float32) * np.float32(0.001)
    cam_pts = capi.frame_points(capi.depth_frame(depth, **K525)).reshape(480, 640, 3)
    for other in (capi.depth_frame(metres, sensor_to_base=s2b, **K525), capi.xyz_frame(cam_pts, sensor_to_base=s2b)):
        assert_same(snapshot(eng, eng.score_frames([other], [inp])[0]), cloud)
    ms = eng.stage_ms()
    assert ms["upload"] > 0
    eng.close()


def test_batch_of_frames_equals_singles(data_dir, surrogate):
    """Frames of different kinds and sizes in one call == the same frames one by one (n_rechecked is counted per batch)"""
    xyz = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    s2b = pose(DOWN, (0.13, 0.2, 0.9))
    depth = render_depth(xyz, s2b)
    metres = (depth.astype(np.float32) * np.float32(0.001))
    crop = metres[60:440, 40:600]                                             # a view: rows 640 floats apart
    s2b_t = pose(tilt(0.1, -0.2, 0.4), (0.1, 0.22, 0.9))
    cam_pts = np.zeros((480, 640, 4), np.float32)                             # pcl::PointXYZ: 16-byte points
    cam_pts[:, :, :3] = capi.frame_points(capi.depth_frame(render_depth(xyz, s2b_t), **K525)).reshape(480, 640, 3)
    rng = np.random.default_rng(9)
    small = fc.u16_image(rng, 61, 5)
    host = [capi.depth_frame(depth, sensor_to_base=s2b, **K525),
            capi.depth_frame(crop, fx=525.0, fy=525.0, cx=319.5 - 40, cy=239.5 - 60, sensor_to_base=s2b, min_depth=0.3, max_depth=0.88),
            capi.xyz_frame(cam_pts, sensor_to_base=s2b_t),
            capi.depth_frame(small, sensor_to_base=fc.tilted_pose(rng), **fc._intrinsics(rng, 61, 5)),
            capi.depth_frame(depth, sensor_to_base=s2b_t, **K525)]
    frames = host[:4] + [device_copy(host[4], depth)]                        # the last one device-resident
    inputs = [capi.default_input(**C3_IN), capi.default_input(**dict(C3_IN, approach_vector=(0.1, -0.1, 1.0))), capi.default_input(**C3_IN),
              capi.default_input(), capi.default_input(**dict(C3_IN, show_only_best_grasp=1))]
    n = len(frames)
    eng = make_engine(data_dir, surrogate, max_clouds=n, max_points=4 * 640 * 480, **C3_CFG)
    outs = eng.score_frames(frames, inputs)
    assert sum(o["n_evals"] >= 20000 and o["eval"] > 50 for o in outs) >= 3
    batch = snapshot(eng, None, n)
    points = [eng.debug_points(b).tobytes() for b in range(n)]
    tops = eng.top_grasps(k=8)
    for b in range(n):
        o = eng.score_frames([frames[b]], [inputs[b]])[0]
        strip = lambda d: {k: v for k, v in d.items() if k != "n_rechecked"}
        assert strip(o) == strip(outs[b]), b
        assert eng.debug_points(0).tobytes() == points[b] == capi.frame_points(host[b]).tobytes(), b
        single = snapshot(eng, None)
        for r in range(eng.cfg.n_rolls):
            assert single["grid", 0, r] == batch["grid", b, r], (b, r)
        assert eng.top_grasps(k=8)[0] == tops[b], b
    eng.close()


def test_million_pixel_frame_on_the_bucket_sorted_binning_path(data_dir, tmp_path):
    """A seeded 1024 x 1024 F32 frame, a third of it NaN, on a 256 x 256 grid with 36 rolls: binning sorts the million points into
    spatial buckets (grids beyond LDS size), NaN points included.  Same result as the cloud path."""
    model = models.write_random_model(str(tmp_path / "m64.model"), 64, seed=5)
    rng = np.random.default_rng(31)
    n = 1024
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    relief = 0.06 * np.sin(xx / 37.0) * np.cos(yy / 53.0) + 0.05 * (rng.random((n, n)) < 0.02) + 0.004 * rng.random((n, n))
    depth = (2.0 - 0.08 - relief).astype(np.float32)
    depth[rng.random((n, n)) < 0.33] = np.nan
    s2b = pose(tilt(0.02, -0.03, 0.3), (0.01, -0.02, 2.0))
    frame = capi.depth_frame(depth, fx=800.0, fy=800.0, cx=511.5, cy=511.5, sensor_to_base=s2b)
    pts = capi.frame_points(frame)
    assert 0.6 < np.isfinite(pts).all(axis=1).mean() < 0.7
    eng = make_engine(data_dir, model, grid_h=256, grid_w=256, n_rolls=36, roll_step_deg=5, max_points=n * n)
    inp = capi.default_input(grasp_area_length_x=256, grasp_area_length_y=256)
    a = eng.score(pts, inp)
    assert a["n_evals"] > 1000000
    cloud = snapshot(eng, a)
    b = eng.score_frames([frame], [inp])[0]
    assert (fc.words(eng.debug_points(0)) == fc.words(pts)).all()
    assert_same(snapshot(eng, b), cloud)
    eng.close()


def test_engine_side_refusals_leave_the_engine_usable(data_dir, surrogate):
    """Every refusal of haf_score_frames returns its code and a text, before any device work; the next valid call is served as if nothing
    had happened."""
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=4096)
    L, h = eng._L, eng._h
    inp = capi.default_input()
    rng = np.random.default_rng(4)
    img = fc.u16_image(rng, 61, 5)
    good = capi.depth_frame(img, sensor_to_base=pose(DOWN, (0.0, 0.0, 0.9)), **fc._intrinsics(rng, 61, 5))
    ref = eng.score_frames([good], [inp])[0]
    ref_pts = eng.debug_points(0).tobytes()

    def refused(n, frames, inputs, out, code):
        rc = L.haf_score_frames(h, n, frames, inputs, out)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text, (rc, code, text)
        assert eng.score_frames([good], [inp])[0] == ref and eng.debug_points(0).tobytes() == ref_pts
        return text

    one, gi, out = (capi.Frame * 2)(good, good), (capi.GraspInput * 2)(inp, inp), (capi.GraspOutput * 2)()
    for args in ((1, None, gi, out), (1, one, None, out), (1, one, gi, None), (0, one, gi, out), (-3, one, gi, out)):
        refused(*args, capi.HAF_E_ARG)
    assert L.haf_score_frames(None, 1, one, gi, out) == capi.HAF_E_ARG
    three = (capi.Frame * 3)(good, good, good)
    assert "max_clouds" in refused(3, three, (capi.GraspInput * 3)(inp, inp, inp), (capi.GraspOutput * 3)(), capi.HAF_E_CAPACITY)
    big = np.ones((64, 65), np.uint16)                                       # 4160 > 4096 pixels in one frame; 2 x 2100 in two
    assert "max_points" in refused(1, (capi.Frame * 1)(capi.depth_frame(big, **K525)), gi, out, capi.HAF_E_CAPACITY)
    half = capi.depth_frame(np.ones((42, 50), np.uint16), **K525)
    assert "max_points" in refused(2, (capi.Frame * 2)(half, half), gi, out, capi.HAF_E_CAPACITY)
    for name, frame, code, _ in fc.refusal_frames():
        text = refused(1, (capi.Frame * 1)(frame), gi, out, code)
        assert "frame 0" in text, (name, text)
        refused(2, (capi.Frame * 2)(good, frame), gi, out, code)             # the second frame is checked before the first is touched
    eng.close()


def test_probability_mode_takes_frames(data_dir, golden_dir, tmp_path):
    """HAF_FLAG_PROBABILITY: only the source of the cloud differs, so the mode is served -- same outputs, fp32 vote grids, grasps grids
    and probabilities as the cloud path."""
    import json
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), os.path.join(golden_dir, "surrogate.model"), pj["probA"], pj["probB"])
    xyz = pcdio.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    s2b = pose(tilt(0.1, 0.05, -0.4), (0.02, 0.01, 0.8))
    frame = capi.depth_frame(render_depth(xyz, s2b), sensor_to_base=s2b, **K525)
    pts = capi.frame_points(frame)
    eng = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=1 << 19)
    inp = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=32)

    def snap(out):
        s = snapshot(eng, out)
        for r in range(eng.cfg.n_rolls):
            s["prob", r] = (eng.debug(capi.DBG_GRASPSGRID, 0, r).tobytes(), eng.debug(capi.DBG_PROBABILITY, 0, r).tobytes())
        return s
    a = snap(eng.score(pts, inp))
    assert a["out"]["n_evals"] >= 3000 and a["out"]["eval"] > -20
    b = snap(eng.score_frames([frame], [inp])[0])
    assert_same(b, a)
    eng.close()


def _write_binary_pcd(path, pts):
    head = "# .PCD v0.7\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (len(pts), len(pts))
    with open(path, "wb") as f:
        f.write(head.encode() + np.ascontiguousarray(pts, np.float32).tobytes())


def test_cli_depth_prints_what_the_cloud_of_the_same_frame_prints(data_dir, surrogate, tmp_path):
    """haf_grasp_cli --depth on a written PGM == the CLI on a binary PCD of haf_frame_points of the same frame: the per-roll hypotheses,
    the result line, and the ranked candidates of --top-k 5; also through the Python mirror of the action server."""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    xyz = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    s2b = pose(tilt(0.05, -0.1, 0.2), (0.13, 0.2, 0.9))
    depth = render_depth(xyz, s2b)
    pgm, pcd = str(tmp_path / "depth.pgm"), str(tmp_path / "points.pcd")
    fc.write_pgm16(pgm, depth)
    assert (capi.load_pgm16(pgm) == depth).all()
    frame = capi.depth_frame(depth, sensor_to_base=s2b, min_depth=0.2, max_depth=1.5, **K525)
    _write_binary_pcd(pcd, capi.frame_points(frame))
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42"]
    src = ["--depth", pgm, "--intrinsics", "525", "525", "319.5", "239.5", "--depth-range", "0.2", "1.5", "--sensor-pose"] + ["%.9g" % v for v in s2b]
    for extra in ([], ["--hypotheses"], ["--hypotheses", "--top-k", "5"], ["--show-only-best", "--hypotheses", "--top-k", "5", "--top-radius", "3"]):
        a = subprocess.run(common + extra + src, check=True, capture_output=True, text=True)
        b = subprocess.run(common + extra + [pcd], check=True, capture_output=True, text=True)
        la, lb = a.stdout.strip().splitlines(), b.stdout.strip().splitlines()
        assert la == lb, (extra, la, lb)
        final = [l for l in la if not l.startswith(("hypothesis ", "top "))]
        assert len(final) == 1 and int(final[0].split()[0]) > 50
        if not extra:
            plain_eval = int(final[0].split()[0])
        if extra == ["--hypotheses", "--top-k", "5"]:
            assert sum(l.startswith("hypothesis ") for l in la) >= 10 and sum(l.startswith("top ") for l in la) == 5
    bad = subprocess.run(common + ["--depth", str(tmp_path / "missing.pgm"), "--intrinsics", "525", "525", "319.5", "239.5"], capture_output=True, text=True)
    assert bad.returncode == 1 and "cannot open" in bad.stderr
    assert subprocess.run(common + ["--depth", pgm], capture_output=True, text=True).returncode == 2      # no intrinsics: usage
    # the Python mirror of the action interface
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 19, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    res = srv.execute_frame(goal, frame)
    top = srv.top_grasps(k=3)
    goal.input_pc = capi.frame_points(frame)
    assert srv.execute(goal) == res and srv.top_grasps(k=3) == top and res.eval == plain_eval
    srv.close()
