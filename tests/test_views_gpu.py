"""haf_score_views on the MI355X (include/hafgrasp.h): several sensor views fused into one cloud of their valid points, compacted on the
device by k_view_points (csrc/frames.hip).  The compacted points against haf_view_points as multisets, word for word; the views path
against the cloud path on the same engine and against the CPU oracle; batches, the bucket-sorted binning path, all-invalid requests,
one view against haf_score_frames, the engine-side refusals, probability mode and the CLI.  Every comparison is an equality.
Testing build throughout; the guard zones around every device buffer are checked after each test."""
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
from test_frames_gpu import (C3_CFG, C3_IN, DOWN, K525, TABLE1, _files, _write_binary_pcd, assert_same, device_copy, kernel_cases,
                             make_engine, pose, render_depth, snapshot, tilt)

pytestmark = pytest.mark.gpu

CAM_A = pose(tilt(0.21, -0.17, 0.6), (0.20, 0.13, 0.9))
CAM_B = pose(tilt(-0.25, 0.20, -0.8), (0.04, 0.34, 0.85))
CAM_C = pose(tilt(0.05, 0.30, 2.0), (0.30, 0.30, 0.95))


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


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


def sorted_rows(points):
    w = fc.words(points)
    return w[np.lexsort((w[:, 2], w[:, 1], w[:, 0]))]


def two_cameras(xyz, a=CAM_A, b=CAM_B):
    return [capi.depth_frame(render_depth(xyz, a), sensor_to_base=a, **K525), capi.depth_frame(render_depth(xyz, b), sensor_to_base=b, **K525)]


def view_sets():
    """-> list of (name, [host frame, ...], [the same frames, some device-resident]): every case of the frames kernel test -- all kinds on
    all shapes, padded rows, 640 x 480 one element off a 16-byte boundary, widths 1..17 -- three to a request, in three residences"""
    cases = kernel_cases()
    out = []
    for k in range(0, len(cases), 3):
        chunk = cases[k:k + 3]
        host = [c[1] for c in chunk]
        for where in ("host", "device", "mixed"):
            use = [f if where == "host" or (where == "mixed" and i % 2 == 0) else device_copy(f, img) for i, (_, f, img) in enumerate(chunk)]
            out.append(("%s..%s_%s" % (chunk[0][0], chunk[-1][0], where), host, use))
    return out


def test_kernel_compacts_exactly_the_valid_points(data_dir, surrogate):
    """haf_debug_fetch_points after haf_score_views, rows sorted == haf_view_points, rows sorted, every word; the counts agree; a second
    call gives the same multiset"""
    eng = make_engine(data_dir, surrogate, max_points=4 * 640 * 480)
    inp = capi.default_input()
    seen = kinds = 0
    for name, host, use in view_sets():
        want = sorted_rows(capi.view_points(host))
        for again in range(2):
            _, counts = eng.score_views([use], [inp])
            assert counts == [len(want)], (name, again, counts, len(want))
            got = sorted_rows(eng.fetch_points(0))
            bad = np.flatnonzero((got != want).any(axis=1)) if got.shape == want.shape else None
            assert got.shape == want.shape and bad.size == 0, (name, again, got.shape, want.shape, None if bad is None else (bad[:5], got[bad[:5]], want[bad[:5]]))
        seen += 1
        kinds |= sum(1 << f.kind for f in host)
    assert seen >= 3 * 27 and kinds & 7 == 7
    eng.close()


def test_views_path_equals_cloud_path_equals_oracle(data_dir, surrogate, orc, table1):
    """table1 rendered from two differently tilted cameras at C3 (56 x 56, 20 rolls): haf_score_views leaves exactly what haf_score leaves
    for haf_view_points of the two frames on the same engine, and that is what the CPU oracle computes from the fused cloud"""
    frames = two_cameras(table1)
    pts = capi.view_points(frames)
    per_view = [len(capi.view_points([f])) for f in frames]
    assert min(per_view) > 20000 and len(pts) == sum(per_view) < 2 * 640 * 480 // 2
    eng = make_engine(data_dir, surrogate, max_points=1 << 20, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    got, want = compare_full(eng, orc, pts, C3_CFG, C3_IN)
    print("two cameras: %d + %d valid points, n_evals %d eval %d best (%d, %d, %d)" % (per_view[0], per_view[1], got["n_evals"], got["eval"],
                                                                                     got["best_row"], got["best_col"], got["best_roll"]))
    assert got["n_evals"] >= 20000 and got["eval"] > 50                     # the comparison cannot pass on empty grids
    cloud = snapshot(eng, got)
    outs, counts = eng.score_views([frames], [inp])
    assert counts == [len(pts)]
    assert (sorted_rows(eng.fetch_points(0)) == sorted_rows(pts)).all()
    assert_same(snapshot(eng, outs[0]), cloud)
    for roll in range(want["rolls_done"]):
        assert (eng.debug(capi.DBG_HEIGHTS, 0, roll).view(np.uint32) == want["heights"][roll].view(np.uint32)).all()
        assert (eng.debug(capi.DBG_LABELS, 0, roll) == want["labels"][roll]).all()
        assert (eng.roll_grid(0, roll)[0] == want["graspseval"][roll]).all()
    out = outs[0]
    assert (out["eval"], out["best_row"], out["best_col"], out["best_roll"]) == (want["eval"], want["row"], want["col"], want["roll_idx"])
    # the fused scene is not either view's: scoring one camera alone gives other height grids
    single = snapshot(eng, eng.score_frames([frames[0]], [inp])[0])
    assert any(single["grid", 0, r] != cloud["grid", 0, r] for r in range(eng.cfg.n_rolls))
    # device-resident views, and the views in the other order: the same cloud as a set, so the same everything
    a, b = (render_depth(table1, CAM_A), render_depth(table1, CAM_B))
    dev = [device_copy(frames[0], a), device_copy(frames[1], b)]
    for use in (dev, [frames[1], dev[0]]):
        outs, counts = eng.score_views([use], [inp])
        assert counts == [len(pts)]
        assert_same(snapshot(eng, outs[0]), cloud)
    eng.close()


def test_views_on_the_bucket_sorted_binning_path(data_dir, tmp_path, table1):
    """The same two cameras on a 160 x 160 grid (beyond LDS size, more than 32768 points): binning sorts the cloud into spatial buckets,
    sized on the host by the upper bound and walked to the live count.  Same result as the cloud path."""
    model = models.write_random_model(str(tmp_path / "m64.model"), 64, seed=5)
    frames = two_cameras(table1)
    pts = capi.view_points(frames)
    assert len(pts) >= 32768
    eng = make_engine(data_dir, model, grid_h=160, grid_w=160, n_rolls=8, roll_step_deg=20, max_points=1 << 20)
    inp = capi.default_input(grasp_area_length_x=160, grasp_area_length_y=160, grasp_area_center=(0.13, 0.25, 0.0))
    a = eng.score(pts, inp)
    assert a["n_evals"] > 10000
    cloud = snapshot(eng, a)
    outs, counts = eng.score_views([frames], [inp])
    assert counts == [len(pts)] and (sorted_rows(eng.fetch_points(0)) == sorted_rows(pts)).all()
    assert_same(snapshot(eng, outs[0]), cloud)
    eng.close()


def test_batch_of_view_sets_equals_singles(data_dir, surrogate, table1):
    """Three requests with 1, 2 and 3 views of mixed kinds and residence in one call == the three requests one by one, and == the cloud
    path on each request's fused cloud (n_rechecked is counted per batch)"""
    da, db, dc = (render_depth(table1, c) for c in (CAM_A, CAM_B, CAM_C))
    fa, fb = capi.depth_frame(da, sensor_to_base=CAM_A, **K525), capi.depth_frame(db, sensor_to_base=CAM_B, **K525)
    metres = dc.astype(np.float32) * np.float32(0.001)
    fcm = capi.depth_frame(metres, sensor_to_base=CAM_C, depth_scale=1.0, **K525)
    cam_pts = np.zeros((480, 640, 4), np.float32)                            # pcl::PointXYZ: 16-byte points, sensor frame of camera B
    cam_pts[:, :, :3] = capi.frame_points(capi.depth_frame(db, **K525)).reshape(480, 640, 3)
    fx = capi.xyz_frame(cam_pts, sensor_to_base=CAM_B)
    host = [[fa], [fb, fcm], [fa, fx, fcm]]
    sets = [[fa], [device_copy(fb, db), fcm], [fa, fx, device_copy(fcm, metres)]]
    inputs = [capi.default_input(**C3_IN), capi.default_input(**dict(C3_IN, approach_vector=(0.1, -0.1, 1.0))),
              capi.default_input(**dict(C3_IN, show_only_best_grasp=1))]
    eng = make_engine(data_dir, surrogate, max_clouds=3, max_points=6 * 640 * 480, **C3_CFG)
    outs, counts = eng.score_views(sets, inputs)
    fused = [capi.view_points(h) for h in host]
    assert counts == [len(p) for p in fused]
    assert sum(o["n_evals"] >= 20000 and o["eval"] > 50 for o in outs) >= 2
    batch = snapshot(eng, None, 3)
    points = [sorted_rows(eng.fetch_points(b)) for b in range(3)]
    tops = eng.top_grasps(k=8)
    strip = lambda d: {k: v for k, v in d.items() if k != "n_rechecked"}
    for b in range(3):
        assert (points[b] == sorted_rows(fused[b])).all(), b
        for how in ("views", "cloud"):
            if how == "views":
                o1, c1 = eng.score_views([sets[b]], [inputs[b]])
                assert c1 == [counts[b]]
                o = o1[0]
            else:
                o = eng.score(fused[b], inputs[b])
            assert strip(o) == strip(outs[b]), (b, how)
            single = snapshot(eng, None)
            for r in range(eng.cfg.n_rolls):
                assert single["grid", 0, r] == batch["grid", b, r], (b, how, r)
            assert eng.top_grasps(k=8)[0] == tops[b], (b, how)
    eng.close()


def test_all_invalid_views_equal_the_empty_cloud(data_dir, surrogate):
    """A request whose every view is invalid: the counter stays 0 although the host sized the launches for all the pixels; what is left
    is what an empty cloud leaves.  Also next to a real request in one batch."""
    blank = [capi.depth_frame(np.zeros((48, 64), np.uint16), **K525), capi.depth_frame(np.full((5, 61), np.nan, np.float32), **K525),
             capi.xyz_frame(np.full((3, 7, 3), np.inf, np.float32))]
    assert len(capi.view_points(blank)) == 0
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=1 << 16)
    inp = capi.default_input()
    empty = snapshot(eng, eng.score(np.zeros((0, 3), np.float32), inp))
    outs, counts = eng.score_views([blank], [inp])
    assert counts == [0] and eng.fetch_points(0).shape == (0, 3)
    assert_same(snapshot(eng, outs[0]), empty)
    rng = np.random.default_rng(12)
    real = [capi.depth_frame(fc.u16_image(rng, 61, 5), sensor_to_base=pose(DOWN, (0.0, 0.0, 0.9)), **fc._intrinsics(rng, 61, 5))]
    one = snapshot(eng, eng.score(capi.view_points(real), inp))
    outs, counts = eng.score_views([blank, real], [inp, inp])
    assert counts == [0, len(capi.view_points(real))]
    both = snapshot(eng, None, 2)
    for r in range(eng.cfg.n_rolls):
        assert both["grid", 0, r] == empty["grid", 0, r] and both["grid", 1, r] == one["grid", 0, r]
    eng.close()


def test_one_view_equals_score_frames(data_dir, surrogate, table1):
    """haf_score_views with a single view leaves what haf_score_frames leaves for that frame (which bins the invalid pixels too)"""
    frame = two_cameras(table1)[0]
    eng = make_engine(data_dir, surrogate, max_points=1 << 19, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    out = eng.score_frames([frame], [inp])[0]
    assert out["n_evals"] >= 20000 and out["eval"] > 50
    frames = snapshot(eng, out)
    outs, counts = eng.score_views([[frame]], [inp])
    assert counts == [len(capi.view_points([frame]))] and counts[0] < 640 * 480
    assert_same(snapshot(eng, outs[0]), frames)
    eng.close()


def test_engine_side_refusals_leave_the_engine_usable(data_dir, surrogate):
    """Every refusal of haf_score_views returns its code and a text that names the request and the view, before any device work: the
    last-batch state is still the previous call's, and the next valid call is served as if nothing had happened.  A device-resident XYZ
    view next to a host XYZ view is NOT a refusal: the host one is staged in its own raw area, never where the points are written."""
    import torch
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=4096)
    L, h = eng._L, eng._h
    inp = capi.default_input()
    rng = np.random.default_rng(4)
    good = capi.depth_frame(fc.u16_image(rng, 61, 5), sensor_to_base=pose(DOWN, (0.0, 0.0, 0.9)), **fc._intrinsics(rng, 61, 5))
    xyz_img = fc.xyz_image(rng, 17, 9, 4)
    xyz_host = capi.xyz_frame(xyz_img, sensor_to_base=fc.tilted_pose(rng))
    xyz_dev = device_copy(xyz_host, xyz_img)
    ref_sets = [[good, xyz_host, xyz_dev]]
    ref, ref_counts = eng.score_views(ref_sets, [inp])
    assert ref_counts == [len(capi.view_points([good, xyz_host, xyz_host]))]
    assert (sorted_rows(eng.fetch_points(0)) == sorted_rows(capi.view_points([good, xyz_host, xyz_host]))).all()
    ref_snap, ref_pts = snapshot(eng, ref[0]), sorted_rows(eng.fetch_points(0)).tobytes()
    # ... in the other order too, and twice the host one
    for use in ([xyz_dev, xyz_host], [xyz_host, xyz_host, good]):
        _, c = eng.score_views([use], [inp])
        want = capi.view_points([xyz_host if f is xyz_dev else f for f in use])
        assert c == [len(want)] and (sorted_rows(eng.fetch_points(0)) == sorted_rows(want)).all()
    eng.score_views(ref_sets, [inp])

    def refused(n, per, frames, inputs, out, code):
        cnt = (C.c_int64 * 4)(*([-7] * 4))
        rc = L.haf_score_views(h, n, per, frames, inputs, out, cnt)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text, (rc, code, text)
        assert list(cnt) == [-7] * 4
        # the last-batch state is the previous call's ...
        assert snapshot(eng, ref[0]) == ref_snap and sorted_rows(eng.fetch_points(0)).tobytes() == ref_pts
        # ... and the next call is served
        o, c = eng.score_views(ref_sets, [inp])
        assert o == ref and c == ref_counts and sorted_rows(eng.fetch_points(0)).tobytes() == ref_pts
        return text

    two, gi, out = (capi.Frame * 2)(good, good), (capi.GraspInput * 2)(inp, inp), (capi.GraspOutput * 2)()
    per = lambda *v: (C.c_int32 * len(v))(*v)
    for args in ((1, None, two, gi, out), (1, per(1), None, gi, out), (1, per(1), two, None, out), (1, per(1), two, gi, None),
                 (0, per(1), two, gi, out), (-3, per(1), two, gi, out)):
        refused(*args, capi.HAF_E_ARG)
    assert L.haf_score_views(None, 1, per(1), two, gi, out, None) == capi.HAF_E_ARG
    many = (capi.Frame * 17)(*([good] * 17))
    for v in (0, -1, 17):
        assert "request 0" in refused(1, per(v), many, gi, out, capi.HAF_E_ARG)
    assert "request 1" in refused(2, per(1, 0), many, gi, out, capi.HAF_E_ARG)
    assert "max_clouds" in refused(3, per(1, 1, 1), many, (capi.GraspInput * 3)(inp, inp, inp), (capi.GraspOutput * 3)(), capi.HAF_E_CAPACITY)
    half = capi.depth_frame(np.ones((42, 50), np.uint16), **K525)              # 2 x 2100 pixels > 4096, in one request or in two
    halves = (capi.Frame * 2)(half, half)
    assert "max_points" in refused(1, per(2), halves, gi, out, capi.HAF_E_CAPACITY)
    assert "max_points" in refused(2, per(1, 1), halves, gi, out, capi.HAF_E_CAPACITY)
    for name, frame, code, _ in fc.refusal_frames():
        text = refused(1, per(2), (capi.Frame * 2)(good, frame), gi, out, code)
        assert "request 0 view 1" in text, (name, text)
    text = refused(2, per(1, 2), (capi.Frame * 3)(good, good, fc.refusal_frames()[0][1]), gi, out, capi.HAF_E_ARG)
    assert "request 1 view 1" in text, text
    torch.cuda.synchronize()
    eng.close()


def test_probability_mode_takes_views(data_dir, golden_dir, tmp_path):
    """HAF_FLAG_PROBABILITY: only the source of the cloud differs -- same outputs, fp32 vote grids, grasps grids and probabilities as the
    cloud path on the fused cloud"""
    import json
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), os.path.join(golden_dir, "surrogate.model"), pj["probA"], pj["probB"])
    xyz = pcdio.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    a, b = pose(tilt(0.1, 0.05, -0.4), (0.02, 0.01, 0.8)), pose(tilt(-0.2, 0.1, 0.9), (-0.03, 0.05, 0.75))
    frames = two_cameras(xyz, a, b)
    pts = capi.view_points(frames)
    eng = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=1 << 20)
    inp = capi.default_input(grasp_area_length_x=32, grasp_area_length_y=32)

    def snap(out):
        s = snapshot(eng, out)
        for r in range(eng.cfg.n_rolls):
            s["prob", r] = (eng.debug(capi.DBG_GRASPSGRID, 0, r).tobytes(), eng.debug(capi.DBG_PROBABILITY, 0, r).tobytes())
        return s
    want = snap(eng.score(pts, inp))
    assert want["out"]["n_evals"] >= 3000 and want["out"]["eval"] > -20
    outs, counts = eng.score_views([frames], [inp])
    assert counts == [len(pts)]
    assert_same(snap(outs[0]), want)
    eng.close()


def test_cli_two_depth_views_print_what_the_fused_cloud_prints(data_dir, surrogate, tmp_path, table1):
    """haf_grasp_cli with two --depth files, each with its own pose and range (the second inherits the first one's intrinsics) == the CLI
    on a binary PCD of haf_view_points of the two frames; also through the Python mirror of the action server"""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    da, db = render_depth(table1, CAM_A), render_depth(table1, CAM_B)
    pa, pb, pcd = str(tmp_path / "a.pgm"), str(tmp_path / "b.pgm"), str(tmp_path / "fused.pcd")
    fc.write_pgm16(pa, da)
    fc.write_pgm16(pb, db)
    frames = [capi.depth_frame(da, sensor_to_base=CAM_A, min_depth=0.2, max_depth=1.5, **K525),
              capi.depth_frame(db, sensor_to_base=CAM_B, min_depth=0.2, max_depth=0.85, **K525)]
    fused = capi.view_points(frames)
    assert len(fused) < len(capi.view_points(two_cameras(table1)))          # the second view's own range cuts points
    _write_binary_pcd(pcd, fused)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42"]
    src = ["--intrinsics", "525", "525", "319.5", "239.5", "--depth-range", "0.2", "1.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % v for v in CAM_A] + \
          ["--depth", pb, "--depth-range", "0.2", "0.85", "--sensor-pose"] + ["%.9g" % v for v in CAM_B]
    for extra in ([], ["--hypotheses", "--top-k", "5"]):
        a = subprocess.run(common + extra + src, check=True, capture_output=True, text=True)
        b = subprocess.run(common + extra + [pcd], check=True, capture_output=True, text=True)
        la, lb = a.stdout.strip().splitlines(), b.stdout.strip().splitlines()
        assert la == lb, (extra, la, lb)
        final = [l for l in la if not l.startswith(("hypothesis ", "top "))]
        assert len(final) == 1 and int(final[0].split()[0]) > 50
        assert "2 views fused: %d valid points" % len(fused) in a.stderr
        if extra:
            assert sum(l.startswith("hypothesis ") for l in la) >= 10 and sum(l.startswith("top ") for l in la) == 5
        else:
            plain_eval = int(final[0].split()[0])
    seventeen = sum((["--depth", pa] for _ in range(17)), [])
    assert subprocess.run(common + ["--intrinsics", "525", "525", "319.5", "239.5"] + seventeen, capture_output=True, text=True).returncode == 2
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    res = srv.execute_views(goal, frames)
    top = srv.top_grasps(k=3)
    goal.input_pc = fused
    assert srv.execute(goal) == res and srv.top_grasps(k=3) == top and res.eval == plain_eval
    srv.close()
