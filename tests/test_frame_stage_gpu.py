"""The wiring of the sensor-frame staging code (csrc/frame_stage.h, StageBuf in csrc/engine_state.h) into the engine on the MI355X: host
frames large enough to go to the device in several pieces, through every entry point that takes a haf_frame, against the same call on the
same pixels handed over device-resident -- the route that stages nothing.  Every comparison is an equality.  The staging arithmetic itself
is tested without a device (tests/test_frame_stage_cpu.py).  And the way out of a label image: every call that writes one, into every
residence of its output, against its host definition, with the descriptor handed back.  Testing build; the guard zones around every device buffer are checked after
every request and after each test."""
import os

import numpy as np
import pytest

import frame_cases as fc
import pcdio
import segment_cases as sc
import transfer_cases as tc
from haf_grasping_amd import capi
from test_depth_filter_gpu import SENTINEL, device_image, fetch
from test_frames_gpu import C3_IN, K525, TABLE1, assert_same, device_copy, make_engine, render_depth, snapshot
from test_labels_gpu import device_labels
from test_roi_gpu import device_mask, strip
from test_segment_gpu import TABLE1_PARAMS, image_of
from test_views_gpu import CAM_A, sorted_rows

pytestmark = pytest.mark.gpu

CFG = dict(n_rolls=6, roll_step_deg=30, max_points=700000)      # 56 x 56 grids
K200 = dict(fx=164.0, fy=164.0, cx=99.5, cy=59.5)                # the 640 x 480 camera at 200 x 120


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def scenes(data_dir):
    """-> {name: (host frame, its array, device-resident copy, host mask with padded rows, (device mask, its keep-alive))}:
    u16: 640 x 480 depth, rows padded by 3 elements: 614 400 packed bytes, three pieces;
    xyz: 200 x 120 organised cloud, 20-byte points, rows padded by 2 points: 288 000 packed bytes, two pieces"""
    table1 = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    depth = fc.padded(render_depth(table1, CAM_A), 3)
    u16 = capi.depth_frame(depth, sensor_to_base=CAM_A, **K525)
    small = render_depth(table1, CAM_A, width=200, height=120, **K200)
    wide = np.full((120, 202, 5), 7.0, np.float32)
    wide[:, :200, :3] = capi.frame_points(capi.depth_frame(small, **K200)).reshape(120, 200, 3)      # identity pose: sensor-frame points
    cloud = wide[:, :200]
    xyz = capi.xyz_frame(cloud, sensor_to_base=CAM_A)
    assert (u16.row_stride_bytes, xyz.row_stride_bytes, xyz.point_stride_bytes) == (643 * 2, 202 * 20, 20)
    out = {}
    for name, frame, image in (("u16", u16, depth), ("xyz", xyz, cloud)):
        h, w = frame.height, frame.width
        mask = np.full((h, w + 5), 9, np.uint8)
        mask[:, :w] = 0
        mask[h // 4:3 * h // 4, w // 4:3 * w // 4] = 1
        mask = mask[:, :w]
        assert np.isfinite(capi.frame_points(frame)).all(axis=1).mean() > 0.05      # (table1 fills an eighth of the image)
        out[name] = (frame, image, device_copy(frame, image), mask, device_mask(mask))
    return out


@pytest.fixture(scope="module")
def engine(data_dir, golden_dir):
    eng = make_engine(data_dir, os.path.join(golden_dir, "surrogate.model"), **CFG)
    yield eng
    eng.close()


def roi_state(eng, out):
    """what an ROI request leaves, without the tier counts (a host mask is counted, a device-resident one is not: the same labels may
    come from different tiers)"""
    s = snapshot(eng, out)
    del s["tiers"], s["exact"]
    s["out"] = strip(out)
    s["labels"] = [eng.debug(capi.DBG_LABELS, 0, r).tobytes() for r in range(eng.cfg.n_rolls)]
    return s


@pytest.mark.parametrize("name", ["u16", "xyz"])
def test_staged_host_frame_equals_device_resident_frame_on_every_route(engine, scenes, name):
    """haf_score_frames, haf_score_views (as the only view and as the second of two), haf_score_frames_roi with a host mask of padded rows
    and haf_grasp_map: outputs, the points the kernels read (as a sorted multiset for views), the batch's grids, tier counts and ranked
    candidates, and the three map images are those of the same call on the device-resident copy.  So are the stages around a request,
    each with its host side image in padded rows against the device-resident one: haf_segment_frame into a padded host canvas and into
    the engine's image, haf_fit_plane under the mask, haf_measure_labels, haf_filter_depth of the frame twice (depth only),
    haf_grasp_map_best under the mask and haf_grasp_map_labels"""
    eng, inp = engine, capi.default_input(**C3_IN)
    host, _, dev, mask, (dmask, _) = scenes[name]
    other = scenes["xyz" if name == "u16" else "u16"][2]          # device-resident in both calls
    want_points = fc.words(capi.frame_points(host))

    def frames_route(f):
        out = eng.score_frames([f], [inp])[0]
        return snapshot(eng, out), fc.words(eng.debug_points(0)), eng.grasp_map(0, f)

    got, ref = frames_route(host), frames_route(dev)
    assert_same(got[0], ref[0])
    assert (got[1] == ref[1]).all() and (got[1] == want_points).all()
    assert got[0]["out"]["n_evals"] > 1000 and got[0]["out"]["eval"] > 0          # (not a comparison of empty grids)
    for k in ("vote", "roll", "cell"):
        assert (got[2][k] == ref[2][k]).all(), k
    assert (got[2]["cell"] >= 0).any()

    def views_route(views):
        outs, counts = eng.score_views([views], [inp])
        return snapshot(eng, outs[0]), sorted_rows(eng.fetch_points(0)), counts

    for views_host, views_dev in (([host], [dev]), ([other, host], [other, dev])):
        got, ref = views_route(views_host), views_route(views_dev)
        assert got[2] == ref[2] and got[2][0] > 1000
        assert_same(got[0], ref[0])
        assert got[1].shape == ref[1].shape and (got[1] == ref[1]).all()

    def roi_route(f, m):
        out = eng.score_frames_roi([f], [m], [inp])[0]
        return roi_state(eng, out), fc.words(eng.debug_points(0))

    got, ref = roi_route(host, mask), roi_route(dev, dmask)
    assert_same(got[0], ref[0])
    assert (got[1] == ref[1]).all() and (got[1] == want_points).all()
    assert 0 < got[0]["out"]["n_evals"]

    h, w = host.height, host.width
    sp = capi.segment_params(**TABLE1_PARAMS)

    def segment_route(f):
        canvas = np.full((h, w + 2), 0x5A, np.uint8)
        labels, infos, stats = eng.segment(f, sp, host_out=canvas[:, :w])
        assert labels.ctypes.data == canvas.ctypes.data and (canvas[:, w:] == 0x5A).all()
        img, infos_own, stats_own = eng.segment(f, sp, device_out=True)
        return labels.tobytes(), infos.tobytes(), stats, image_of(img, f, np.uint8)[0].tobytes(), infos_own.tobytes(), stats_own

    got, ref = segment_route(host), segment_route(dev)
    assert got == ref and got[0] == got[3] and got[2][3] >= 1                     # (objects were found: not a comparison of empty images)
    n_labels = min(got[2][3], sp.max_labels)
    labels = np.full((h, w + 3), 200, np.uint8)                                   # padded rows, the padding a label that must never be read
    labels[:, :w] = np.frombuffer(got[0], np.uint8).reshape(h, w)
    labels = labels[:, :w]
    dlabels, _keep = device_labels(labels, stride_bytes=w + 5)

    def plane_route(f, m):
        fit = eng.fit_plane(f, mask=m, debug=True)
        return {k: v.tobytes() if isinstance(v, np.ndarray) else v for k, v in fit.items()}

    got, ref = plane_route(host, mask), plane_route(dev, dmask)
    assert_same(got, ref)
    assert got["stats"][1] > 100                                                  # (usable pixels under the mask)
    got, ref = eng.measure_labels(host, labels, n_labels, plane=[0, 0, 1, 0]), eng.measure_labels(dev, dlabels, n_labels, plane=[0, 0, 1, 0])
    assert got.tobytes() == ref.tobytes() and len(got) == n_labels

    if name == "u16":
        def filter_route(frames):
            f, stats = eng.filter_depth(frames)                                   # (into the engine's image: max_points holds two host frames, not a third image)
            assert f.on_device == 1 and f.row_stride_bytes == w * 2
            return fetch(f.data, h * w * 2).tobytes(), stats

        got, ref = filter_route([host, host]), filter_route([dev, dev])
        assert got == ref and got[1][2] > 1000

    eng.score_frames([dev], [inp])
    got, ref = eng.best_in_mask(0, host, mask), eng.best_in_mask(0, dev, mask)
    assert got is not None and got == ref

    def labels_route(f, l):
        res = eng.best_per_label(0, f, l, n_labels)
        return dict(res, picks=res["picks"].tobytes())

    got, ref = labels_route(host, labels), labels_route(dev, dlabels)
    assert_same(got, ref)
    assert len(got["order"]) >= 1


def label_writers():
    """-> [(name, frame, image, call(eng, frame, dtype, **output) -> labels, ref(frame, dtype) -> labels)] for haf_segment_frame,
    haf_segment_cells and haf_transfer_labels, each on a 61 x 5 frame (no multiple of the kernels' 4 or 8 pixel groups: head and tail
    stores run) and on a 1 x 1 frame ((h - 1) * stride vanishes), from the small synthetic scenes of segment_cases, cell_segment_cases
    and transfer_cases"""
    out = []
    n_of = lambda dt: 255 if dt == np.uint8 else 300                               # (a uint8 output holds 255 labels)
    for w, h in ((61, 5), (1, 1)):
        size = "_%dx%d" % (w, h)
        frame, image, kw = sc.make_case("random", "u16", (w, h), False)
        p = capi.segment_params(**kw)
        out.append(("segment" + size, frame, image, lambda eng, f, dt, p=p, **o: eng.segment(f, p, dt, **o)[0],
                    lambda f, dt, p=p: capi.segment_ref(f, p, dt)[0]))
        frame, image, kw = sc.make_case("random", "xyz", (w, h), True)
        p = capi.cell_segment_params(plane=kw["plane"], min_height=0.01, max_height=0.2, min_points=2, max_step=0.03)
        out.append(("cells" + size, frame, image, lambda eng, f, dt, p=p, **o: eng.segment_cells(f, p, dt, **o)[0],
                    lambda f, dt, p=p: capi.segment_cells_ref(f, p, dt)[0]))
        rng = np.random.default_rng([61, w, h])
        frame, image = tc.depth_case_frame(capi.FRAME_DEPTH_F32, w, h, rng, pad=3 if h > 1 else 0, holes=h > 1)
        cam, labels = tc.label_camera(17, 9), tc.label_image(17, 9, np.uint16, rng, 300, pad=5)
        out.append(("transfer" + size, frame, image, lambda eng, f, dt, c=cam, l=labels, **o: eng.transfer_labels(f, c, l, n_of(dt), None, dt, **o)[0],
                    lambda f, dt, c=cam, l=labels: capi.transfer_labels_ref(f, c, l, n_of(dt), None, dt)[0]))
    return out


def test_label_outputs_of_every_residence_and_what_is_handed_back(data_dir, golden_dir):
    """Engine.segment, Engine.segment_cells and Engine.transfer_labels on one small engine (max_points just above 61 x 5), uint8 and
    uint16, into a host canvas whose rows are 80 elements apart, into the caller's device image of the same stride and into the engine's
    own image: the image is the *_ref image, every canvas byte outside it is untouched, and the LabelImage handed back has exactly the
    data, on_device, row_stride_bytes and elem_bytes of where the image lies.  For the 1 x 1 frame the caller's device image is a bare
    pointer, whose stride capi substitutes.  The guard zones are checked inside every call and after the test."""
    eng = make_engine(data_dir, os.path.join(golden_dir, "surrogate.model"), n_rolls=1, max_points=320)
    own, nonzero = set(), 0
    for name, frame, image, call, ref in label_writers():
        h, w = frame.height, frame.width
        dev = device_copy(frame, image)
        for dtype in (np.uint8, np.uint16):
            e, at = np.dtype(dtype).itemsize, (name, dtype.__name__)
            want = ref(frame, dtype)
            assert want.shape == (h, w) and want.dtype == dtype, at
            nonzero += int((want != 0).sum())
            # a host canvas, rows 80 elements apart; a host and a device-resident frame
            for f in (frame, dev):
                canvas = np.full((h, 80), 0x5A, dtype)
                got = call(eng, f, dtype, host_out=canvas[:, :w])
                assert got.ctypes.data == canvas.ctypes.data and (got == want).all() and (canvas[:, w:] == 0x5A).all(), at
            # the caller's device image of the same stride
            keep, ptr, stride, nbytes = device_image(frame, dtype, pad_elems=80 - w)
            img = call(eng, frame, dtype, device_out=(ptr, stride) if h > 1 else ptr)
            assert (img.data, img.on_device, img.row_stride_bytes, img.elem_bytes) == (ptr, 1, 80 * e if h > 1 else w * e, e), at
            labels, pad = image_of(img, frame, dtype)
            whole, off = keep.cpu().numpy(), ptr - keep.data_ptr()
            assert (labels == want).all() and (pad == SENTINEL).all() and (whole[:off] == SENTINEL).all() and (whole[off + nbytes:] == SENTINEL).all(), at
            # the engine's own image, packed
            img = call(eng, dev, dtype, device_out=True)
            assert img.data and (img.on_device, img.row_stride_bytes, img.elem_bytes) == (1, w * e, e), at
            assert (image_of(img, frame, dtype)[0] == want).all(), at
            own.add(img.data)
    assert len(own) == 1                                                           # one image: the three calls share it
    assert nonzero > 100                                                           # (not a comparison of empty images)
    eng.close()


def test_staging_blocks_grow_and_leave_results_as_they_were(data_dir, golden_dir, scenes):
    """a fresh engine: a host XYZ view (the raw area of XYZ views is allocated), an ROI request (the mask area is) and a grasp map of the
    200 x 120 frame (the map block is); then a grasp map of the 640 x 480 frame, for which the map block grows; then the first three
    calls again: the same results"""
    eng, inp = make_engine(data_dir, os.path.join(golden_dir, "surrogate.model"), **CFG), capi.default_input(**C3_IN)
    xyz, _, _, mask, _ = scenes["xyz"]
    u16 = scenes["u16"][0]

    def three_calls():
        outs, counts = eng.score_views([[xyz]], [inp])
        views = (snapshot(eng, outs[0]), sorted_rows(eng.fetch_points(0)).tobytes(), counts)
        roi = roi_state(eng, eng.score_frames_roi([xyz], [mask], [inp])[0])
        return views, roi, {k: v.tobytes() for k, v in eng.grasp_map(0, xyz).items()}

    before = three_calls()
    large = eng.grasp_map(0, u16)
    assert large["vote"].shape == (480, 640) and (large["cell"] >= 0).any()
    after = three_calls()
    assert before[0][1:] == after[0][1:] and before[2] == after[2]
    assert_same(before[0][0], after[0][0])
    assert_same(before[1], after[1])
    assert (eng.grasp_map(0, u16)["vote"] == large["vote"]).all()
    eng.close()
