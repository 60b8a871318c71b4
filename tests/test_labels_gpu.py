"""The best grasp per instance label on the MI355X (include/hafgrasp.h: haf_grasp_map_labels; csrc/graspmap.hip: k_map_labels,
k_label_records).  The engine call against haf_label_best_ref on the engine's own roll grids and against the numpy expectation of
label_cases.py on the map haf_grasp_map returns; its poses against haf_cell_pose and its picks against haf_grasp_map_best; synthetic
grids through the re-vote hook; a batch on a roll sub-range; the composition with haf_score_frames_roi; state preservation; the
engine-side refusals; the CLI.  Every comparison is an equality.  Testing build throughout; the guard zones around every device buffer
are checked after each test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import label_cases as lc
import pcdio
import vote_cases as vc
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, _files, device_copy, make_engine, render_depth
from test_grasp_map_cpu import scene_frames
from test_grasp_map_gpu import engine_grids, full_state
from test_views_gpu import CAM_A

pytestmark = pytest.mark.gpu

H = W = 56
TINY = np.array([[0.0, 0.0, 0.05], [0.01, 0.0, 0.05], [0.0, 0.01, 0.06]], np.float32)


def cell_centre_frame(N):
    """an XYZ frame with one point in the middle of every 1 cm cell of the N x N area around the origin, and its image"""
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    img = np.stack([(ii + 0.5) * 0.01 - N * 0.005, (jj + 0.5) * 0.01 - N * 0.005, np.full((N, N), 0.05)], -1).astype(np.float32)
    return capi.xyz_frame(img), img


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")          # every label call checks the guard zones itself, too
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


@pytest.fixture(scope="module")
def c3(data_dir, surrogate, table1):
    """one C3 engine for the module (56 x 56, 20 rolls of 9 degrees, two requests); score() puts the CAM_A frame of table1 into it as
    the last batch -> dict(eng, inp, fa, da, score)"""
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=2 * 640 * 480, **C3_CFG)
    da = render_depth(table1, CAM_A)
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    inp = capi.default_input(**C3_IN)
    yield dict(eng=eng, inp=inp, fa=fa, da=da, score=lambda: eng.score_frames([fa], [inp])[0])
    eng.close()


def device_labels(labels, stride_bytes=None, offset=0):
    """the label image in device memory, rows stride_bytes apart, its first byte `offset` bytes past a 256-byte boundary, the padding
    full of a label that must never be read -> the (pointer, elem_bytes, stride) tuple capi.label_image takes, and the tensor to keep"""
    import torch
    h, w = labels.shape
    eb = labels.itemsize
    stride_bytes = stride_bytes or w * eb
    host = np.full(offset + h * stride_bytes + 16, 1, np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[offset:], (h, w * eb), (stride_bytes, 1))
    rows[:] = np.ascontiguousarray(labels).view(np.uint8).reshape(h, w * eb)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 256 == 0
    return (dev.data_ptr() + offset, eb, stride_bytes), dev


def device_label_tensor(labels, pad=0):
    """the label image as a device tensor handed over as it is: with pad > 0 a view into a tensor whose rows are `pad` elements longer,
    the padding full of a label that must never be read (torch has no uint16: the 16-bit labels travel as int16, the same bytes)"""
    import torch
    h, w = labels.shape
    wide = np.full((h, w + pad), 1, labels.dtype)
    wide[:, :w] = labels
    dev = torch.from_numpy(wide.view(np.int16) if labels.dtype == np.uint16 else wide).cuda()
    torch.cuda.synchronize()
    return dev[:, :w]


def check_labels(eng, request, inp, roll_first, count, frame, img, labels, n_labels, min_vote, name, grids=None, maps=None, variants=True):
    """best_per_label == label_best_ref on the engine's roll grids == the numpy expectation on the engine's grasp map, for a host frame
    with host labels and (variants) for a device frame with device labels; the poses are cell_pose of the picks -> the result"""
    grids = engine_grids(eng, request, roll_first, count) if grids is None else grids
    maps = eng.grasp_map(request, frame) if maps is None else maps
    want = lc.expect(maps["vote"], maps["roll"], maps["cell"], labels, n_labels, min_vote)
    ref = capi.label_best_ref(eng.cfg, inp, roll_first, grids, frame, labels, n_labels=n_labels, min_vote=min_vote)
    lc.assert_picks_equal(ref, want, name + "/ref")
    got = eng.best_per_label(request, frame, labels, n_labels=n_labels, min_vote=min_vote)
    lc.assert_picks_equal(got, want, name + "/host")
    assert [p is not None for p in got["poses"]] == [bool(f) for f in want[0]["found"]]
    if variants:
        dl, keep = device_labels(labels)
        dev = eng.best_per_label(request, device_copy(frame, img), dl, n_labels=n_labels, min_vote=min_vote)
        lc.assert_picks_equal(dev, want, name + "/device")
        assert dev["poses"] == got["poses"], name
    return got


def check_poses(eng, request, res):
    """poses[l - 1] == haf_cell_pose at the pick's (roll, cell) for EVERY found label, the low-ranked ones at the border of the search
    area included, where the 9 x 8 z window clips"""
    Wg = eng.cfg.grid_w
    assert sorted(res["order"]) == [int(l) + 1 for l in np.flatnonzero(res["picks"]["found"])]
    for l in res["order"]:
        p = res["picks"][l - 1]
        assert res["poses"][l - 1] == eng.cell_pose(request, int(p["roll"]), int(p["cell"]) // Wg, int(p["cell"]) % Wg), l


def test_labels_equal_the_host_definition_and_the_map(c3, table1):
    """The CAM_A frame of table1 scored at C3.  blocks80 as uint8 and interleave(4096) as uint16, host frame with host labels and device
    frame with device labels; device labels 2 bytes past a 16-byte boundary with rows 700 (uint8) and 1400 (uint16) bytes apart; an
    F32 and an XYZ frame (G = 4) that were never scored; labels above n_labels; min_vote 71; poses == haf_cell_pose; three labels of
    blocks80 -- the best, one that shares its top vote with another, one that is not found -- against haf_grasp_map_best."""
    eng, inp, fa, da = c3["eng"], c3["inp"], c3["fa"], c3["da"]
    out = c3["score"]()
    assert out["n_evals"] >= 20000 and out["eval"] > 50
    grids, maps = engine_grids(eng, 0, 0, 20), eng.grasp_map(0, fa)
    b80, i4096 = lc.blocks80(), lc.interleave(4096)
    res = check_labels(eng, 0, inp, 0, 20, fa, da, b80, 48, 1, "blocks80", grids, maps)
    check_poses(eng, 0, res)
    found = len(res["order"])
    tops = [int(res["picks"]["vote"][l - 1]) for l in res["order"]]
    print("blocks80: found %d, top votes %r" % (found, tops))
    assert found >= 15 and 48 - found >= 20 and tops == sorted(tops, reverse=True) and len(set(tops)) < len(tops)
    big = check_labels(eng, 0, inp, 0, 20, fa, da, i4096, 4096, 1, "interleave(4096)", grids, maps)
    check_poses(eng, 0, big)
    assert len(big["order"]) >= 3500
    check_labels(eng, 0, inp, 0, 20, fa, da, b80, 48, 71, "blocks80 min_vote 71", grids, maps, variants=False)
    check_labels(eng, 0, inp, 0, 20, fa, da, b80, 20, 1, "labels above n_labels", grids, maps, variants=False)
    # misaligned device labels with padded rows, against the host result; a padded host view
    for labels, stride, want in ((b80, 700, res), (i4096, 1400, big)):
        dl, keep = device_labels(labels, stride, offset=2)
        assert dl[0] % 16 == 2
        for frame in (fa, device_copy(fa, da)):
            got = eng.best_per_label(0, frame, dl, n_labels=len(want["picks"]))
            assert (got["picks"] == want["picks"]).all() and got["order"] == want["order"] and got["poses"] == want["poses"], stride
    got = eng.best_per_label(0, fa, lc.padded_view(b80.astype(np.uint16), 5))
    assert (got["picks"] == res["picks"]).all() and got["order"] == res["order"]
    # device tensors handed over as they are: a contiguous one and a view with padded rows, 8- and 16-bit
    for labels, pad, want in ((b80, 0, res), (b80, 60, res), (i4096, 0, big), (i4096, 30, big)):
        t = device_label_tensor(labels, pad)
        assert t.is_contiguous() == (pad == 0)
        got = eng.best_per_label(0, device_copy(fa, da), t, n_labels=len(want["picks"]))
        assert (got["picks"] == want["picks"]).all() and got["order"] == want["order"] and got["poses"] == want["poses"], (labels.dtype, pad)
    # the three labels against the masked best
    tied = next(l for k, l in enumerate(res["order"]) if k and tops[k] == tops[k - 1])
    missing = next(l for l in range(1, 49) if not res["picks"]["found"][l - 1])
    for l in (res["order"][0], tied, missing):
        hit = eng.best_in_mask(0, fa, (b80 == l).astype(np.uint8), 1)
        p = res["picks"][l - 1]
        if l == missing:
            assert hit is None and res["poses"][l - 1] is None
        else:
            assert hit == (res["poses"][l - 1], int(p["u"]), int(p["v"])), l
    # frames of the other kinds, four pixels to a lane, never scored
    frames = {name: (frame, img) for name, frame, img in scene_frames(table1)}
    for name in ("f32_cam_b_padded", "xyz16_cam_b"):
        frame, img = frames[name]
        r = check_labels(eng, 0, inp, 0, 20, frame, img, b80, 48, 1, name, grids)
        check_poses(eng, 0, r)
        assert len(r["order"]) >= 5, name


def test_small_frames_partial_groups_and_one_pixel(c3, table1):
    """13 x 7 frames of every kind around the map's best pixel (91 pixels: a partial last group for G = 8 and G = 4, rows that are no
    multiple of a group) and a 1 x 1 frame, labels that change from pixel to pixel, uint8 and uint16, host and device"""
    eng, inp, fa, da = c3["eng"], c3["inp"], c3["fa"], c3["da"]
    c3["score"]()
    grids, maps = engine_grids(eng, 0, 0, 20), eng.grasp_map(0, fa)
    bu, bv = gm.key_argmax(maps["vote"], maps["roll"], None, 1)
    small = lc.small_frames(da, CAM_A, min(max(bu - 6, 0), 640 - 13), min(max(bv - 3, 0), 480 - 7))
    one = [(n, f, i) for n, f, i in scene_frames(table1) if n == "u16_single_pixel"]
    hits = {}
    for name, frame, img in small + one:
        for dtype in (np.uint8, np.uint16):
            labels = lc.interleave(5, frame.width, frame.height).astype(dtype)
            for mv in (1, -100):
                r = check_labels(eng, 0, inp, 0, 20, frame, img, labels, 5, mv, "%s/%s/%d" % (name, dtype.__name__, mv), grids)
                check_poses(eng, 0, r)
                hits[name] = hits.get(name, 0) + len(r["order"])
    print(hits)
    assert all(hits[n] >= 10 for n, _, _ in small) and hits["u16_single_pixel"] >= 2


def test_synthetic_grids_negative_votes_and_the_order_by_pixel(c3):
    """Three rolls, grids installed through the re-vote hook, a frame with one point in the middle of every cell.  (a) votes that are
    nowhere positive: the label over the negative pixels is found with min_vote = -100 and not with 1; a label of ONE pixel whose cell
    is a corner of the grid: its pose's h_locmax is the clipped 9 x 8 window of the re-voted heights by the independent mirror
    vote_cases.z_key, bit for bit (the pose and haf_cell_pose share their device code: their equality says nothing about the window);
    (b) a uniform grid: labels whose picks share vote and roll are ranked by v, then u."""
    eng, inp = c3["eng"], c3["inp"]
    gi = capi.default_input(grasp_area_length_x=54, grasp_area_length_y=54)
    eng.score_rolls([TINY], [gi], 0, 3)
    frame, img = cell_centre_frame(56)
    rows = np.zeros((56, 56), np.int8)
    rows[::3] = -1                                           # every third row -1: no vote is positive, the rows' own votes are negative
    rng = np.random.RandomState(7)                           # heights around -10 and 0, another grid per roll, zeros of both signs
    heights = rng.uniform(-11.0, 1.0, size=(1, 3, 56, 56)).astype(np.float32)
    heights[rng.uniform(size=heights.shape) < 0.03] = 0.0
    heights[rng.uniform(size=heights.shape) < 0.03] = -0.0
    eng.revote(labels=np.stack([rows, np.roll(rows, 1, axis=0), rows.T.copy()]).reshape(1, 3, 56, 56), heights=heights)
    maps = eng.grasp_map(0, frame)
    vote, roll, cell = maps["vote"], maps["roll"], maps["cell"]
    neg = (vote < 0) & (roll >= 0)
    assert vote[roll >= 0].max() <= 0 and neg.sum() > 50 and vote[neg].min() >= -100
    labels = np.where(neg, 1, 2).astype(np.uint8)
    labels[roll < 0] = 0
    corners = (0, 55, 55 * 56, 56 * 56 - 1)
    at_corner = np.argwhere((roll >= 0) & np.isin(cell, corners))
    assert len(at_corner) >= 1                               # (a corner cell scores 0, the border's vote: found with min_vote = -100 only)
    cv, cu = (int(x) for x in at_corner[0])
    labels[cv, cu] = 3
    for mv in (1, -100):
        r = check_labels(eng, 0, gi, 0, 3, frame, img, labels, 3, mv, "negative votes, min_vote %d" % mv, maps=maps)
        check_poses(eng, 0, r)
        assert (1 in r["order"]) == bool(r["picks"]["found"][0]) == (mv == -100) and (mv == -100 or r["order"] == []), (mv, r["order"])
        assert r["order"][-1:] == ([1] if mv == -100 else [])                 # behind the label of the zero votes, when that one has pixels
        if mv == -100:
            p = r["picks"][2]
            assert p["found"] and (int(p["u"]), int(p["v"]), int(p["cell"])) == (cu, cv, int(cell[cv, cu])) and int(p["roll"]) == int(roll[cv, cu])
            want = vc.z_key(heights[0, int(p["roll"])], int(p["cell"]) // 56, int(p["cell"]) % 56)
            got = np.float32(r["poses"][2]["h_locmax"])
            print("corner cell %d of roll %d: h_locmax %r, the mirror %r" % (p["cell"], p["roll"], got, want))
            assert want > -10.0 and got.view(np.uint32) == np.float32(want).view(np.uint32)
    assert eng.best_per_label(0, frame, labels, min_vote=-100)["picks"]["vote"][0] < 0
    # (b)
    eng.revote(labels=np.ones((1, 3, 56, 56), np.int8))
    maps = eng.grasp_map(0, frame)
    flat = (maps["vote"] == maps["vote"].max()) & (maps["roll"] == 0)
    assert flat[10, 40:46].all() and flat[20, 10:16].all() and flat[20, 30:36].all() and maps["vote"].max() > 0
    labels = np.zeros((56, 56), np.uint16)
    labels[20, 30:36], labels[20, 10:16], labels[10, 40:46] = 1, 2, 3
    r = check_labels(eng, 0, gi, 0, 3, frame, img, labels, 3, 1, "identical votes and rolls", maps=maps)
    check_poses(eng, 0, r)
    p = r["picks"]
    assert r["order"] == [3, 2, 1] and len(set(p["vote"])) == 1 and len(set(p["roll"])) == 1
    assert [(int(q["u"]), int(q["v"])) for q in p] == [(30, 20), (10, 20), (40, 10)] and (p["n_pixels"] == 6).all()


def test_second_request_of_a_batch_on_a_roll_subrange(c3, table1):
    """score_rolls([t, t], ..., 7, 6): request 1 answers from its own grids, with global roll indices 7..12"""
    eng, inp, fa, da = c3["eng"], c3["inp"], c3["fa"], c3["da"]
    other = capi.default_input(**dict(C3_IN, approach_vector=(0.1, -0.1, 1.0), gripper_opening_width=2))
    eng.score_rolls([table1, table1], [inp, other], 7, 6)
    b80 = lc.blocks80()
    got = [check_labels(eng, b, gi, 7, 6, fa, da, b80, 48, 1, "request %d" % b) for b, gi in ((0, inp), (1, other))]
    for b, r in enumerate(got):
        check_poses(eng, b, r)
        found = r["picks"][r["picks"]["found"] == 1]
        # (haf_label_best_ref on the CPU oracle's grids of rolls 7..12 finds 17 labels for the first input and 8 for the tilted one: half of each)
        assert len(found) >= (9, 4)[b] and set(found["roll"]) <= set(range(7, 13)) and len(set(found["roll"])) >= 2
    assert (got[0]["picks"] != got[1]["picks"]).any()


def test_roi_request_gives_the_full_request_s_picks(c3):
    """After haf_score_frames_roi with the mask labels != 0 the picks and the order are those after haf_score_frames, the poses equal
    except for n_evals"""
    eng, inp, fa, da = c3["eng"], c3["inp"], c3["fa"], c3["da"]
    v, u = np.mgrid[0:480, 0:640]
    labels = np.where((u // 40) % 2 == 0, lc.blocks80(), 0).astype(np.uint8)
    full_out = c3["score"]()
    full = check_labels(eng, 0, inp, 0, 20, fa, da, labels, 48, 1, "full request", variants=False)
    roi_out = eng.score_frames_roi([fa], [(labels != 0).astype(np.uint8)], [inp])[0]
    roi = check_labels(eng, 0, inp, 0, 20, fa, da, labels, 48, 1, "ROI request", variants=False)
    assert 0 < roi_out["n_evals"] < full_out["n_evals"] and len(full["order"]) >= 7      # (15 on the CPU oracle's grids: half)
    assert (roi["picks"] == full["picks"]).all() and roi["order"] == full["order"]
    differ = 0
    for a, b in zip(roi["poses"], full["poses"]):
        assert (a is None) == (b is None)
        if a is not None:
            assert {k: x for k, x in a.items() if k != "n_evals"} == {k: x for k, x in b.items() if k != "n_evals"}
            differ += a["n_evals"] != b["n_evals"]
    assert differ > 0


def test_label_calls_leave_the_last_batch_as_it_was(c3, table1):
    """haf_top_grasps, haf_get_roll_grid, haf_last_* and haf_debug_fetch* return after label calls -- host and device frames, host and
    device labels, 48 and 4096 labels -- what they returned before; a request whose budget was negative finds nothing"""
    eng, inp, fa, da = c3["eng"], c3["inp"], c3["fa"], c3["da"]
    out = c3["score"]()
    before = full_state(eng, out)
    for labels, n in ((lc.blocks80(), 48), (lc.interleave(4096), 4096)):
        assert eng.best_per_label(0, fa, labels)["order"]
        dl, keep = device_labels(labels, labels.shape[1] * labels.itemsize + 60, offset=2)
        assert eng.best_per_label(0, device_copy(fa, da), dl, n_labels=n)["order"]
    after = full_state(eng, out)
    assert before.keys() == after.keys()
    for k in before:
        assert before[k] == after[k], k
    neg = capi.default_input(max_calculation_time=-1.0, **C3_IN)
    eng.score_batch([table1, table1], [neg, inp])
    none = eng.best_per_label(0, fa, lc.blocks80())
    assert none["order"] == [] and not none["picks"]["found"].any() and (none["picks"]["vote"] == gm.NO_CELL).all() and \
        (none["picks"]["cell"] == -1).all() and (none["picks"]["n_pixels"] == 0).all() and none["poses"] == [None] * 48
    assert len(eng.best_per_label(1, fa, lc.blocks80())["order"]) >= 10


def test_engine_side_refusals_leave_the_engine_as_it_was(data_dir, surrogate, golden_dir, tmp_path, table1):
    """Every refusal of haf_grasp_map_labels returns its code and a text, writes nothing, and leaves the last-batch state and the next
    answer untouched"""
    import json
    import models
    L = capi.testlib()
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    da = render_depth(table1, CAM_A)[:40, :64].copy()
    da[da == 0] = 900
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=4096)
    h = eng._h
    inp = capi.default_input(**C3_IN)
    lab = lc.interleave(6, 64, 40)
    picks = np.full(8, 7, capi.LABEL_PICK_DTYPE)
    poses = (capi.GraspCandidate * 8)()
    C.memset(poses, 0x11, C.sizeof(poses))
    order, nf = np.full(8, 7, np.int32), C.c_int32(7)

    def image(data=lab.ctypes.data, eb=2, dev=0, stride=128):
        return capi.LabelImage(data, eb, dev, stride)

    def rc_of(request=0, frame=fa, img=image(), n=6, out=picks.ctypes.data):
        return L.haf_grasp_map_labels(h, request, C.byref(frame) if frame else None, C.byref(img) if img else None, n, 1, out, poses,
                                      order.ctypes.data, C.byref(nf))

    def untouched():
        return all((picks[f] == 7).all() for f in lc.FIELDS) and (order == 7).all() and nf.value == 7 and bytes(poses) == b"\x11" * C.sizeof(poses)
    assert rc_of() == A and b"no scored batch" in L.haf_last_error(h)
    assert L.haf_grasp_map_labels(None, 0, C.byref(fa), C.byref(image()), 6, 1, picks.ctypes.data, None, None, None) == A
    small = np.ascontiguousarray(table1[::30])                                # (max_points = 4096)
    out = eng.score(small, inp)
    ref_state = full_state(eng, out)
    ref = eng.best_per_label(0, fa, lab)
    big = capi.depth_frame(np.ones((65, 64), np.uint16), **K525)               # 4160 pixels > max_points
    checks = [(rc_of(request=1), A), (rc_of(request=-1), A), (rc_of(frame=None), A), (rc_of(frame=big), CAP),
              (rc_of(img=None), A), (rc_of(img=image(data=None)), A), (rc_of(out=None), A),
              (rc_of(img=image(eb=0)), A), (rc_of(img=image(eb=3)), A), (rc_of(img=image(eb=4)), A),
              (rc_of(img=image(stride=126)), A), (rc_of(img=image(stride=129)), A), (rc_of(img=image(eb=1, stride=63)), A),
              (rc_of(img=image(data=lab.ctypes.data + 1)), A), (rc_of(img=image(dev=2)), A), (rc_of(img=image(dev=-1)), A),
              (rc_of(n=0), A), (rc_of(n=-1), A), (rc_of(n=capi.MAX_LABELS + 1), A)]
    for i, (rc, code) in enumerate(checks):
        assert rc == code and L.haf_last_error(h), (i, rc, code)
    for name, frame, code, _ in fc.refusal_frames():
        assert rc_of(frame=frame) == code and L.haf_last_error(h), name
    assert untouched()
    now = full_state(eng, out)
    assert now.keys() == ref_state.keys()
    for k in ref_state:
        assert now[k] == ref_state[k], k
    again = eng.best_per_label(0, fa, lab)
    assert (again["picks"] == ref["picks"]).all() and again["order"] == ref["order"] and again["poses"] == ref["poses"]
    # poses, order and n_found may be left out
    assert L.haf_grasp_map_labels(h, 0, C.byref(fa), C.byref(image()), 6, 1, picks.ctypes.data, None, None, None) == capi.HAF_OK
    assert (picks[:6] == ref["picks"]).all() and (picks["found"][6:] == 7).all()
    eng.close()
    # probability mode: fp32 votes, no map
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as fh:
        pj = json.load(fh)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    prob = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=1 << 18)
    prob.score(table1, inp)
    with pytest.raises(capi.HafError) as ei:
        prob.best_per_label(0, fa, lab)
    assert ei.value.code == A and "PROBABILITY" in str(ei.value)
    prob.close()


def assert_object_lines(lines, objects, scale, name):
    """lines: the CLI's "object <label> <u> <v> <hypothesis>" lines; objects: [(label, candidate dict, u, v)] in rank order.  The integers
    are compared exactly, the nine floats of grasp points 1 and 2 and the approach vector as the "%g" text allows (6 significant digits)"""
    assert len(lines) == len(objects), (name, len(lines), len(objects))
    for line, (l, c, pu, pv) in zip(lines, objects):
        t = line.split()
        assert t[0] == "object" and [int(x) for x in t[1:5]] == [l * scale, pu, pv, c["eval"]], (name, line)
        np.testing.assert_allclose([float(x) for x in t[5:14]], list(c["grasp_point1"]) + list(c["grasp_point2"]) + list(c["approach_vector"]),
                                   rtol=1e-5, atol=1e-6)


def engine_objects(eng, frame, labels):
    res = eng.best_per_label(0, frame, labels)
    return [(l, res["poses"][l - 1], int(res["picks"]["u"][l - 1]), int(res["picks"]["v"][l - 1])) for l in res["order"]]


def test_cli_prints_one_line_per_object(data_dir, surrogate, tmp_path, table1):
    """haf_grasp_cli --depth ... --labels FILE.pgm, 8- and 16-bit: after the normal output one "object <label> <u> <v> <hypothesis>"
    line per found object, in rank order, built from haf_grasp_map_labels for the same goal; with --roi-mask the same objects; also
    through the Python mirror of the action server"""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    da = render_depth(table1, CAM_A)
    pa, p8, p16, proi = (str(tmp_path / n) for n in ("a.pgm", "lab8.pgm", "lab16.pgm", "roi.pgm"))
    fc.write_pgm16(pa, da)
    v, u = np.mgrid[0:480, 0:640]
    labels = np.where((u // 40) % 2 == 0, lc.blocks80(), 0).astype(np.uint8)
    with open(p8, "wb") as f:
        f.write(b"P5\n# instance labels\n640 480\n255\n" + labels.tobytes())
    fc.write_pgm16(p16, labels.astype(np.uint16) * 50, maxval=65535)           # labels 50, 100, .. 2400: most slots of the table stay empty
    with open(proi, "wb") as f:
        f.write(b"P5 640 480 255\n" + ((labels != 0) * np.uint8(255)).astype(np.uint8).tobytes())
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % x for x in CAM_A]
    plain = subprocess.run(common, check=True, capture_output=True, text=True).stdout
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    frame = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    res = srv.execute_frame(goal, frame)
    assert int(plain.splitlines()[-1].split()[0]) == res.eval > 50
    objects = srv.best_per_object(frame, labels)
    assert len(objects) >= 7
    want = engine_objects(srv.engine, frame, labels)
    assert [(l, m.eval, m.graspPoint1, pu, pv) for l, m, pu, pv in objects] == [(l, c["eval"], c["grasp_point1"], pu, pv) for l, c, pu, pv in want]
    for path, scale in ((p8, 1), (p16, 50)):
        run = subprocess.run(common + ["--labels", path], check=True, capture_output=True, text=True).stdout
        assert run.startswith(plain)
        assert_object_lines(run[len(plain):].splitlines(), want, scale, path)
    roi_res, roi_objects = srv.execute_frame_objects(goal, frame, labels)
    assert [(l, pu, pv, m.eval, m.graspPoint1) for l, m, pu, pv in roi_objects] == [(l, pu, pv, m.eval, m.graspPoint1) for l, m, pu, pv in objects]
    run = subprocess.run(common + ["--labels", p8, "--roi-mask", proi], check=True, capture_output=True, text=True).stdout.splitlines()
    assert_object_lines([ln for ln in run if ln.startswith("object ")], engine_objects(srv.engine, frame, labels), 1, "with --roi-mask")
    empty = str(tmp_path / "empty.pgm")
    with open(empty, "wb") as f:
        f.write(b"P5 640 480 255\n" + bytes(640 * 480))
    assert subprocess.run(common + ["--labels", empty], check=True, capture_output=True, text=True).stdout == plain
    # a segmenter that found nothing: no objects, with n_labels left to its default too
    zero = np.zeros((480, 640), np.uint8)
    assert srv.best_per_object(frame, zero, n_labels=1) == [] and srv.best_per_object(frame, zero) == []
    none = srv.engine.best_per_label(0, frame, zero)
    assert none["order"] == [] and none["poses"] == [None] and len(none["picks"]) == 1 and not none["picks"]["found"].any()
    res0, objects0 = srv.execute_frame_objects(goal, frame, zero)
    assert objects0 == [] and res0.eval == -20
    # labels without a depth image are a usage error
    assert subprocess.run([cli, "--features", f_, "--range", r_, "--model", surrogate, "--labels", p8, os.path.join(data_dir, "pcd2.pcd")],
                          capture_output=True, text=True).returncode == 2
    srv.close()
