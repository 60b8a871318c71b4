"""haf_score_views_roi on the MI355X (include/hafgrasp.h; csrc/roi.hip: k_roi_mark_view): a fused request of several views scored only
near the cells of the masked pixels of its masked views.  One view against haf_score_frames_roi; two cameras at C3 against the CPU
oracle's full run on the fused cloud -- ROI cells, evaluated cells, labels, vote grids, records, output -- in every residence and
order; a view without a mask; empty ROIs; the marking kernel on every kind, shape and stride against haf_roi_cells_views; rows of
several 64-bit words on a larger grid against the engine's own full haf_score_views; a batch against its requests one by one; the
state behind a call, the refusals; the CLI and the server.  Every comparison is an equality.  Testing build throughout; the guard zones
around every device buffer are checked after every request and after each test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import models
import roi_cases as rc
import views_roi_cases as vr
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import oracle_input
from test_frames_gpu import C3_CFG, C3_IN, K525, _files, device_copy, make_engine, render_depth, snapshot
from test_grasp_map_gpu import full_state
from test_roi_gpu import _canaries, check_roi_state, device_mask, expected, orc, strip, surrogate, table1  # noqa: F401  (fixtures)
from test_views_gpu import CAM_A, CAM_B, pose, tilt, view_sets

pytestmark = pytest.mark.gpu

H = W = 56
POSE = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector", "roll", "eval", "best_row", "best_col", "best_roll", "best_vote")


@pytest.fixture(scope="module")
def cams(table1):
    """table1 from CAM_A and CAM_B -> (frames, images, words of the pixels' points, masks): roi_cases.C3_RECT in A, in B the valid pixels
    whose base-frame (x, y) lies in the bounding box of A's masked points; computed once, never written"""
    imgs = [render_depth(table1, CAM_A), render_depth(table1, CAM_B)]
    frames = [capi.depth_frame(imgs[0], sensor_to_base=CAM_A, **K525), capi.depth_frame(imgs[1], sensor_to_base=CAM_B, **K525)]
    words = [fc.mirror_points(f, i) for f, i in zip(frames, imgs)]
    ma = vr.rect_mask(rc.C3_RECT, 480, 640)
    return frames, imgs, words, [ma, vr.bbox_mask(words[0], ma, words[1], 480, 640)]


@pytest.fixture(scope="module")
def c3_fused(orc, cams):
    """the CPU oracle's full request on the fused cloud of the two cameras at C3; computed once, never written"""
    return orc.run(capi.view_points(cams[0]), O.make_cfg(**C3_CFG), oracle_input(C3_IN))


def joined(words, masks):
    """the views' points and masks one after the other, as roi_cases.mirror_roi takes one frame's: the union of the views' cell sets"""
    ms = [np.zeros(len(w), np.uint8) if m is None else np.asarray(m).reshape(-1) for w, m in zip(words, masks)]
    return np.concatenate(words), np.concatenate(ms)


def roi_grids(eng, request, R):
    return np.stack([eng.debug(capi.DBG_ROI, request, r) for r in range(R)])


def state(eng, out, request=0):
    """what the issue compares between two ROI calls: the output without n_rechecked, every roll grid, DBG_MASK, DBG_LABELS, DBG_ROI,
    the heights and haf_top_grasps"""
    s = dict(out=strip(out), top=eng.top_grasps(k=16)[request])
    for r in range(eng.cfg.n_rolls):
        ev, m = eng.roll_grid(request, r)
        s[r] = (ev.tobytes(), m.tobytes()) + tuple(eng.debug(w, request, r).tobytes() for w in (capi.DBG_MASK, capi.DBG_LABELS, capi.DBG_ROI, capi.DBG_HEIGHTS))
    return s


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k] == b[k], (what, k)


def test_one_view_equals_score_frames_roi(data_dir, surrogate, cams):
    """One view under its mask is haf_score_frames_roi on that frame and mask: every output field except n_rechecked, every roll grid,
    DBG_MASK, DBG_LABELS, DBG_ROI and haf_top_grasps; for a host mask and for a device mask with a padded stride, the frame host- and
    device-resident"""
    frames, imgs, words, masks = cams
    eng = make_engine(data_dir, surrogate, max_points=640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    dm, keep = device_mask(masks[0])
    dev = device_copy(frames[0], imgs[0])
    for how, m in (("host mask", masks[0]), ("device mask", dm)):
        want = state(eng, eng.score_frames_roi([frames[0]], [m], [inp])[0])
        assert want["out"]["best_vote"] == 93 and want["out"]["n_evals"] == 6368           # (roi_cases.C3_RECT on camera A's own grids)
        for f in (frames[0], dev):
            outs, counts = eng.score_views_roi([[f]], [[m]], [inp])
            assert counts == [len(capi.view_points([frames[0]]))]
            same(state(eng, outs[0]), want, how)
    eng.close()


def test_two_views_equal_the_oracle_restricted_to_the_union(data_dir, surrogate, cams, c3_fused):
    """table1 from CAM_A + CAM_B at C3, the rectangle in A and the bounding-box mask in B, against the CPU oracle's full run on
    haf_view_points of the two frames: DBG_ROI is S, DBG_MASK is dilate(S) & the full mask, the labels are the oracle's on E and -1
    elsewhere, the roll grids V on S and 0 elsewhere, records and output test_roi_gpu.expected's construction.  On the oracle:
    sum |S_r| = 4 410, sum |E_r| = 7 395 of 31 093, best vote 87.  Host / device residences of frames and masks, mixed, and the views
    in the other order all leave the same state."""
    frames, imgs, words, masks = cams
    full = c3_fused
    eng = make_engine(data_dir, surrogate, max_points=2 * 640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    jw, jm = joined(words, masks)
    want = expected(eng, inp, full["M"], jw, jm, full["mask"], full["labels"], full["graspseval"], full["heights"])
    S, E, votes = want[0], want[1], want[3]
    assert (int(S.sum()), int(E.sum()), full["n_evals"], int(votes.max())) == (4410, 7395, 31093, 87)
    assert 0 < E.sum() < full["n_evals"] / 2 and votes.max() > 0
    # the best vote is the maximum of the FULL request's grasp map over both views' masked pixels
    outs, counts = eng.score_views([frames], [inp])
    n_valid = len(capi.view_points(frames))
    assert counts == [n_valid] and outs[0]["n_evals"] == full["n_evals"]
    map_best = max(int(eng.grasp_map(0, f)["vote"][m != 0].max()) for f, m in zip(frames, masks))
    assert map_best == int(votes.max())
    dev = [device_copy(f, i) for f, i in zip(frames, imgs)]
    dms = [device_mask(m) for m in masks]
    ref = None
    for how, fs, ms in (("host/host", frames, masks), ("device/device", dev, [d[0] for d in dms]), ("mixed", [frames[0], dev[1]], [dms[0][0], masks[1]]),
                        ("other order", [dev[1], frames[0]], [masks[1], masks[0]])):
        outs, counts = eng.score_views_roi([fs], [ms], [inp])
        got = outs[0]
        assert counts == [n_valid], how
        check_roi_state(eng, 0, got, want, how)
        assert (roi_grids(eng, 0, 20) == S).all(), how
        assert got["n_evals"] == int(E.sum()) == eng.last_counts()["n_evals"] and got["best_vote"] == map_best, how
        now = state(eng, got)
        if ref is None:
            ref = now
        same(now, ref, how)
    eng.close()


def test_an_unmasked_view_still_shapes_the_scene(data_dir, surrogate, cams, c3_fused):
    """A masked, B without a mask: S is S_A (3 800 cells, 6 368 evaluations) but labels and votes are the FUSED scene's, best vote 87 --
    not what haf_score_frames_roi on A alone finds on camera A's own height grids, best vote 93"""
    frames, imgs, words, masks = cams
    full = c3_fused
    eng = make_engine(data_dir, surrogate, max_points=2 * 640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    jw, jm = joined(words, [masks[0], None])
    want = expected(eng, inp, full["M"], jw, jm, full["mask"], full["labels"], full["graspseval"], full["heights"])
    assert (int(want[0].sum()), int(want[1].sum()), int(want[3].max())) == (3800, 6368, 87)
    assert (want[0] == rc.mirror_roi(full["M"], words[0], masks[0], H, W)).all()
    alone = eng.score_frames_roi([frames[0]], [masks[0]], [inp])[0]
    alone_state = state(eng, alone)
    dm, keep = device_mask(masks[0])                      # (keep: the tensor behind the pointer)
    for fs, ms in ((frames, [masks[0], None]), ([frames[1], frames[0]], [None, dm])):
        got = eng.score_views_roi([fs], [ms], [inp])[0][0]
        check_roi_state(eng, 0, got, want, "B unmasked")
        assert (roi_grids(eng, 0, 20) == want[0]).all()
        assert got["best_vote"] == 87 and alone["best_vote"] == 93
        now = state(eng, got)
        assert all(now[r][4] == alone_state[r][4] for r in range(20))                        # the same ROI cells ...
        assert any(now[r][0] != alone_state[r][0] for r in range(20)) and any(now[r][3] != alone_state[r][3] for r in range(20))   # ... other votes, other labels
        assert any(now[r][5] != alone_state[r][5] for r in range(20)) and now["out"] != alone_state["out"]
    eng.close()


def test_an_empty_roi_is_nothing_found(data_dir, surrogate, cams):
    """every mask NULL, all zeros, or over invalid pixels only: eval -20, n_evals 0, HAF_OK, and n_points still counts the cloud"""
    frames, imgs, words, masks = cams
    eng = make_engine(data_dir, surrogate, max_points=2 * 640 * 480, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    n_valid = len(capi.view_points(frames))
    zeros = np.zeros((480, 640), np.uint8)
    invalid = [(~np.isfinite(vr.points(w)).all(axis=1)).astype(np.uint8).reshape(480, 640) for w in words]
    assert all(m.any() for m in invalid)
    dz, keep = device_mask(zeros)                         # (keep: the tensor behind the pointer)
    for name, ms in (("null", [None, None]), ("zeros", [zeros, dz]), ("invalid", invalid), ("zeros and null", [zeros, None])):
        outs, counts = eng.score_views_roi([frames], [ms], [inp])
        assert counts == [n_valid] and n_valid > 80000, name
        assert (outs[0]["eval"], outs[0]["n_evals"], outs[0]["best_vote"]) == (-20, 0, 0), (name, outs[0])
        assert not roi_grids(eng, 0, 20).any() and eng.last_counts()["n_evals"] == 0
        assert not any(eng.debug(capi.DBG_MASK, 0, r).any() for r in range(20))
    eng.close()


def recentred(frame, like=None):
    """a copy of `frame` (of `like`'s pose when given) whose translation puts the xy median of its finite points at the origin, so that
    the grid catches them"""
    g = capi.Frame.from_buffer_copy(frame)
    for name in ("_keep",):
        if hasattr(frame, name):
            setattr(g, name, getattr(frame, name))
    if like is not None:
        for k in range(12):
            g.sensor_to_base[k] = like.sensor_to_base[k]
        return g
    pts = capi.frame_points(frame)
    ok = np.isfinite(pts).all(axis=1)
    if ok.any():
        c = np.median(pts[ok].astype(np.float64), axis=0)
        g.sensor_to_base[3] = np.float32(frame.sensor_to_base[3] - c[0])
        g.sensor_to_base[7] = np.float32(frame.sensor_to_base[7] - c[1])
    return g


def test_marking_kernel_equals_the_host_definition_on_every_shape(data_dir, surrogate):
    """DBG_ROI == haf_roi_cells_views for every roll, on the view triples of test_views_gpu.view_sets(): all three kinds, every shape,
    padded rows, 640 x 480 one element off a 16-byte boundary (every group read pixel by pixel), widths 1..17 (groups across rows, the
    tail group), host, device and mixed residence -- under all-ones and seeded random masks, host masks and device masks with a padded
    stride.  A 200 x 200 grid (rows of four 64-bit words), 3 rolls, the grasp area the whole grid; every view's pose is moved so that
    its points lie around the origin (the median of x and of y at 0), or the grid would see none of them."""
    cfg_kw = dict(grid_h=200, grid_w=200, n_rolls=3, roll_step_deg=40)
    eng = make_engine(data_dir, surrogate, max_points=4 * 640 * 480, **cfg_kw)
    cfg, inp = eng.cfg, capi.default_input(grasp_area_length_x=200, grasp_area_length_y=200)
    rng = np.random.default_rng(8)
    marked_kinds = small_marked = device_masks = cases = 0
    for name, host, use in view_sets():
        host = [recentred(f) for f in host]
        use = [recentred(u, like=h) for u, h in zip(use, host)]
        for which in ("ones", "random"):
            if which == "ones":
                masks = [np.ones((f.height, f.width), np.uint8) for f in host]
            else:
                masks = [(rng.random((f.height, f.width)) < 0.3).astype(np.uint8) * np.uint8(rng.integers(1, 256)) for f in host]
            want = np.stack([capi.roi_cells_views(cfg, inp, r, host, masks, want=("roi",))["roi"] for r in range(3)])
            given, keep = [], []
            for k, m in enumerate(masks):
                if (cases + k) % 2:
                    dm, kp = device_mask(m, pad=(cases + k) % 5 + 1)
                    given.append(dm)
                    keep.append(kp)
                    device_masks += 1
                else:
                    given.append(m)
            outs, counts = eng.score_views_roi([use], [given], [inp])
            got = roi_grids(eng, 0, 3)
            assert (got == want).all(), (name, which, int((got != want).sum()), int(want.sum()))
            assert counts == [len(capi.view_points(host))], (name, which)
            if want.any():
                for f, m in zip(host, masks):
                    if capi.roi_cells_views(cfg, inp, 0, [f], [m], want=("roi",))["roi"].any():
                        marked_kinds |= 1 << f.kind       # (a bit per kind: two views of one kind are still that kind)
                small_marked += all(f.width <= 17 for f in host)
            cases += 1
    assert cases >= 2 * 3 * 27 and marked_kinds == 7 and small_marked >= 10 and device_masks >= cases, (cases, marked_kinds, small_marked, device_masks)
    eng.close()


def two_synthetic_cameras(grid):
    xyz = models.synthetic_cloud(grid=grid, k=3, seed=2)
    cam0 = np.array([1, 0, 0, 0.0, 0, -1, 0, 0.0, 0, 0, -1, 1.5], np.float32)
    cam1 = pose(tilt(0.22, -0.16, 0.5), (0.25, -0.2, 1.45))
    imgs = [render_depth(xyz, cam0), render_depth(xyz, cam1)]
    frames = [capi.depth_frame(imgs[0], sensor_to_base=cam0, **K525), capi.depth_frame(imgs[1], sensor_to_base=cam1, **K525)]
    return frames, imgs, [fc.mirror_points(f, i) for f, i in zip(frames, imgs)]


def test_rows_of_several_words_equal_the_full_views_request_restricted(data_dir, tmp_path):
    """131 x 131 (rows of three 64-bit ROI words, the last one partial), 8 rolls, a random 64-SV model, the synthetic cloud seen from two
    cameras: against the engine's own full haf_score_views, which the other suites pin to the oracle.  The rectangle in view 0 lies
    around the best pixel of the full request's grasp map and runs on to the image's right edge, so that the cell sets reach the rows'
    last word; view 1 is masked by the bounding-box rule.  DBG_ROI is exactly the mirror's
    and the host definition's union and has cells in columns >= 64 and >= 128; labels, votes, records and output follow from the full
    request's grids; the full request afterwards is what it was."""
    grid, R = 131, 8
    model = models.write_random_model(str(tmp_path / "m64.model"), 64, seed=5, balanced=True)
    cfg_kw = dict(grid_h=grid, grid_w=grid, n_rolls=R, roll_step_deg=20)
    in_kw = dict(grasp_area_length_x=grid, grasp_area_length_y=grid)
    frames, imgs, words = two_synthetic_cameras(grid)
    eng = make_engine(data_dir, model, max_points=2 * 640 * 480, **cfg_kw)
    inp = capi.default_input(**in_kw)
    full_out = eng.score_views([frames], [inp])[0][0]
    before = snapshot(eng, full_out)
    fm = np.stack([eng.debug(capi.DBG_MASK, 0, r) for r in range(R)])
    fl = np.stack([eng.debug(capi.DBG_LABELS, 0, r) for r in range(R)])
    fh = np.stack([eng.debug(capi.DBG_HEIGHTS, 0, r) for r in range(R)])
    fv = np.stack([eng.roll_grid(0, r)[0] for r in range(R)])
    assert full_out["n_evals"] >= R * 10000 and (fv > 0).any() and (fl == 1).any()
    maps = [eng.grasp_map(0, f) for f in frames]
    bu, bv = gm.key_argmax(maps[0]["vote"], maps[0]["roll"], None, 1)
    ma = vr.rect_mask((max(0, bv - 60), min(480, bv + 60), max(0, bu - 80), 640), 480, 640)      # (on to the image's edge: the grid's last columns)
    masks = [ma, vr.bbox_mask(words[0], ma, words[1], 480, 640)]
    assert masks[1].any()
    Ms = rc.oracle_transforms(cfg_kw, in_kw, 0, R)
    jw, jm = joined(words, masks)
    want = expected(eng, inp, Ms, jw, jm, fm, fl, fv, fh)
    S, E = want[0], want[1]
    host_def = np.stack([capi.roi_cells_views(eng.cfg, inp, r, frames, masks, want=("roi",))["roi"] for r in range(R)])
    assert (host_def == S).all()
    assert S[:, :, 64:128].any() and S[:, :, 128:].any() and S[:, :, :64].any()
    best = max(int(m["vote"][k != 0].max()) for m, k in zip(maps, masks))
    assert 0 < E.sum() < full_out["n_evals"] / 2 and int(want[3].max()) == best > 0
    dev = [device_copy(f, i) for f, i in zip(frames, imgs)]
    dms = [device_mask(m) for m in masks]                 # ((pointer, stride), the tensor behind it) per view, alive to the end
    for how, fs, ms in (("host", frames, masks), ("device", dev, [d[0] for d in dms])):
        got = eng.score_views_roi([fs], [ms], [inp])[0][0]
        check_roi_state(eng, 0, got, want, "131 " + how)
        assert (roi_grids(eng, 0, R) == S).all(), how
        assert got["best_vote"] == best
    again = eng.score_views([frames], [inp])[0][0]
    after = snapshot(eng, again)
    assert before.keys() == after.keys()
    for key in before:
        assert before[key] == after[key], key
    eng.close()


def test_batch_equals_its_requests_one_by_one(data_dir, surrogate, cams):
    """Three requests in one call -- one view (camera B, device-resident, a device mask), two views (A masked, B without a mask) and two
    views with a negative budget -- with different inputs: the batch equals the requests one by one in the output and in every grid"""
    frames, imgs, words, masks = cams
    dev_b = device_copy(frames[1], imgs[1])
    dm, keep = device_mask(masks[1])
    sets = [[dev_b], [frames[0], frames[1]], [frames[1], frames[0]]]
    msets = [[dm], [masks[0], None], [masks[1], masks[0]]]
    inputs = [capi.default_input(**dict(C3_IN, approach_vector=(0.1, -0.1, 1.0), gripper_opening_width=2)), capi.default_input(**C3_IN),
              capi.default_input(max_calculation_time=-1.0, **C3_IN)]
    eng = make_engine(data_dir, surrogate, max_clouds=3, max_points=5 * 640 * 480, **C3_CFG)
    outs, counts = eng.score_views_roi(sets, msets, inputs)
    batch = [state(eng, outs[b], b) for b in range(3)]
    assert outs[0]["eval"] > -20 and outs[0]["n_evals"] > 0 and outs[1]["best_vote"] == 87 and outs[1]["n_evals"] == 6368
    assert outs[2]["rolls_done"] == 0 and outs[2]["n_evals"] == 0
    assert counts[0] == len(capi.view_points([frames[1]])) and counts[1] == counts[2] == len(capi.view_points(frames))
    assert strip(outs[2]) == strip(eng.score_views([sets[2]], [inputs[2]])[0][0])          # no roll ran: the reference's untouched overall best
    for b in range(3):
        o, c = eng.score_views_roi([sets[b]], [msets[b]], [inputs[b]])
        assert strip(o[0]) == strip(outs[b]), b
        if b == 2:
            assert c == [-1]                              # (alone, a request with a negative budget scores nothing: no last batch, no count)
            continue
        assert c == [counts[b]]
        same(state(eng, o[0]), batch[b], b)
    eng.close()


def test_state_behind_a_call_and_the_refusals(data_dir, surrogate, golden_dir, tmp_path):
    """haf_screen_form is the same before and after a call and the next plain haf_score_views equals one made before; every refusal
    returns its code and a text that names the call, the request and the view, before any device work: the last batch is untouched;
    a view's frame is refused before its mask; HAF_DBG_ROI after a plain request is HAF_E_ARG; HAF_FLAG_PROBABILITY is refused."""
    import json
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    eng = make_engine(data_dir, surrogate, max_clouds=2, max_points=4096)
    L, h = eng._L, eng._h
    inp = capi.default_input()
    rng = np.random.default_rng(4)
    img = fc.u16_image(rng, 61, 5)
    good = capi.depth_frame(img, sensor_to_base=np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0.9], np.float32), **fc._intrinsics(rng, 61, 5))
    mask = np.ones((5, 61), np.uint8)
    form = (eng.screen_form(), eng.screen_state())
    out0 = eng.score_views([[good, good]], [inp])[0][0]
    ref = full_state(eng, out0)
    with pytest.raises(capi.HafError) as ei:
        eng.debug(capi.DBG_ROI, 0, 0)
    assert ei.value.code == A and "ROI" in str(ei.value)
    got = eng.score_views_roi([[good, good]], [[mask, None]], [inp])[0][0]
    assert 0 < got["n_evals"] <= out0["n_evals"] and eng.debug(capi.DBG_ROI, 0, 0).any()
    assert (eng.screen_form(), eng.screen_state()) == form
    again = full_state(eng, eng.score_views([[good, good]], [inp])[0][0])
    assert all(again[k] == ref[k] for k in ref if k != "stage_ms") and (eng.screen_form(), eng.screen_state()) == form

    def roi(m=mask.ctypes.data, stride=61, on_device=0):
        return capi.Roi(m, stride, on_device)

    def refused(n, per, frames, rois, inputs, out, code):
        cnt = (C.c_int64 * 4)(*([-7] * 4))
        rc_ = L.haf_score_views_roi(h, n, per, frames, rois, inputs, out, cnt)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc_ == code and "haf_score_views_roi" in text, (rc_, code, text)
        assert list(cnt) == [-7] * 4
        now = full_state(eng, out0)
        assert all(now[k] == ref[k] for k in ref if k != "stage_ms")
        return text

    per = lambda *v: (C.c_int32 * len(v))(*v)
    three, gi, out = (capi.Frame * 3)(good, good, good), (capi.GraspInput * 2)(inp, inp), (capi.GraspOutput * 2)()
    rr = (capi.Roi * 3)(roi(), roi(), roi())
    for args in ((1, None, three, rr, gi, out), (1, per(2), None, rr, gi, out), (1, per(2), three, None, gi, out), (1, per(2), three, rr, None, out),
                 (1, per(2), three, rr, gi, None), (0, per(2), three, rr, gi, out), (-3, per(2), three, rr, gi, out)):
        refused(*args, A)
    assert L.haf_score_views_roi(None, 1, per(2), three, rr, gi, out, None) == A
    many = (capi.Frame * 17)(*([good] * 17))
    many_r = (capi.Roi * 17)(*([roi()] * 17))
    for v in (0, -1, 17):
        assert "request 0" in refused(1, per(v), many, many_r, gi, out, A)
    assert "request 1" in refused(2, per(1, 0), many, many_r, gi, out, A)
    assert "max_clouds" in refused(3, per(1, 1, 1), many, many_r, (capi.GraspInput * 3)(inp, inp, inp), (capi.GraspOutput * 3)(), CAP)
    half = capi.depth_frame(np.ones((42, 50), np.uint16), **K525)              # 2 x 2100 pixels > 4096, in one request or in two
    halves = (capi.Frame * 2)(half, half)
    big_r = (capi.Roi * 2)(roi(m=None), roi(m=None))
    assert "max_points" in refused(1, per(2), halves, big_r, gi, out, CAP)
    assert "max_points" in refused(2, per(1, 1), halves, big_r, gi, out, CAP)
    for bad in (roi(stride=60), roi(stride=0), roi(on_device=2), roi(on_device=-1)):
        assert "request 0 view 0" in refused(1, per(2), three, (capi.Roi * 3)(bad, roi(), roi()), gi, out, A)
        assert "request 0 view 1" in refused(1, per(2), three, (capi.Roi * 3)(roi(), bad, roi()), gi, out, A)
        assert "request 1 view 1" in refused(2, per(1, 2), three, (capi.Roi * 3)(roi(), roi(), bad), gi, out, A)      # before request 0 is touched
    for name, frame, code, _ in fc.refusal_frames():
        fr = (capi.Frame * 2)(good, frame)
        assert "request 0 view 1" in refused(1, per(2), fr, rr, gi, out, code), name
        # a view's frame before its own mask, but behind the masks of the views in front of it
        text = refused(1, per(2), fr, (capi.Roi * 2)(roi(), roi(stride=1)), gi, out, code)
        assert "request 0 view 1" in text and "haf_roi" not in text, (name, text)
        text = refused(1, per(2), fr, (capi.Roi * 2)(roi(stride=1), roi()), gi, out, A)
        assert "request 0 view 0" in text and "haf_roi" in text, (name, text)
    # a NULL mask's other fields are ignored, and the valid call is served
    rc_ = L.haf_score_views_roi(h, 1, per(2), three, (capi.Roi * 2)(roi(), roi(m=None, stride=0, on_device=9)), gi, out, None)
    assert rc_ == capi.HAF_OK and out[0].n_evals == got["n_evals"]
    eng.close()
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as fh:
        pj = json.load(fh)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    prob = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=4096)
    with pytest.raises(capi.HafError) as ei:
        prob.score_views_roi([[good, good]], [[mask, None]], [inp])
    assert ei.value.code == A and "PROBABILITY" in str(ei.value)
    prob.close()


def test_cli_and_server_score_the_fused_request_under_the_masks(data_dir, surrogate, tmp_path, cams):
    """haf_grasp_cli with two --depth, each with its --view-roi-mask, prints the grasp Engine.score_views_roi returns for the same goal;
    --top-k 2 behind it prints the same line first; CalcGraspPointsServer.execute_views(roi_masks=) agrees.  --roi-mask with two
    --depth stays a usage error, and so is --view-roi-mask in front of the first --depth."""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    frames, imgs, words, masks = cams
    pa, pb, qa, qb = (str(tmp_path / n) for n in ("a.pgm", "b.pgm", "ma.pgm", "mb.pgm"))
    fc.write_pgm16(pa, imgs[0])
    fc.write_pgm16(pb, imgs[1])
    for path, m in ((qa, masks[0]), (qb, masks[1])):
        with open(path, "wb") as f:
            f.write(b"P5\n# an instance mask\n640 480\n255\n" + (m * np.uint8(200)).tobytes())
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5"]
    va = ["--depth", pa, "--sensor-pose"] + ["%.9g" % v for v in CAM_A]
    vb = ["--depth", pb, "--sensor-pose"] + ["%.9g" % v for v in CAM_B]
    plain = subprocess.run(common + va + vb, check=True, capture_output=True, text=True).stdout.splitlines()
    run = subprocess.run(common + va + ["--view-roi-mask", qa] + vb + ["--view-roi-mask", qb, "--top-k", "2"], check=True, capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert len(plain) == 1 and len(lines) in (2, 3) and lines[1].startswith("top 1 ") and lines[1][len("top 1 "):] == lines[0]
    assert "2 views fused: %d valid points" % len(capi.view_points(frames)) in run.stderr
    only_a = subprocess.run(common + va + ["--view-roi-mask", qa] + vb, check=True, capture_output=True, text=True).stdout.splitlines()
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    res = srv.execute_views(goal, frames, roi_masks=masks)
    out = srv.engine.score_views_roi([frames], [masks], [goal.to_c()])[0][0]
    assert int(lines[0].split()[0]) == res.eval == out["eval"] == 87 - 20 and int(plain[0].split()[0]) > res.eval
    line = [float(t) for t in lines[0].split()[1:10]]                        # grasp points 1 and 2, approach vector: "%g" text
    np.testing.assert_allclose(line, list(out["grasp_point1"]) + list(out["grasp_point2"]) + list(out["approach_vector"]), rtol=1e-5, atol=1e-6)
    res_a = srv.execute_views(goal, frames, roi_masks=[masks[0], None])
    assert int(only_a[0].split()[0]) == res_a.eval == 87 - 20
    assert srv.execute_views(goal, frames).eval == int(plain[0].split()[0])
    srv.close()
    assert subprocess.run(common + va + vb + ["--roi-mask", qa], capture_output=True, text=True).returncode == 2
    assert subprocess.run(common + ["--view-roi-mask", qa] + va, capture_output=True, text=True).returncode == 2
    assert subprocess.run(common + va + ["--view-roi-mask", qa, "--roi-mask", qa], capture_output=True, text=True).returncode == 2
