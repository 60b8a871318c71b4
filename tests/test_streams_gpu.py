"""haf_set_stream / haf_get_stream on the MI355X: every call of the interface on a caller's stream, with stream-ordered inputs (the
stream contract of include/hafgrasp.h).  stream_cases.py has the detector -- late inputs, late poison -- and the scene.

The table: every call runs with every device-resident input late and every caller-owned device output poisoned late, on
  torch   a torch.cuda.Stream() (non-blocking: the default stream does not order it by accident),
  null    HIP's default stream, handed over as 0 (torch.cuda.default_stream()),
  own     the engine's own stream, restored through the handle get_stream() gave before a switch; inputs produced on a torch stream and
          joined by wait_stream and one synchronisation (the contract before this one).
Each mode gets a fresh engine, so every first-use allocation of every call happens on that mode's stream with the inputs still late.
Expected values are the host definitions (haf_*_ref) and, for the scoring family, the same call with host-resident inputs on a
second engine that never leaves its own stream -- which test_frames_gpu, test_roi_gpu, test_views*_gpu and test_objects_gpu tie to the
oracle.  Every comparison is an equality of bytes.  At most three streams are alive at a time: two engines' and one torch stream."""
import math
import os

import numpy as np
import pytest

import clearance_cases as cc
import object_cases as oc
import plane_cases as pc
import stream_cases as sc
from haf_grasping_amd import capi
from test_depth_filter_gpu import fetch
from test_frames_gpu import make_engine, snapshot

pytestmark = pytest.mark.gpu

PX, W, H = sc.PX, oc.W, oc.H
MAP_IMAGES = (("vote", 2), ("roll", 2), ("cell", 4))


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries():
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


class Host:
    """the residence of the expected values: every input where it lies on the host, every output a host array; no stream work"""
    host = True

    def frame(self, frame, image):
        return frame

    def rows(self, array):
        return array

    def labels(self, array):
        return array

    def cloud(self, xyz):
        return xyz

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class Ctx:
    """an engine, the mode it runs in and what arms a call in that mode"""

    def __init__(self, tctx, e, mode, own=None):
        self.torch, self.S, self.cycles = tctx
        self.e, self.mode = e, mode
        self.joined = None
        if own is not None:                               # the engine is in this mode already
            self.own = own
            if mode == "own":
                self.joined = self.torch.cuda.ExternalStream(own)
            return
        self.own = e.get_stream()
        if mode == "torch":
            e.set_stream(self.S.cuda_stream)
        elif mode == "null":
            e.set_stream(0)
        elif mode == "own":
            e.set_stream(self.S.cuda_stream)              # away from the own stream and back through the saved handle
            e.set_stream(self.own)
            self.joined = self.torch.cuda.ExternalStream(self.own)
        want = dict(torch=self.S.cuda_stream, null=0, own=self.own)[mode]
        assert e.get_stream() == want, (mode, e.get_stream(), want)

    def late(self, **kw):
        stream = self.torch.cuda.default_stream() if self.mode == "null" else self.S
        return sc.Late(self.torch, stream, self.cycles, joined=self.joined, **kw)


@pytest.fixture(scope="module")
def tctx():
    """(torch, the module's one torch stream, the calibrated cycle count of the delay)"""
    import torch
    S = torch.cuda.Stream()
    cycles, cal = sc.calibrate_sleep(torch, S)
    print("stream delay calibration: %r" % (cal,))
    return torch, S, cycles


_TABLE = {}


def release_table_engine():
    ctx = _TABLE.pop("ctx", None)
    if ctx is not None:
        ctx.e.close()


def table_ctx(mode, data_dir, surrogate, tctx):
    """the table's engine of `mode`: created when the mode is first asked for, the previous mode's closed before"""
    ctx = _TABLE.get("ctx")
    if ctx is None or ctx.mode != mode:
        release_table_engine()
        ctx = _TABLE["ctx"] = Ctx(tctx, make_engine(data_dir, surrogate, **sc.ENGINE_KW), mode)
    return ctx


@pytest.fixture(scope="module", autouse=True)
def _close_table_engine():
    yield
    release_table_engine()


# ---- the rows: row(e, s, mk) -> something comparable; mk() gives the residence of one call (a Late to arm, or Host) -----------------------

def packed_rows(flat, width_bytes, stride, height):
    return np.stack([flat[v * stride:v * stride + width_bytes] for v in range(height)])


def base_batch(e, s):
    """the scored batch the last-batch readers read: one plain request, host frame"""
    e.score_frames([s["frames"]["u16"][0]], [s["inputs"][0]])


def row_score(e, s, mk):
    d = mk()
    c = d.cloud(s["clouds"][0])
    with d:
        out = e.score(c, s["inputs"][0])
    return snapshot(e, [out], 1)


def row_score_batch(e, s, mk):
    d = mk()
    clouds = [d.cloud(c) for c in s["clouds"]]
    with d:
        outs = e.score_batch(clouds, [s["inputs"][0], s["inputs"][4]])
    return snapshot(e, outs, 2)


def row_score_frames(e, s, mk):
    d = mk()
    frames = [d.frame(*s["frames"][k]) for k in ("u16", "f32", "xyz")]
    with d:
        outs = e.score_frames(frames, [s["inputs"][0], s["inputs"][2], s["inputs"][4]])
    return snapshot(e, outs, 3)


def row_score_frames_roi(e, s, mk):
    d = mk()
    frames = [d.frame(*s["frames"]["u16"]), d.frame(*s["frames"]["xyz"])]
    masks = [d.rows(s["masks"][1]), d.rows(s["masks"][6])]
    with d:
        outs = e.score_frames_roi(frames, masks, [s["inputs"][0], s["inputs"][4]])
    return snapshot(e, outs, 2)


def row_score_views(e, s, mk):
    d = mk()
    views = [[d.frame(*s["frames"]["u16"]), d.frame(*s["frames"]["f32"])]]
    with d:
        outs, counts = e.score_views(views, [s["inputs"][0]])
    return dict(snapshot(e, outs, 1), counts=counts)


def row_score_views_roi(e, s, mk):
    d = mk()
    views = [[d.frame(*s["frames"]["f32"]), d.frame(*s["frames"]["xyz"])]]
    masks = [[d.rows(s["masks"][1]), d.rows(s["masks"][2])]]
    with d:
        outs, counts = e.score_views_roi(views, masks, [s["inputs"][1]])
    return dict(snapshot(e, outs, 1), counts=counts)


def row_score_objects(e, s, mk):
    d = mk()
    frame, labels = d.frame(*s["frames"]["f32"]), d.labels(s["labels"])
    with d:
        outs, picks, poses, order = e.score_objects(frame, labels, oc.N_LABELS, oc.OBJECT_LABELS, s["inputs"], min_vote=oc.MIN_VOTE)
    return dict(snapshot(e, outs, len(oc.OBJECT_LABELS)), picks=picks.tobytes(), poses=poses, order=order)


def row_grasp_map(e, s, mk):
    base_batch(e, s)
    d = mk()
    frame = d.frame(*s["frames"]["f32"])
    if d.host:
        m = e.grasp_map(0, frame)
        return tuple(m[k].tobytes() for k, _ in MAP_IMAGES)
    out = {k: d.output(PX * nb, 16) for k, nb in MAP_IMAGES}
    with d:
        e.grasp_map(0, frame, device_out=out)
    return tuple(d.read(i).tobytes() for i in range(3))


def row_best_in_mask(e, s, mk):
    base_batch(e, s)
    d = mk()
    frame = d.frame(*s["frames"]["xyz"])
    with d:
        return e.best_in_mask(0, frame, s["mask_any"], min_vote=1)


def row_best_per_label(e, s, mk):
    base_batch(e, s)
    d = mk()
    frame, labels = d.frame(*s["frames"]["u16"]), d.labels(s["labels16"])
    with d:
        got = e.best_per_label(0, frame, labels, n_labels=oc.N_LABELS, min_vote=1)
    return got["picks"].tobytes(), got["poses"], got["order"]


def row_top_grasps(e, s, mk):
    """haf_top_grasps behind a scoring call whose frame was late"""
    d = mk()
    frame = d.frame(*s["frames"]["xyz"])
    with d:
        e.score_frames([frame], [s["inputs"][4]])
    return e.top_grasps(k=8, min_vote=1)


SCORING_ROWS = [row_score, row_score_batch, row_score_frames, row_score_frames_roi, row_score_views, row_score_views_roi, row_score_objects,
                row_grasp_map, row_best_in_mask, row_best_per_label, row_top_grasps]


def filter_into(e, d, exposures, device_image):
    """haf_filter_depth into the caller's poisoned, padded device image or (device_image False) the engine's own -> (image, stats)"""
    stride = (W + 3) * 2
    if device_image:
        ptr = d.output((H - 1) * stride + W * 2, 18)      # one element past a 16-byte boundary
        with d:
            frame, stats = e.filter_depth(exposures, None, device_out=(ptr, stride))
        assert frame.on_device == 1 and frame.data == ptr
        return packed_rows(d.read(0), W * 2, stride, H).view(np.uint16), stats
    with d:
        frame, stats = e.filter_depth(exposures)
    assert frame.on_device == 1
    return fetch(frame.data, PX * 2).view(np.uint16).reshape(H, W), stats


def same_filter(s, got, where):
    image, stats = got
    assert image.tobytes() == s["filtered"].tobytes() and stats == s["filter_stats"], (where, stats, s["filter_stats"])


def row_filter_depth(e, s, mk):
    for device_image in (True, False):
        d = mk()
        same_filter(s, filter_into(e, d, [d.frame(f, img) for f, img in s["exposures"]], device_image), device_image)
    # once more into the engine's own image, which now has an address: poisoned late like a caller's
    d = mk()
    exposures = [d.frame(f, img) for f, img in s["exposures"]]
    d.alias(e.filter_depth([f for f, _ in s["exposures"][:1]])[0].data, PX * 2)
    same_filter(s, filter_into(e, d, exposures, False), "own image, poisoned")


def row_filter_depth_host_frames(e, s, mk):
    """host-resident exposures go up through the pinned staging area; the caller's device image is poisoned late"""
    same_filter(s, filter_into(e, mk(), [f for f, _ in s["exposures"]], True), "host exposures")


def labels_into(call, d, frame, device_image, own_ptr=None):
    """a label-writing call into the caller's poisoned, padded uint8 device image or the engine's own -> what the call returns, the
    labels as a host array"""
    stride = W + 5
    if device_image:
        ptr = d.output((H - 1) * stride + W, 3)
        with d:
            got = call(frame, (ptr, stride))
        assert got[0].data == ptr and got[0].on_device == 1 and got[0].row_stride_bytes == stride
        return (packed_rows(d.read(0), W, stride, H),) + tuple(got[1:])
    if own_ptr is not None:
        d.alias(own_ptr, PX)
    with d:
        got = call(frame, True)
    assert got[0].on_device == 1 and got[0].row_stride_bytes == W and own_ptr in (None, got[0].data)
    return (fetch(got[0].data, PX).reshape(H, W),) + tuple(got[1:])


def same_segments(got, want, where):
    assert got[0].tobytes() == np.ascontiguousarray(want[0]).tobytes(), where
    assert got[1].tobytes() == want[1].tobytes() and got[2] == want[2], where


def own_label_image(e, s):
    """the address of the engine's own label image (one image for both segmenters and the transfer)"""
    return e.segment(s["frames"]["u16"][0], capi.segment_params(**sc.SEGMENT_KW), device_out=True)[0].data


def row_segment(e, s, mk):
    p = capi.segment_params(**sc.SEGMENT_KW)
    call = lambda frame, out: e.segment(frame, p, device_out=out)
    for device_image in (True, False):
        d = mk()
        same_segments(labels_into(call, d, d.frame(*s["frames"]["u16"]), device_image), s["segment"], device_image)
    d = mk()
    same_segments(labels_into(call, d, d.frame(*s["frames"]["u16"]), False, own_label_image(e, s)), s["segment"], "own image, poisoned")


def row_segment_cells(e, s, mk):
    p = capi.cell_segment_params(**sc.CELL_KW)
    call = lambda frame, out: e.segment_cells(frame, p, device_out=out)
    for device_image in (True, False):
        d = mk()
        same_segments(labels_into(call, d, d.frame(*s["frames"]["u16"]), device_image), s["cells"], device_image)
    d = mk()
    same_segments(labels_into(call, d, d.frame(*s["frames"]["u16"]), False, own_label_image(e, s)), s["cells"], "own image, poisoned")


def row_fit_plane(e, s, mk):
    d = mk()
    frame, mask = d.frame(*s["frames"]["u16"]), d.rows(s["mask_any"])
    with d:
        got = e.fit_plane(frame, None, mask, debug=True)
    pc.same(got, s["plane"], "frame and mask late")


def row_measure_labels(e, s, mk):
    d = mk()
    frame, labels = d.frame(*s["frames"]["u16"]), d.labels(s["labels16"])
    with d:
        got = e.measure_labels(frame, labels, oc.N_LABELS, [0.0, 0.0, 1.0, 0.0])
    assert got.tobytes() == s["shapes"].tobytes()


def row_transfer_labels(e, s, mk):
    name, frame, image, cam, cam_labels, n_labels, kw = s["transfer"]
    want, p = s["transfer_want"], capi.transfer_params(**kw)
    n = frame.width * frame.height
    for device_image in (True, False):
        d = mk()
        dev, lab = d.frame(frame, image), d.labels(cam_labels)
        if device_image:
            ptr = d.output(n, 3)
            with d:
                img, stats = e.transfer_labels(dev, cam, lab, n_labels, p, device_out=(ptr, frame.width))
            got = d.read(0)
        else:
            with d:
                img, stats = e.transfer_labels(dev, cam, lab, n_labels, p, device_out=True)
            got = fetch(img.data, n)
        assert got.tobytes() == np.ascontiguousarray(want[0]).tobytes() and stats == want[1], (name, device_image, stats, want[1])


def row_check_grasps(e, s, mk):
    d = mk()
    frame, mask = d.frame(*s["frames"]["u16"]), d.rows(s["mask_any"])
    with d:
        got = e.check_grasps(frame, s["grasps"], None, mask)
    cc.same(got, s["clearance"], "frame and mask late")


HOST_DEFINITION_ROWS = [row_filter_depth, row_filter_depth_host_frames, row_segment, row_segment_cells, row_fit_plane, row_measure_labels,
                        row_transfer_labels, row_check_grasps]


# ---- the chain --------------------------------------------------------------------------------------------------------------------------

def chain(e, s, mk):
    """filter_depth (device image) -> fit_plane -> segment (device image) -> measure_labels -> score_objects -> top_grasps -> check_grasps,
    each stage fed from the one before; only the first call's exposures go through mk().  With Host: the chain of host definitions,
    scored on `e` from host memory."""
    d = mk()
    fp, host = capi.depth_filter(), d.host
    if host:
        image, fstats = capi.filter_depth_ref([f for f, _ in s["exposures"]], fp)
        f0 = s["exposures"][0][0]
        frame = capi.depth_frame(image, f0.fx, f0.fy, f0.cx, f0.cy, sensor_to_base=list(f0.sensor_to_base))
        fit = capi.fit_plane_ref(frame, None, None, debug=True)
        labels, infos, sstats = capi.segment_ref(frame, capi.segment_params(**dict(sc.SEGMENT_KW, plane=fit["plane"])))
        n = len(infos)
        shapes = capi.measure_labels_ref(frame, labels, n, fit["plane"])
    else:
        exposures = [d.frame(f, img) for f, img in s["exposures"]]
        with d:
            frame, fstats = e.filter_depth(exposures, fp)
        fit = e.fit_plane(frame, None, None, debug=True)
        labels, infos, sstats = e.segment(frame, capi.segment_params(**dict(sc.SEGMENT_KW, plane=fit["plane"])), device_out=True)
        n = len(infos)
        shapes = e.measure_labels(frame, labels, n, fit["plane"])
    assert n >= 2 and shapes["found"].all()
    base = capi.default_input(grasp_area_center=(0.0, 0.0, 0.0), grasp_area_length_x=oc.GRID, grasp_area_length_y=oc.GRID)
    inputs = [capi.object_input(e.cfg, base, shapes[l], 4)[0] for l in range(n)]
    outs, picks, poses, order = e.score_objects(frame, labels, n, list(range(1, n + 1)), inputs)
    top = e.top_grasps(k=8, min_vote=1)
    grasps = [g for per in top for g in per]
    assert len(grasps) >= 2
    clear = (e.check_grasps if not host else capi.check_grasps_ref)(frame, grasps)
    return dict(snapshot(e, outs, n), fstats=fstats, plane=fit["plane"].tobytes(), moments=fit["moments"], infos=infos.tobytes(), sstats=sstats,
                shapes=shapes.tobytes(), picks=picks.tobytes(), poses=poses, order=order, clear=clear[0].tobytes(), free=clear[1].tolist())


@pytest.fixture(scope="module")
def want(data_dir, surrogate):
    """the scoring family's expected values: every scoring row and the chain with host-resident inputs on an engine that never leaves its
    own stream; computed once, the engine closed before any other engine exists"""
    s = sc.scene()
    ref = make_engine(data_dir, surrogate, **sc.ENGINE_KW)
    out = {row.__name__: row(ref, s, Host) for row in SCORING_ROWS}
    out["chain"] = chain(ref, s, Host)
    ref.close()
    # the late inputs can change every one of them: an all-zero frame scores nothing
    assert out["row_score_frames"]["out"][0]["n_evals"] > 0 and out["row_top_grasps"][0] and out["row_best_in_mask"] is not None
    return out


def assert_same(got, expected, where):
    if isinstance(expected, dict):
        assert got.keys() == expected.keys(), where
        for k in expected:
            assert got[k] == expected[k], (where, k)
    else:
        assert got == expected, where


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

TABLE = [(mode, row) for mode in sc.MODES for row in SCORING_ROWS + HOST_DEFINITION_ROWS]


@pytest.mark.parametrize("mode,row", TABLE, ids=["%s-%s" % (m, r.__name__[4:]) for m, r in TABLE])
def test_call_on_a_callers_stream(data_dir, surrogate, tctx, want, mode, row):
    ctx = table_ctx(mode, data_dir, surrogate, tctx)
    got = row(ctx.e, sc.scene(), ctx.late)
    if row in SCORING_ROWS:
        assert_same(got, want[row.__name__], (mode, row.__name__))
    assert ctx.e.get_stream() == dict(torch=ctx.S.cuda_stream, null=0, own=ctx.own)[mode]


def test_control_a_wrong_stream_is_caught(data_dir, surrogate, tctx, monkeypatch):
    """the detector detects: an engine on its own stream, the frame produced late on a torch stream and NOT joined.  The calls run
    during the delay, read the zeros and return the all-zero frame's result, which is not the expected one.  (Without the guard check
    inside the calls, whatever the suite was started with: it begins with hipDeviceSynchronize, which waits for the delay on the
    OTHER stream too, and a call that waits for every stream cannot show that it was on the wrong one)"""
    monkeypatch.delenv("HAF_CANARY_CHECK", raising=False)
    release_table_engine()
    torch, S, cycles = tctx
    s = sc.scene()
    zero_segment, zero_clear = sc.zero_frame_results()
    e = make_engine(data_dir, surrogate, **sc.ENGINE_KW)
    try:
        for call, zero, expected, same in (
                (lambda f: e.segment(f, capi.segment_params(**sc.SEGMENT_KW)), zero_segment, s["segment"], same_segments),
                (lambda f: e.check_grasps(f, s["grasps"]), zero_clear, capi.check_grasps_ref(s["frames"]["u16"][0], s["grasps"]), cc.same)):
            call(s["frames"]["u16"][0])                     # (the call's first-use allocations, out of the way)
            d = sc.Late(torch, S, cycles, control=True)
            frame = d.frame(*s["frames"]["u16"])
            with d:
                got = call(frame)
                assert not d.late.query(), "the wrongly streamed call did not end inside the delay"
            same(got, zero, "the all-zero frame's result")
            with pytest.raises(AssertionError):
                same(got, expected, "the expected result")
        # and the poison: the same engine writes a caller's device image from a host frame during the delay; the late fill overwrites it
        d = sc.Late(torch, S, cycles, control=True)
        stride = W + 5
        ptr = d.output((H - 1) * stride + W, 3)
        with d:
            got = e.segment(s["frames"]["u16"][0], capi.segment_params(**sc.SEGMENT_KW), device_out=(ptr, stride))
            assert not d.late.query(), "the wrongly streamed call did not end inside the delay"
        same_segments((s["segment"][0],) + tuple(got[1:]), s["segment"], "what the call itself returned")
        assert (d.read(0) == sc.POISON).all()             # (__exit__ has synchronised the stream: the fill is done)
    finally:
        S.synchronize()                                   # before anything is freed
        e.close()


def test_the_chain_on_a_torch_stream(data_dir, surrogate, tctx, want):
    """the whole chain with the first exposures late and no synchronisation written by the test between the stages"""
    release_table_engine()
    e = make_engine(data_dir, surrogate, **sc.ENGINE_KW)
    try:
        ctx = Ctx(tctx, e, "torch")
        assert_same(chain(e, sc.scene(), ctx.late), want["chain"], "chain")
    finally:
        e.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------------------------

def last_batch_state(e, s):
    state = dict(top=e.top_grasps(k=8, min_vote=1), counts=e.last_counts(), exact=e.last_exact_tiers(), points=e.fetch_points(0, PX).tobytes())
    m = e.grasp_map(0, s["frames"]["u16"][0])
    state["map"] = tuple(m[k].tobytes() for k, _ in MAP_IMAGES)
    for r in range(e.cfg.n_rolls):
        state["grid", r] = tuple(a.tobytes() for a in e.roll_grid(0, r))
    return state


def test_switching_streams(data_dir, surrogate, tctx, want):
    """the last batch survives a switch; the first request after a switch in each direction, own -> torch -> null -> torch -> own, equals
    a fresh engine's in results and tier counters; get_stream reports what was set; handing over the current handle changes nothing;
    stage timings on a caller's stream are finite"""
    release_table_engine()
    torch, S, cycles = tctx
    s = sc.scene()
    e = make_engine(data_dir, surrogate, **sc.ENGINE_KW)
    try:
        own = e.get_stream()
        assert own != 0 and own != S.cuda_stream
        e.set_stream(e.get_stream())                      # a no-op on the own stream: the handle stays valid
        assert e.get_stream() == own
        expected = want["row_score_frames"]
        assert_same(row_score_frames(e, s, Host), expected, "own stream")      # (ends with the unsynchronised clear of the counters)
        base_batch(e, s)
        state = last_batch_state(e, s)
        for name, handle in (("torch", S.cuda_stream), ("null", 0), ("torch", S.cuda_stream), ("own", own)):
            e.set_stream(handle)
            assert e.get_stream() == handle, name
            e.set_stream(e.get_stream())
            assert e.get_stream() == handle, name
            # read the last batch without another request
            assert_same(last_batch_state(e, s), state, ("last batch after the switch to", name))
            # the first request on the new stream, inputs late where the test can enqueue on it
            got = row_score_frames(e, s, Ctx(tctx, e, name, own=own).late)
            assert_same(got, expected, ("first request after the switch to", name))
            if name != "own":
                ms = e.stage_ms()
                assert all(math.isfinite(v) and v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0, (name, ms)
            base_batch(e, s)
            assert_same(last_batch_state(e, s), state, ("the batch again on", name))
    finally:
        e.close()
    # the caller's stream is the caller's: it outlives the engine and still works
    with torch.cuda.stream(S):
        total = torch.ones(4096, device="cuda").sum()
    S.synchronize()
    assert total.item() == 4096


def test_two_engines_take_turns_on_one_stream(data_dir, surrogate, tctx, want):
    release_table_engine()
    s = sc.scene()
    a, b = (make_engine(data_dir, surrogate, **sc.ENGINE_KW) for _ in range(2))
    try:
        ca, cb = Ctx(tctx, a, "torch"), Ctx(tctx, b, "torch")
        for turn in range(2):
            assert_same(row_score_frames(a, s, ca.late), want["row_score_frames"], ("a", turn))
            assert_same(row_score_objects(b, s, cb.late), want["row_score_objects"], ("b", turn))
            row_segment(a, s, ca.late)
            assert_same(row_best_per_label(b, s, cb.late), want["row_best_per_label"], ("b", turn))
            row_check_grasps(b, s, cb.late)
            assert_same(row_top_grasps(a, s, ca.late), want["row_top_grasps"], ("a", turn))
    finally:
        a.close()
        b.close()
    torch, S, _ = tctx
    with torch.cuda.stream(S):
        total = torch.ones(4096, device="cuda").sum()
    S.synchronize()
    assert total.item() == 4096
