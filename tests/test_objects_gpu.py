"""haf_score_objects on the MI355X (include/hafgrasp.h; csrc/engine_objects.cpp, csrc/roi.hip: k_roi_mark_objects, csrc/graspmap.hip:
k_map_labels_objects / k_object_records).  The definition of record is a composition of calls that exist -- request b is
haf_score_frames_roi under the mask `labels == object_labels[b]`, its pick the entry of that label of haf_grasp_map_labels after it -- and
every test here compares the fused call against that composition, the CPU expectations of object_cases.py or the state a reference call
leaves, by equality.  The one field left out of the comparison of outputs is n_rechecked, which every batched call counts per batch (the
header says so): it is checked against the batch's own counter instead.  Testing build, the guard zones checked inside every call and
after every test.  The engines hold exactly one frame (max_points = width x height): the frame counts once, whatever n_objects is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import object_cases as oc
import shape_cases as sc
from haf_grasping_amd import capi
from test_frames_gpu import _files, device_copy, make_engine
from test_label_shape_gpu import FAR_GOAL, OUTSIDE_LABEL, SEGMENT_OVER_FIT, device_labels
from test_plane_cpu import table1_frame
from test_views_gpu import CAM_A

pytestmark = pytest.mark.gpu

PX = oc.W * oc.H
R = oc.CFG_KW["n_rolls"]


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
    e = make_engine(data_dir, surrogate, max_points=PX, max_clouds=8, grid_h=oc.GRID, grid_w=oc.GRID, **oc.CFG_KW)
    yield e
    e.close()


def pick_key(p):
    return (-int(p["vote"]), int(p["roll"]), int(p["v"]) * oc.W + int(p["u"]))


def negative(inp):
    return int(inp.max_calculation_time) < 0


def request_state(e, b, frame):
    """what the getters say about request b of the last batch"""
    s = dict(top=e.top_grasps(k=8)[b], points=e.debug_points(b, PX).tobytes())
    m = e.grasp_map(b, frame)
    s["map"] = tuple(m[k].tobytes() for k in ("vote", "roll", "cell"))
    for r in range(R):
        ev, mask = e.roll_grid(b, r)
        s["grid", r] = (ev.tobytes(), mask.tobytes(), e.debug(capi.DBG_ROI, b, r).tobytes(), e.debug(capi.DBG_HEIGHTS, b, r).tobytes())
    return s


def compose(e, frame, labels, object_labels, inputs, min_vote=oc.MIN_VOTE, with_state=False):
    """the definition of record, call by call -> dict(outs, picks, poses, order, n_evals, states)"""
    host = np.asarray(labels)
    outs, poses, states = [], [], []
    picks = np.zeros(len(object_labels), capi.LABEL_PICK_DTYPE)
    n_evals = 0
    for b, (l, inp) in enumerate(zip(object_labels, inputs)):
        outs.append(e.score_frames_roi([frame], [(host == l).astype(np.uint8)], [inp])[0])
        if negative(inp):                                 # no roll ran: nothing scored, nothing found
            picks[b] = (0, -1, -1, capi.MAP_NO_CELL, -1, -1, 0)
            poses.append(None)
            states.append(None)
            continue
        n_evals += e.last_counts()["n_evals"]
        res = e.best_per_label(0, frame, host, n_labels=oc.N_LABELS, min_vote=min_vote)
        picks[b] = res["picks"][l - 1]
        poses.append(res["poses"][l - 1])
        states.append(request_state(e, 0, frame) if with_state else None)
    order = sorted((b for b in range(len(object_labels)) if picks["found"][b]), key=lambda b: pick_key(picks[b]))
    return dict(outs=outs, picks=picks, poses=poses, order=order, n_evals=n_evals, states=states)


def without_rechecked(out):
    return {k: v for k, v in out.items() if k != "n_rechecked"}


def assert_equals_composition(e, got, want, where):
    outs, picks, poses, order = got
    assert [without_rechecked(o) for o in outs] == [without_rechecked(o) for o in want["outs"]], where
    assert picks.tobytes() == want["picks"].tobytes(), (where, picks, want["picks"])
    assert poses == want["poses"], where
    assert order == want["order"], where                  # (n_found is its length)
    if any(p is not None for p in want["poses"]) or any(o["rolls_done"] for o in want["outs"]):
        counts = e.last_counts()
        assert counts["n_evals"] == want["n_evals"], where
        # rechecks are counted per batch and attributed to the first request
        assert [o["n_rechecked"] for o in outs[1:]] == [0] * (len(outs) - 1), where


@pytest.fixture(scope="module")
def reference(eng):
    """the composition on the u16 frame, host frame and host labels, with every request's state: computed once, shared, unchanged"""
    x = oc.expectations("u16")
    return compose(eng, x["frame"], x["labels"], oc.OBJECT_LABELS, x["inputs"], with_state=True)


def label_variants(labels):
    """(name, what score_objects takes): uint8 and uint16, rows padded, on the host and on the device"""
    u8, u16 = sc.padded_labels(labels, 5), sc.padded_labels(labels.astype(np.uint16), 3)      # (the padding holds label 1)
    return [("host u8", u8), ("host u16", u16), ("device u8", device_labels(u8)), ("device u16", device_labels(u16))]


@pytest.mark.parametrize("kind", ["u16", "f32", "xyz"])
def test_fused_equals_the_composition(eng, reference, kind):
    """every field of out, picks, poses, order and n_found; host and device frames crossed with the four label images"""
    x = oc.expectations("u16")
    labels, inputs = x["labels"], x["inputs"]
    frame, image = (x["frame"], x["image"]) if kind == "u16" else oc.frame_of(kind, pad=3)
    want = reference if kind == "u16" else compose(eng, frame, labels, oc.OBJECT_LABELS, inputs)
    assert want["picks"]["found"].sum() >= 2 and not want["picks"]["found"].all()
    dev = device_copy(frame, image)
    variants = label_variants(labels)
    for fr, where in ((frame, "host frame"), (dev, "device frame")):
        for name, lab in (variants if kind == "u16" else variants[1:3] if fr is frame else variants[::3]):
            got = eng.score_objects(fr, lab, oc.N_LABELS, oc.OBJECT_LABELS, inputs, min_vote=oc.MIN_VOTE)
            assert_equals_composition(eng, got, want, (kind, where, name))
    if kind == "u16":
        # the picks are the CPU's: each object's own request through the oracle, haf_label_best_ref on its grids
        assert want["picks"].tobytes() == x["picks"].tobytes()
        # and another min_vote moves both the same way
        top = int(want["picks"]["vote"].max())
        want_top = compose(eng, frame, labels, oc.OBJECT_LABELS, inputs, min_vote=top)
        assert 1 <= want_top["picks"]["found"].sum() < want["picks"]["found"].sum()
        assert_equals_composition(eng, eng.score_objects(frame, labels, oc.N_LABELS, oc.OBJECT_LABELS, inputs, min_vote=top), want_top, "min_vote")


def test_roi_sets_are_the_cpu_cell_sets(eng):
    """haf_debug_fetch(HAF_DBG_ROI) of every request and roll == haf_roi_cells under `labels == l` and the object's input: a pixel of
    the neighbouring box, of the unlisted label or of a value above n_labels marks nothing"""
    x = oc.expectations("u16")
    eng.score_objects(x["frame"], device_labels(sc.padded_labels(x["labels"], 5)), oc.N_LABELS, oc.OBJECT_LABELS, x["inputs"])
    for b in range(len(oc.OBJECT_LABELS)):
        for r in range(R):
            assert (eng.debug(capi.DBG_ROI, b, r) == x["cells"][b][r]).all(), (b, r)


def test_state_afterwards_is_the_batch_of_roi_requests(eng, reference):
    """haf_top_grasps, haf_grasp_map, haf_get_roll_grid, HAF_DBG_ROI, the height grids and the points of every request b equal what they
    return after the reference call for that object; haf_last_counts is the batch's; haf_debug_fetch_points returns the frame's points"""
    x = oc.expectations("u16")
    eng.score_objects(x["frame"], x["labels"], oc.N_LABELS, oc.OBJECT_LABELS, x["inputs"])
    assert eng.last_counts()["n_evals"] == reference["n_evals"]
    pts = capi.frame_points(x["frame"]).astype(np.float32).tobytes()
    for b in range(len(oc.OBJECT_LABELS)):
        got, want = request_state(eng, b, x["frame"]), reference["states"][b]
        assert got.keys() == want.keys()
        for k in want:
            assert got[k] == want[k], (b, k)
        assert got["points"] == pts, b
    # (this engine holds one frame: haf_score_frames_roi cannot take these requests as one batch)
    masks = [(x["labels"] == l).astype(np.uint8) for l in oc.OBJECT_LABELS[:2]]
    with pytest.raises(capi.HafError):
        eng.score_frames_roi([x["frame"]] * 2, masks, x["inputs"][:2])


def test_shapes_of_the_call(data_dir, surrogate, eng, reference):
    x = oc.expectations("u16")
    frame, labels, inputs = x["frame"], x["labels"], x["inputs"]

    def subset(idx, ins=None):
        ins = ins if ins is not None else [inputs[i] for i in idx]
        picks = reference["picks"][idx].copy()
        poses = [reference["poses"][i] for i in idx]
        outs = [reference["outs"][i] for i in idx]
        order = sorted((b for b in range(len(idx)) if picks["found"][b]), key=lambda b: pick_key(picks[b]))
        return [oc.OBJECT_LABELS[i] for i in idx], ins, dict(outs=outs, picks=picks, poses=poses, order=order, n_evals=None)

    def check(idx, where):
        ol, ins, want = subset(idx)
        outs, picks, poses, order = eng.score_objects(frame, labels, oc.N_LABELS, ol, ins)
        assert [without_rechecked(o) for o in outs] == [without_rechecked(o) for o in want["outs"]], where
        assert picks.tobytes() == want["picks"].tobytes() and poses == want["poses"] and order == want["order"], where

    check([0], "one object")
    check([3], "one object, none found")
    check([4, 3, 2, 1, 0], "object_labels in descending order")
    check([1, 4], "fewer")
    check([0, 1, 2, 3, 4], "more again: the buffers are reused")
    # n_objects == max_clouds
    e5 = make_engine(data_dir, surrogate, max_points=PX, max_clouds=5, grid_h=oc.GRID, grid_w=oc.GRID, **oc.CFG_KW)
    got = e5.score_objects(frame, labels, oc.N_LABELS, oc.OBJECT_LABELS, inputs)
    assert_equals_composition(e5, got, reference, "n_objects == max_clouds")
    e5.close()
    # one request with a negative budget among normal ones
    ins = [capi.GraspInput.from_buffer_copy(i) for i in inputs]
    ins[1].max_calculation_time = -1
    want = compose(eng, frame, labels, oc.OBJECT_LABELS, ins)
    assert not want["picks"]["found"][1] and want["picks"]["found"][0]
    got = eng.score_objects(frame, labels, oc.N_LABELS, oc.OBJECT_LABELS, ins)
    # (the batch still bins and evaluates that request, as every batch with one such request does: n_evals is the batch's)
    assert_equals_composition(eng, got, dict(want, n_evals=eng.last_counts()["n_evals"]), "a negative budget")
    for b in (0, 2, 4):                                   # the others are untouched by it
        assert got[1][b].tobytes() == reference["picks"][b].tobytes() and got[2][b] == reference["poses"][b]
    # every budget negative: nothing runs, nothing is found
    for i in ins:
        i.max_calculation_time = -1
    outs, picks, poses, order = eng.score_objects(frame, labels, oc.N_LABELS, oc.OBJECT_LABELS, ins)
    assert not picks["found"].any() and order == [] and poses == [None] * len(ins)
    assert [without_rechecked(o) for o in outs] == [without_rechecked(o) for o in compose(eng, frame, labels, oc.OBJECT_LABELS, ins)["outs"]]


def test_interleaving_with_plain_requests(data_dir, surrogate, reference):
    """an objects call between two haf_score_frames calls leaves their results and the engine's screening form unchanged"""
    x = oc.expectations("u16")
    e = make_engine(data_dir, surrogate, max_points=PX, max_clouds=8, grid_h=oc.GRID, grid_w=oc.GRID, **oc.CFG_KW)
    inp = capi.default_input(grasp_area_center=(-0.27, 0.16, 0.0), grasp_area_length_x=oc.GRID, grasp_area_length_y=oc.GRID)

    def plain():
        out = e.score_frames([x["frame"]], [inp])[0]
        grids = [tuple(a.tobytes() for a in e.roll_grid(0, r)) for r in range(R)]
        return out, grids, e.top_grasps(k=8), e.last_counts(), e.prestage_forms() if hasattr(e, "prestage_forms") else None

    form, before = e.screen_form(), plain()
    got = e.score_objects(x["frame"], x["labels"], oc.N_LABELS, oc.OBJECT_LABELS, x["inputs"])
    assert_equals_composition(e, got, reference, "between two plain calls")
    assert e.screen_form() == form
    after = plain()
    assert before == after and e.screen_form() == form
    e.close()


def raw_call(e, frame, img, n_labels, object_labels, inputs, picks, with_out=True):
    n = len(object_labels) if object_labels is not None else 0
    ol = (C.c_int32 * max(1, n))(*(object_labels or [])) if object_labels is not None else None
    gi = (capi.GraspInput * max(1, len(inputs)))(*inputs) if inputs is not None else None
    out = (capi.GraspOutput * max(1, n))()
    return e._L.haf_score_objects(e._h, C.byref(frame) if frame is not None else None, C.byref(img) if img is not None else None, n_labels, n, ol,
                                  gi, 1, out if with_out else None, picks.ctypes.data if picks is not None else None, None, None, None)


def test_refusals_leave_the_engine_as_it_was(data_dir, surrogate, golden_dir, tmp_path):
    """every refusal returns its code and a text that names the call, writes nothing, and leaves the previous batch readable"""
    import json
    import models
    x = oc.expectations("u16")
    frame, labels, inputs = x["frame"], np.ascontiguousarray(x["labels"]), x["inputs"]
    e = make_engine(data_dir, surrogate, max_points=PX, max_clouds=4, grid_h=oc.GRID, grid_w=oc.GRID, **oc.CFG_KW)
    ol, ins = oc.OBJECT_LABELS[:3], inputs[:3]
    first = e.score_objects(frame, labels, oc.N_LABELS, ol, ins)
    before = [request_state(e, b, frame) for b in range(3)]
    img, _ = capi.label_image(labels, frame, oc.N_LABELS)
    bad_frame = capi.Frame.from_buffer_copy(frame)
    bad_frame.width = 0
    bad_dev = capi.Frame.from_buffer_copy(frame)
    bad_dev.on_device = 7
    big_z = np.full((oc.H, oc.W + 1), 0.7)
    big, _ = oc.pc.depth_frame_of(big_z, "u16", oc.POSE)
    big_img, _ = capi.label_image(np.ones((oc.H, oc.W + 1), np.uint8), big, 1)
    img3 = capi.LabelImage(img.data, 3, 0, img.row_stride_bytes)
    img_dev = capi.LabelImage(img.data, 1, 5, img.row_stride_bytes)
    img_narrow = capi.LabelImage(img.data, 1, 0, oc.W - 1)
    img_null = capi.LabelImage(None, 1, 0, oc.W)
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    cases = [("null frame", None, img, oc.N_LABELS, ol, ins, True, True, A),
             ("a frame haf_score_frames refuses", bad_frame, img, oc.N_LABELS, ol, ins, True, True, A),
             ("frame on_device", bad_dev, img, oc.N_LABELS, ol, ins, True, True, A),
             ("more pixels than max_points", big, big_img, 1, [1], ins[:1], True, True, CAP),
             ("null labels", frame, None, oc.N_LABELS, ol, ins, True, True, A),
             ("null label data", frame, img_null, oc.N_LABELS, ol, ins, True, True, A),
             ("elem_bytes", frame, img3, oc.N_LABELS, ol, ins, True, True, A),
             ("label on_device", frame, img_dev, oc.N_LABELS, ol, ins, True, True, A),
             ("label stride", frame, img_narrow, oc.N_LABELS, ol, ins, True, True, A),
             ("n_labels 0", frame, img, 0, ol, ins, True, True, A),
             ("n_labels above HAF_MAX_LABELS", frame, img, capi.MAX_LABELS + 1, ol, ins, True, True, A),
             ("null picks", frame, img, oc.N_LABELS, ol, ins, False, True, A),
             ("null out", frame, img, oc.N_LABELS, ol, ins, True, False, A),
             ("null inputs", frame, img, oc.N_LABELS, ol, None, True, True, A),
             ("null object_labels", frame, img, oc.N_LABELS, None, ins, True, True, A),
             ("n_objects 0", frame, img, oc.N_LABELS, [], ins, True, True, A),
             ("n_objects > max_clouds", frame, img, oc.N_LABELS, oc.OBJECT_LABELS, inputs, True, True, CAP),
             ("label 0", frame, img, oc.N_LABELS, [1, 0, 2], ins, True, True, A),
             ("label above n_labels", frame, img, oc.N_LABELS, [1, oc.N_LABELS + 1, 2], ins, True, True, A),
             ("a label listed twice", frame, img, oc.N_LABELS, [1, 2, 1], ins, True, True, A)]
    untouched = np.frombuffer(bytes([0x5A]) * (8 * capi.LABEL_PICK_DTYPE.itemsize), capi.LABEL_PICK_DTYPE).copy()
    for name, fr, im, nl, lab, inp, with_picks, with_out, code in cases:
        picks = untouched.copy()
        rc = raw_call(e, fr, im, nl, lab, inp, picks if with_picks else None, with_out)
        text = (e._L.haf_last_error(e._h) or b"").decode()
        assert rc == code and text.startswith("haf_score_objects: "), (name, rc, code, text)
        assert picks.tobytes() == untouched.tobytes(), name
        after = [request_state(e, b, frame) for b in range(3)] if name in ("null frame", "a label listed twice", "more pixels than max_points") else None
        assert after is None or after == before, name
    assert e._L.haf_score_objects(None, C.byref(frame), C.byref(img), oc.N_LABELS, 1, (C.c_int32 * 1)(1), (capi.GraspInput * 1)(ins[0]), 1,
                                  (capi.GraspOutput * 1)(), untouched.copy().ctypes.data, None, None, None) == A
    again = e.score_objects(frame, labels, oc.N_LABELS, ol, ins)
    assert again[1].tobytes() == first[1].tobytes() and again[2] == first[2] and again[3] == first[3]
    assert [without_rechecked(o) for o in again[0]] == [without_rechecked(o) for o in first[0]]
    e.close()
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    e = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=PX, max_clouds=4, grid_h=oc.GRID, grid_w=oc.GRID, **oc.CFG_KW)
    picks = untouched.copy()
    assert raw_call(e, frame, img, oc.N_LABELS, ol, ins, picks) == A and b"HAF_FLAG_PROBABILITY" in e._L.haf_last_error(e._h)
    assert picks.tobytes() == untouched.tobytes()
    e.close()


def test_server_flow_on_table1_fused_equals_unfused(data_dir, surrogate, tmp_path):
    """CalcGraspPointsServer.execute_frame_per_object(fused=True) == the existing route, more than one chunk of max_clouds; a server that
    holds exactly one frame runs the fused route where the existing one degenerates to a request per chunk; the command line"""
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    fa, da = table1_frame(data_dir)
    f_, r_ = _files(data_dir)
    sp = capi.segment_params(plane=capi.fit_plane_ref(fa)["plane"], **SEGMENT_OVER_FIT)
    goal = GraspInputMsg(**FAR_GOAL)
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 22, max_clouds=4, **oc.CFG_KW)
    unfused = srv.execute_frame_per_object(goal, fa, sp)
    fused = srv.execute_frame_per_object(goal, fa, sp, fused=True)
    assert fused == unfused and len(fused) > 4 and OUTSIDE_LABEL in [o[0] for o in fused]
    srv.close()
    one = CalcGraspPointsServer(f_, r_, surrogate, max_points=640 * 480, max_clouds=4, **oc.CFG_KW)
    assert one.execute_frame_per_object(goal, fa, sp, fused=True) == unfused
    one.close()
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    pa = str(tmp_path / "a.pgm")
    fc.write_pgm16(pa, da)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.06", "0.45", "0",
              "--search-size", "42", "42", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", pa, "--sensor-pose"] + ["%.9g" % v for v in CAM_A]
    common += ["--segment", "0.03,0,0.02,50", "--plane", "fit", "--per-object", "4"]
    a = subprocess.run(common, check=True, capture_output=True, text=True).stdout
    b = subprocess.run(common + ["--fused"], check=True, capture_output=True, text=True).stdout
    assert a == b and len([ln for ln in a.splitlines() if ln.startswith("object ")]) == len(unfused)
