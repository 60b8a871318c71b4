"""The one block and the one scratch that the calls outside the request path share (haf_engine::call_io, call_scratch; call_buffers and
call_finish of csrc/engine_stage.cpp) on the MI355X: every such call on ONE engine, in two cyclic orders, so that each finds the leftovers
of two different predecessors in the buffers it lays out for itself.  A call that read a region before writing it -- a table it
accumulates into, a key it takes a maximum into, a parent word -- would now read another call's bytes there and return something else.

Every result is compared word for word with the call's host definition of record (haf_segment_ref, haf_segment_cells_ref,
haf_fit_plane_ref, haf_check_grasps_ref, haf_measure_labels_ref, haf_transfer_labels_ref, haf_grasp_map_ref, haf_label_best_ref); the
calls without one (haf_top_grasps, haf_score_objects, haf_grasp_map_best, haf_cell_pose) with the same call as the first such call of a
fresh engine.  Each call runs with host-resident input and output and with device-resident input and output.  In the middle of the second
order a grasp map of a 640 x 480 host frame makes the block grow while it holds another call's leftovers: at max_points = 320 000 the
largest block of the other calls is haf_transfer_labels' 1.28 MB, that map's is 3.07 MB.  Testing build; the guard zones around every
device buffer are checked inside every call and after the test."""
import os

import numpy as np
import pytest

import cell_segment_cases as csc
import clearance_cases as cc
import object_cases as oc
import plane_cases as pc
import segment_cases as sc
import shape_cases as shc
import transfer_cases as tc
from haf_grasping_amd import capi
from test_cell_segment_gpu import cells_into
from test_frames_gpu import device_copy, make_engine
from test_grasp_map_gpu import device_images, engine_grids
from test_label_shape_gpu import device_labels
from test_plane_gpu import device_mask
from test_segment_gpu import segment_into
from test_transfer_gpu import device_labels as device_camera_labels, transfer_into

pytestmark = pytest.mark.gpu

R = 6
CFG = dict(n_rolls=R, roll_step_deg=30, grid_h=oc.GRID, grid_w=oc.GRID, max_points=320000, max_clouds=8)
VGA = (640, 480)


@pytest.fixture(autouse=True)
def _canaries(monkeypatch):
    monkeypatch.setenv("HAF_CANARY_CHECK", "1")
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


def by_name(cases, name):
    return next(c for c in cases if c[0] == name)


def vga_frame():
    """object_cases' scene in the middle of a 640 x 480 image of the same camera axis: the table all around it"""
    z = np.full((VGA[1], VGA[0]), pc.TABLE)
    z[180:180 + oc.H, 240:240 + oc.W] = oc.scene_z()
    return pc.depth_frame_of(z, "u16", oc.POSE)


def plain(x):
    """a result of candidate dicts, tuples and arrays as something `==` compares"""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


class Scene:
    """the inputs of every call, their device-resident copies and the expectations that need no engine, built once"""

    def __init__(self, cfg):
        self.frame, self.image = oc.frame_of("u16", 3)
        self.dev = device_copy(self.frame, self.image)
        self.labels = pc.padded_mask(oc.labels_u8(), 5)
        self.dlabels = device_labels(self.labels)
        self.mask = pc.padded_mask((self.labels != 0).astype(np.uint8), 7)
        shapes = capi.measure_labels_ref(self.frame, np.ascontiguousarray(self.labels), oc.N_LABELS, [0.0, 0.0, 1.0, 0.0])
        base = capi.default_input(grasp_area_center=(0.0, 0.0, 0.0), grasp_area_length_x=oc.GRID, grasp_area_length_y=oc.GRID)
        self.inputs = [capi.object_input(cfg, base, shapes[l - 1], 4)[0] for l in oc.OBJECT_LABELS]
        self.inp = self.inputs[0]
        self.big, _ = vga_frame()
        # the smallest cases of each call's own module that still span more than one workgroup or tile
        self.segment = sc.make_case("random", "f32", (65, 17), True)
        self.cells = csc.grid_case("random", 65, 17)[1:]
        self.planes = [by_name(pc.small_cases(), n) for n in ("boxes_masked_u16_67x33", "holes_f32_130x17")]
        self.clearance = by_name(cc.small_cases(), "boxes_masked_u16_pad3")
        self.shape = by_name(shc.small_cases(), "split_u16_130x33")
        self.transfer = by_name(tc.kind_cases(), "kind_f32_uint16")


def score_base(e, s):
    return e.score_frames([s.frame], [s.inp])[0]


def no_definition_calls(s):
    """name -> call(engine) for the calls whose expected value is the same call on a fresh engine"""
    return dict(top=lambda e: e.top_grasps(k=8, min_vote=1),
                best=lambda e: [e.best_in_mask(0, f, s.mask, min_vote=1) for f in (s.frame, s.dev)],
                pose=lambda e: [e.cell_pose(0, r, 30, 27) for r in (0, R - 1)],
                objects=lambda e: [e.score_objects(f, l, oc.N_LABELS, oc.OBJECT_LABELS, s.inputs, min_vote=oc.MIN_VOTE)
                                   for f, l in ((s.frame, s.labels), (s.dev, s.dlabels))])


@pytest.fixture(scope="module")
def scene():
    return Scene(capi.default_config(**CFG))


@pytest.fixture(scope="module")
def fresh(data_dir, golden_dir, scene):
    """each call without a host definition as the first call of its kind on an engine of its own, behind the one scored request"""
    out = {}
    for name, call in no_definition_calls(scene).items():
        e = make_engine(data_dir, os.path.join(golden_dir, "surrogate.model"), **CFG)
        out["vote"] = score_base(e, scene)["best_vote"]
        out[name] = plain(call(e))
        e.close()
    assert out["vote"] >= 1 and out["top"][0] and out["best"][0] is not None and len(out["objects"][0][3]) >= 1      # (not comparisons of nothing)
    return out


def calls(e, s, fresh):
    """-> [(name, call())]: every call that goes through call_buffers, each asserting its own result"""
    grids = engine_grids(e, 0, 0, R)

    def segment():
        frame, image, kw = s.segment
        p = capi.segment_params(**kw)
        want = capi.segment_ref(frame, p)
        assert len(want[1]) >= 2
        for f, mode in ((frame, "host"), (device_copy(frame, image), "device"), (frame, "engine")):
            assert sc.same(segment_into(e, f, p, np.uint8, mode, "segment"), want), mode

    def segment_cells():
        frame, image, kw = s.cells
        p = capi.cell_segment_params(**kw)
        want = capi.segment_cells_ref(frame, p, cell_labels=True)
        assert len(want[1]) >= 2
        for f, mode in ((frame, "host"), (device_copy(frame, image), "device")):
            assert csc.same(cells_into(e, f, p, np.uint8, mode, "cells"), want), mode

    def fit_plane():
        for name, frame, image, kw, mask in s.planes:
            p = capi.plane_params(**kw)
            want = capi.fit_plane_ref(frame, p, mask, debug=True)
            keep, dmask = device_mask(mask) if mask is not None else (None, None)
            pc.same(e.fit_plane(frame, p, mask, debug=True), want, name + ", host")
            pc.same(e.fit_plane(device_copy(frame, image), p, dmask, debug=True), want, name + ", device")

    def check_grasps():
        name, frame, image, kw, grasps, mask = s.clearance
        g = capi.gripper(**kw)
        want = capi.check_grasps_ref(frame, grasps, g, mask)
        keep, dmask = device_mask(mask)
        cc.same(e.check_grasps(frame, grasps, g, mask), want, "host")
        cc.same(e.check_grasps(device_copy(frame, image), grasps, g, dmask), want, "device")

    def measure_labels():
        name, frame, image, labels, n_labels, plane = s.shape
        want = capi.measure_labels_ref(frame, labels, n_labels, plane)
        assert want["found"].sum() >= 2
        assert e.measure_labels(frame, labels, n_labels, plane).tobytes() == want.tobytes()
        assert e.measure_labels(device_copy(frame, image), device_labels(labels), n_labels, plane).tobytes() == want.tobytes()

    def transfer_labels():
        name, frame, image, cam, labels, n_labels, kw = s.transfer
        p = capi.transfer_params(**kw)
        want = capi.transfer_labels_ref(frame, cam, labels, n_labels, p, np.uint16, zbuffer=True)
        assert want[0].any()
        for f, l, mode in ((frame, labels, "host"), (device_copy(frame, image), device_camera_labels(labels), "device")):
            assert tc.same(transfer_into(e, f, cam, l, n_labels, p, np.uint16, mode, name), want), mode

    def grasp_map_of(frame, dev=None):
        want = capi.grasp_map_ref(e.cfg, s.inp, 0, grids, frame)
        assert (want["cell"] >= 0).any()
        got = e.grasp_map(0, frame)
        for k in want:
            assert (got[k] == want[k]).all(), k
        if dev is not None:
            ptrs, read = device_images(frame.width * frame.height, 1)
            e.grasp_map(0, dev, device_out=ptrs)
            got = read((frame.height, frame.width))
            for k in want:
                assert (got[k] == want[k]).all(), (k, "device")

    def best_per_label():
        want = capi.label_best_ref(e.cfg, s.inp, 0, grids, s.frame, s.labels, n_labels=oc.N_LABELS, min_vote=1)
        assert len(want["order"]) >= 1
        for f, l in ((s.frame, s.labels), (s.dev, s.dlabels)):
            got = e.best_per_label(0, f, l, n_labels=oc.N_LABELS, min_vote=1)
            assert got["picks"].tobytes() == want["picks"].tobytes() and got["order"] == want["order"]

    def score_objects():
        assert plain(no_definition_calls(s)["objects"](e)) == fresh["objects"]
        assert score_base(e, s)["best_vote"] == fresh["vote"]            # the last batch is the one scored request again

    def against_fresh(name):
        def call():
            assert plain(no_definition_calls(s)[name](e)) == fresh[name], name
        return call

    return [("segment_frame", segment), ("segment_cells", segment_cells), ("fit_plane", fit_plane), ("check_grasps", check_grasps),
            ("measure_labels", measure_labels), ("transfer_labels", transfer_labels), ("grasp_map", lambda: grasp_map_of(s.frame, s.dev)),
            ("grasp_map_best", against_fresh("best")), ("grasp_map_labels", best_per_label), ("cell_pose", against_fresh("pose")),
            ("score_objects", score_objects), ("top_grasps", against_fresh("top"))], lambda: grasp_map_of(s.big)


def test_every_call_on_the_leftovers_of_two_different_predecessors(data_dir, golden_dir, scene, fresh):
    e = make_engine(data_dir, os.path.join(golden_dir, "surrogate.model"), **CFG)
    assert score_base(e, scene)["best_vote"] == fresh["vote"]
    table, large_map = calls(e, scene, fresh)
    n = len(table)
    orders = [list(range(n)), [(5 * i) % n for i in range(n)]]          # (5 and n = 12 have no common factor: a cycle through every call)
    ran = {i: set() for i in range(n)}
    for k, order in enumerate(orders):
        assert sorted(order) == list(range(n))
        cycle = order + order[:1]                                       # cyclic: the first call once more, behind the last
        for at, i in enumerate(cycle):
            if k == 1 and at == n // 2:
                large_map()                                             # the block grows here, full of call cycle[at - 1]'s bytes
            table[i][1]()
            if at:
                ran[i].add(cycle[at - 1])
    assert all(len(before) >= 2 for before in ran.values()), ran
    e.close()
