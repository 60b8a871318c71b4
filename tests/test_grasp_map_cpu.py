"""The host definitions of record of the per-pixel grasp maps (include/hafgrasp.h: haf_point_cells, haf_grasp_map_ref): no device, no
engine.  haf_point_cells against the CPU oracle's height grids, haf_grasp_map_ref against a numpy mirror built on the oracle's own roll
transforms and vote grids (grasp_map_cases.py), non-vacuity of both on the golden scene, and every refusal.  Every comparison is an
equality."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import pcdio
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import oracle_input
from test_frames_gpu import C3_CFG, C3_IN, DOWN, K525, TABLE1, pose, render_depth
from test_views_gpu import CAM_A, CAM_B

H = W = 56
TILTED_IN = dict(C3_IN, approach_vector=(0.1, -0.1, 1.0), gripper_opening_width=2)


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


@pytest.fixture(scope="module")
def orc(data_dir, golden_dir):
    return O.Oracle(os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures"),
                    os.path.join(golden_dir, "surrogate.model"))


def run_oracle(orc, xyz, in_kw):
    return orc.run(xyz, O.make_cfg(**C3_CFG), oracle_input(in_kw))


@pytest.fixture(scope="module")
def scene(orc, table1):
    """table1 at C3 (56 x 56, 20 rolls of 9 degrees) as the CPU oracle scores it"""
    return run_oracle(orc, table1, C3_IN)


@pytest.mark.parametrize("in_kw", [C3_IN, TILTED_IN], ids=["c3", "tilted_width2"])
def test_point_cells_reproduce_the_oracle_height_grids(orc, table1, scene, in_kw):
    """Every roll: the maximum of the transformed z over the points haf_point_cells puts into a cell, 0 for an empty cell, is the
    oracle's height grid word for word.  The cells come from the code under test (its own fill_roll_geo, its own cell arithmetic), z'
    from the oracle's M: a wrong transform, range test or index lands points in other cells and changes a maximum."""
    want = scene if in_kw is C3_IN else run_oracle(orc, table1, in_kw)
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**in_kw)
    pts = np.ascontiguousarray(table1[:, :3], np.float32)
    filled = 0
    for roll in range(cfg.n_rolls):
        cells = capi.point_cells(cfg, inp, roll, table1)
        mirror, pz = gm.mirror_cells(want["M"][roll], pts, H, W)
        assert (cells == mirror).all(), roll
        has = cells >= 0
        grid = np.full(H * W, -np.inf, np.float32)
        np.maximum.at(grid, cells[has], pz[has])
        empty = np.isinf(grid)
        grid[empty] = 0
        filled += int((~empty).sum())
        assert (grid.view(np.uint32) == want["heights"][roll].reshape(-1).view(np.uint32)).all(), roll
    print("%d cells filled over %d rolls" % (filled, cfg.n_rolls))
    assert filled >= cfg.n_rolls * 1000
    # a strided cloud (pcl::PointXYZ) gives the same cells
    wide = np.zeros((len(pts), 4), np.float32)
    wide[:, :3] = pts
    assert (capi.point_cells(cfg, inp, 7, wide) == capi.point_cells(cfg, inp, 7, pts)).all()


def scene_frames(table1):
    """-> list of (name, host frame, image): the golden scene in all three kinds, with padded rows, 16-byte points, a 1 x 1 frame and
    all-invalid frames"""
    da, db = render_depth(table1, CAM_A), render_depth(table1, CAM_B)
    metres = db.astype(np.float32) * np.float32(0.001)
    cam_pts = np.zeros((480, 640, 4), np.float32)                            # pcl::PointXYZ, sensor frame of camera B
    cam_pts[:, :, :3] = capi.frame_points(capi.depth_frame(db, **K525)).reshape(480, 640, 3)
    own = gm.organised(table1)
    one = np.array([[900]], np.uint16)                                       # straight down onto the centre of the search area
    out = [("table1_xyz", capi.xyz_frame(own), own),
           ("u16_cam_a", capi.depth_frame(da, sensor_to_base=CAM_A, **K525), da),
           ("u16_cam_a_padded", None, fc.padded(da, 5)),
           ("f32_cam_b_padded", None, fc.padded(metres, 3)),
           ("xyz16_cam_b", capi.xyz_frame(cam_pts, sensor_to_base=CAM_B), cam_pts),
           ("xyz_padded", None, fc.padded(own, 2)),
           ("u16_single_pixel", capi.depth_frame(one, 525.0, 525.0, 0.0, 0.0, sensor_to_base=pose(DOWN, (0.13, 0.25, 0.9))), one),
           ("u16_all_invalid", capi.depth_frame(np.zeros((48, 64), np.uint16), sensor_to_base=CAM_A, **K525), np.zeros((48, 64), np.uint16)),
           ("f32_all_invalid", capi.depth_frame(np.full((5, 61), np.nan, np.float32), **K525), np.full((5, 61), np.nan, np.float32)),
           ("xyz_all_invalid", capi.xyz_frame(np.full((3, 7, 3), np.inf, np.float32)), np.full((3, 7, 3), np.inf, np.float32))]
    made = []
    for name, frame, img in out:
        if frame is None:
            frame = capi.xyz_frame(img) if img.ndim == 3 else \
                capi.depth_frame(img, sensor_to_base=CAM_A if img.dtype == np.uint16 else CAM_B, **K525)
            assert frame.row_stride_bytes > frame.width * (12 if img.ndim == 3 else img.itemsize)
        made.append((name, frame, img))
    return made


def test_grasp_map_ref_equals_the_numpy_mirror(table1, scene):
    """haf_grasp_map_ref on the oracle's vote grids == the numpy mirror on the oracle's M and the same grids, every pixel of all three
    images: the golden scene in every kind (padded rows, 16-byte points, 1 x 1, all-invalid) and every frame of frame_cases.cases()
    (special values, limits, odd shapes).  Also a roll sub-range with its global indices, and outputs left out one by one."""
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    kinds, hit = 0, {}
    for name, frame, img in scene_frames(table1) + list(fc.cases()):
        words = fc.mirror_points(frame, img)
        assert (fc.words(capi.frame_points(frame)) == words).all(), name
        want = gm.mirror_map(scene["M"], scene["graspseval"], 0, words, H, W)
        got = capi.grasp_map_ref(cfg, inp, 0, scene["graspseval"], frame)
        gm.assert_map_equal(got, want, name)
        kinds |= 1 << frame.kind
        hit[name] = int((want[1] >= 0).sum())
        if name.endswith("all_invalid"):
            assert hit[name] == 0 and (got["vote"] == gm.NO_CELL).all() and (got["roll"] == -1).all() and (got["cell"] == -1).all()
    assert kinds == 7
    print({k: v for k, v in hit.items() if v})
    assert hit["u16_single_pixel"] == 1
    for name in ("table1_xyz", "u16_cam_a", "u16_cam_a_padded", "f32_cam_b_padded", "xyz16_cam_b", "xyz_padded"):
        assert hit[name] >= 10000, (name, hit[name])
    # rolls 5..11 only: global roll indices, the lowest roll of the range wins a tie
    _, frame, img = scene_frames(table1)[1]
    words = fc.mirror_points(frame, img)
    want = gm.mirror_map(scene["M"][5:12], scene["graspseval"][5:12], 5, words, H, W)
    got = capi.grasp_map_ref(cfg, inp, 5, scene["graspseval"][5:12], frame)
    gm.assert_map_equal(got, want, "rolls 5..11")
    assert set(np.unique(got["roll"])) <= set(range(5, 12)) | {-1} and (got["roll"] >= 5).sum() >= 10000
    for keep in ("vote", "roll", "cell"):
        part = capi.grasp_map_ref(cfg, inp, 5, scene["graspseval"][5:12], frame, want=(keep,))
        assert list(part) == [keep] and (part[keep] == got[keep]).all()
    # no roll ran: no cell anywhere
    none = capi.grasp_map_ref(cfg, inp, 0, np.zeros((0, H, W), np.float32), frame)
    assert (none["vote"] == gm.NO_CELL).all() and (none["roll"] == -1).all() and (none["cell"] == -1).all()


def map_figures(vote, roll):
    v = vote.astype(np.int64).reshape(-1)
    return dict(positive=int((v > 0).sum()), rolls=int(np.unique(roll[(vote > 0)]).size), top=int(v.max()), no_cell=int((roll < 0).sum()))


def test_maps_of_the_golden_scene_are_not_vacuous(table1, scene):
    """The conditions are on the ORACLE-derived expectation (numpy mirror on the oracle's M and vote grids), which the code under test
    must then equal.
    table1's own points as an XYZ frame: measured 27 747 of 102 876 finite points with a positive best vote, all 20 rolls among the
    winners, maximum 101 = the oracle's top vote.  Required: >= 10 000 positive pixels, >= 10 distinct winning rolls, maximum == top.
    table1 rendered as a 640 x 480 U16 frame from CAM_A: measured 10 776 pixels with a positive best vote, 20 winning rolls, maximum 101
    and 266 985 NO_CELL pixels (all of them zero-depth pixels, which exist by construction).  Required: at least half of each -- 5 388
    positive pixels, 10 rolls, a maximum of 51 -- and >= 1 000 NO_CELL pixels."""
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    own = gm.organised(table1)
    frame = capi.xyz_frame(own)
    want = gm.mirror_map(scene["M"], scene["graspseval"], 0, fc.mirror_points(frame, own), H, W)
    fig = map_figures(want[0], want[1])
    print("table1 as an XYZ frame:", fig, "finite points", int(np.isfinite(table1).all(axis=1).sum()), "oracle top", scene["top"])
    assert fig["positive"] >= 10000 and fig["rolls"] >= 10 and fig["top"] == scene["top"]
    gm.assert_map_equal(capi.grasp_map_ref(cfg, inp, 0, scene["graspseval"], frame), want, "table1_xyz")
    depth = render_depth(table1, CAM_A)
    frame = capi.depth_frame(depth, sensor_to_base=CAM_A, **K525)
    want = gm.mirror_map(scene["M"], scene["graspseval"], 0, fc.mirror_points(frame, depth), H, W)
    fig = map_figures(want[0], want[1])
    print("table1 rendered from CAM_A:", fig, "zero-depth pixels", int((depth == 0).sum()))
    assert fig["positive"] >= 5388 and fig["rolls"] >= 10 and fig["top"] >= 51 and fig["no_cell"] >= 1000
    gm.assert_map_equal(capi.grasp_map_ref(cfg, inp, 0, scene["graspseval"], frame), want, "u16_cam_a")


def test_host_functions_refuse_what_they_must():
    """Every HAF_E_ARG / HAF_E_CAPACITY case of haf_point_cells and haf_grasp_map_ref; nothing is written by a refused call"""
    L = capi.lib()
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    pts = np.zeros((4, 3), np.float32)
    cells = np.full(4, 77, np.int32)
    pc = lambda cfg_=cfg, inp_=inp, roll=0, xyz=pts.ctypes.data, n=4, stride=3, out=cells.ctypes.data: \
        L.haf_point_cells(C.byref(cfg_) if cfg_ else None, C.byref(inp_) if inp_ else None, roll, xyz, n, stride, out)
    assert pc() == capi.HAF_OK and (cells != 77).all()
    cells[:] = 77
    assert pc(n=0, xyz=None) == capi.HAF_OK
    for kw in (dict(cfg_=None), dict(inp_=None), dict(out=None), dict(xyz=None), dict(roll=-1), dict(roll=cfg.n_rolls), dict(stride=2), dict(stride=0),
               dict(cfg_=capi.default_config(grid_h=0)), dict(cfg_=capi.default_config(grid_w=-3)), dict(cfg_=capi.default_config(n_rolls=0))):
        assert pc(**kw) == A, kw
    assert pc(n=(1 << 31)) == CAP
    assert (cells == 77).all()

    grids = np.zeros((cfg.n_rolls, H, W), np.float32)
    img = np.full((3, 4), 900, np.uint16)
    good = capi.depth_frame(img, **K525)
    vote, roll, cell = np.full((3, 4), 7, np.int16), np.full((3, 4), 7, np.int16), np.full((3, 4), 7, np.int32)

    def ref(cfg_=cfg, inp_=inp, first=0, count=cfg.n_rolls, g=grids.ctypes.data, frame=good):
        return L.haf_grasp_map_ref(C.byref(cfg_) if cfg_ else None, C.byref(inp_) if inp_ else None, first, count, g,
                                   C.byref(frame) if frame else None, vote.ctypes.data, roll.ctypes.data, cell.ctypes.data)
    assert ref() == capi.HAF_OK and (vote != 7).all()
    assert L.haf_grasp_map_ref(C.byref(cfg), C.byref(inp), 0, cfg.n_rolls, grids.ctypes.data, C.byref(good), None, None, None) == capi.HAF_OK
    assert ref(count=0, g=None) == capi.HAF_OK and (vote == gm.NO_CELL).all()
    for a in (vote, roll, cell):
        a[:] = 7
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    for kw in (dict(cfg_=None), dict(inp_=None), dict(frame=None), dict(g=None), dict(first=-1), dict(count=-1), dict(first=1), dict(first=cfg.n_rolls, count=1),
               dict(count=cfg.n_rolls + 1), dict(cfg_=capi.default_config(grid_h=0)), dict(cfg_=capi.default_config(n_rolls=0), count=0), dict(frame=dev)):
        assert ref(**kw) == A, kw
    seen = set()
    for name, frame, code, _ in fc.refusal_frames():
        assert ref(frame=frame) == code, name
        seen.add(code)
    assert seen == {A, CAP}
    assert (vote == 7).all() and (roll == 7).all() and (cell == 7).all()
