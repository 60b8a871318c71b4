"""Shared by tests/test_objects_cpu.py and tests/test_objects_gpu.py (haf_score_objects, include/hafgrasp.h): one small synthetic scene --
a 160 x 120 depth frame of a table with six boxes seen from straight above, its hand-built label image and one request per listed
object -- in which the ROI marking, the binning and the label pass all see more than one workgroup and more than one object, and the
expectations both suites share: every object's request alone through the oracle (the CPU picks) and through haf_roi_cells (the cell
sets).  The engine is the 56 x 56 one with C3_CFG.

The label image holds on purpose:
  labels 1 and 2   two boxes side by side: the pixels along their common edge fall into the same grid cells;
  label 3          a box a third of whose pixels are invalid (NaN points);
  label 4          a box that IS listed, with a request centred far away from it: outside its own request's grid, no qualifying pixel;
  label 5          a box that is present and NOT listed;
  value 9          above n_labels = 6: ignored like background;
  label 6          a listed box on its own, far enough from the others to be alone in its request's grid."""
import functools
import os

import numpy as np

import plane_cases as pc
from haf_grasping_amd import capi

W, H = 160, 120
N_LABELS = 6
GRID = 56
CFG_KW = dict(n_rolls=20, roll_step_deg=9)               # test_frames_gpu.C3_CFG
MIN_VOTE = 1
OBJECT_LABELS = [1, 2, 3, 4, 6]                          # label 5 is present and not listed
FAR_LABEL = 4
UNLISTED_LABEL = 5
ABOVE_VALUE = 9
# label -> (u0, u1, v0, v1, height over the table in metres); pixels are 7 mm apart on the table (plane_cases.FX at 0.7 m)
BOXES = {1: (30, 37, 24, 46, 0.08), 2: (37, 45, 24, 46, 0.05), 3: (92, 100, 30, 52, 0.07), 4: (138, 148, 92, 110, 0.06),
         5: (60, 68, 84, 104, 0.06), 6: (20, 28, 82, 104, 0.08)}
# the camera looks straight down from 0.7 m above the table's origin: depth z -> base height TABLE - z
POSE = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, pc.TABLE], np.float32)


def scene_z():
    """depth in metres per pixel, NaN where invalid"""
    rng = np.random.default_rng(20251019)
    z = np.full((H, W), pc.TABLE) + rng.uniform(-0.001, 0.001, (H, W))
    for label, (u0, u1, v0, v1, h) in BOXES.items():
        z[v0:v1, u0:u1] = pc.TABLE - h
    z.reshape(-1)[rng.random(W * H) < 0.02] = np.nan      # a sprinkle of invalid pixels everywhere
    u0, u1, v0, v1, _ = BOXES[3]
    z[v0:v1:3, u0:u1] = np.nan                            # every third row of label 3
    return z


def labels_u8():
    lab = np.zeros((H, W), np.uint8)
    for label, (u0, u1, v0, v1, _) in BOXES.items():
        lab[v0:v1, u0:u1] = label
    lab[2:5, 150:156] = ABOVE_VALUE                       # table pixels with a value above n_labels
    return lab


def frame_of(kind, pad=0):
    """-> (frame, image) of the scene as a u16 / f32 / xyz frame (plane_cases.depth_frame_of)"""
    return pc.depth_frame_of(scene_z(), kind, POSE, pad)


def engine_cfg():
    return capi.default_config(grid_h=GRID, grid_w=GRID, **CFG_KW)


def object_inputs(frame, labels):
    """one request per listed object: haf_object_input on the object's measured box -- but label FAR_LABEL's request is centred on the
    opposite corner of the table, so that the object lies outside its own request's grid"""
    cfg = engine_cfg()
    shapes = capi.measure_labels_ref(frame, labels, N_LABELS, [0.0, 0.0, 1.0, 0.0])
    base = capi.default_input(grasp_area_center=(0.0, 0.0, 0.0), grasp_area_length_x=GRID, grasp_area_length_y=GRID)
    out = []
    for l in OBJECT_LABELS:
        assert shapes["found"][l - 1]
        inp, _ = capi.object_input(cfg, base, shapes[l - 1], 4)
        if l == FAR_LABEL:
            inp.grasp_area_center[0], inp.grasp_area_center[1] = -0.25, 0.15
        out.append(inp)
    return out


def input_kw(inp):
    return dict(grasp_area_center=tuple(inp.grasp_area_center), grasp_area_length_x=inp.grasp_area_length_x,
                grasp_area_length_y=inp.grasp_area_length_y)


@functools.lru_cache(maxsize=None)
def expectations(kind="u16"):
    """computed once per frame kind and shared: per listed object b -- its request alone on the CPU
      picks[b]   haf_label_best_ref's entry of its label on the oracle's grids of ITS input, min_vote = MIN_VOTE;
      cells[b]   uint8 [R, GRID, GRID]: haf_roi_cells under the mask `labels == its label` and its input, roll by roll
    -> dict(frame, image, labels, inputs, picks, cells)"""
    from oracle import oracle as O
    from oracle_inputs import oracle_input
    import conftest
    frame, image = frame_of(kind)
    labels = labels_u8()
    inputs = object_inputs(frame, labels)
    cfg = engine_cfg()
    orc = O.Oracle(os.path.join(conftest.DATA, "Features.txt"), os.path.join(conftest.DATA, "range21062012_allfeatures"),
                   os.path.join(conftest.GOLDEN, "surrogate.model"))
    pts = capi.frame_points(frame)
    pts = pts[np.isfinite(pts).all(axis=1)]
    picks = np.zeros(len(OBJECT_LABELS), capi.LABEL_PICK_DTYPE)
    cells = []
    for b, (l, inp) in enumerate(zip(OBJECT_LABELS, inputs)):
        grids = orc.run(pts, O.make_cfg(H=GRID, W=GRID, **CFG_KW), oracle_input(input_kw(inp)))["graspseval"]
        picks[b] = capi.label_best_ref(cfg, inp, 0, grids, frame, labels, n_labels=N_LABELS, min_vote=MIN_VOTE)["picks"][l - 1]
        mask = (labels == l).astype(np.uint8)
        cells.append(np.stack([capi.roi_cells(cfg, inp, r, frame, mask, want=("roi",))["roi"] for r in range(CFG_KW["n_rolls"])]))
    return dict(frame=frame, image=image, labels=labels, inputs=inputs, picks=picks, cells=cells)
