"""CPU tests of haf_score_views_roi's host side (include/hafgrasp.h): haf_roi_cells_views -- the host definition of record of the ROI
cell sets of a fused request, the union over its masked views -- against haf_roi_cells per view and against the numpy mirror on the
oracle's transforms, its refusals, and the exports.  Every comparison is an equality.  The engine path needs a GPU:
tests/test_views_roi_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import frame_cases as fc
import pcdio
import roi_cases as rc
import views_roi_cases as vr
from haf_grasping_amd import capi
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, render_depth
from test_views_gpu import CAM_A, CAM_B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 56
NEW_NAMES = {"haf_roi_cells_views", "haf_score_views_roi"}


@pytest.fixture(scope="module")
def two_views(data_dir):
    """table1 from CAM_A and CAM_B: (frames, images, words of the pixels' points, masks): the C3 rectangle in A, the bounding-box rule in B"""
    xyz = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    imgs = [render_depth(xyz, CAM_A), render_depth(xyz, CAM_B)]
    frames = [capi.depth_frame(imgs[0], sensor_to_base=CAM_A, **K525), capi.depth_frame(imgs[1], sensor_to_base=CAM_B, **K525)]
    words = [fc.mirror_points(f, i) for f, i in zip(frames, imgs)]
    ma = vr.rect_mask(rc.C3_RECT, 480, 640)
    mb = vr.bbox_mask(words[0], ma, words[1], 480, 640)
    return frames, imgs, words, [ma, mb]


def test_views_definition_is_the_union_of_its_parts(two_views):
    """haf_roi_cells_views == the OR of haf_roi_cells over the masked views == roi_cases.mirror_roi on the ORACLE's roll transforms, roi
    and eval, for table1 from CAM_A + CAM_B at C3, all 20 rolls.  Mask A is roi_cases.C3_RECT, mask B the valid pixels of B whose
    base-frame (x, y) lies in the bounding box of A's masked points: 3 410 masked valid pixels in A and 2 821 in B; over the 20 rolls
    |S_A| = 3 800, |S_B| = 2 232, |S_A u S_B| = 4 410 -- B adds 610 cells, A adds 2 178, neither set contains the other, and no roll's
    set is empty.  With B's mask NULL the result is S_A, with every mask NULL it is empty."""
    frames, imgs, words, masks = two_views
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    valid = [np.isfinite(vr.points(w)).all(axis=1).reshape(480, 640) for w in words]
    assert [int((m != 0)[v].sum()) for m, v in zip(masks, valid)] == [3410, 2821]
    Ms = rc.oracle_transforms(C3_CFG, C3_IN, 0, 20)
    SA, SB = (rc.mirror_roi(Ms, words[k], masks[k], H, W) for k in range(2))
    U = vr.mirror_union(Ms, words, masks, H, W)
    assert (U == (SA | SB)).all()
    assert (int(SA.sum()), int(SB.sum()), int(U.sum())) == (3800, 2232, 4410)
    assert int((SB & ~SA).sum()) == 610 and int((SA & ~SB).sum()) == 2178
    assert all(U[r].any() for r in range(20))
    D = rc.dilate(U)
    for r in range(20):
        got = capi.roi_cells_views(cfg, inp, r, frames, masks)
        parts = [capi.roi_cells(cfg, inp, r, frames[k], masks[k], want=("roi",))["roi"] for k in range(2)]
        assert (got["roi"] == (parts[0] | parts[1])).all(), r
        assert (got["roi"] == U[r]).all() and (got["eval"] == D[r]).all(), r
        assert set(np.unique(got["roi"])) <= {0, 1} and set(np.unique(got["eval"])) <= {0, 1}
        only_a = capi.roi_cells_views(cfg, inp, r, frames, [masks[0], None])
        assert (only_a["roi"] == SA[r]).all() and (only_a["eval"] == rc.dilate(SA[r])).all(), r
        only_b = capi.roi_cells_views(cfg, inp, r, frames, [None, masks[1]], want=("roi",))
        assert list(only_b) == ["roi"] and (only_b["roi"] == SB[r]).all(), r
        none = capi.roi_cells_views(cfg, inp, r, frames, [None, None])
        assert not none["roi"].any() and not none["eval"].any()
    # a padded stride and values other than 1, the views in the other order: the same union
    wide = np.full((480, 645), 9, np.uint8)
    wide[:, :640] = masks[0] * 200
    got = capi.roi_cells_views(cfg, inp, 7, frames[::-1], [masks[1], wide[:, :640]])
    assert (got["roi"] == U[7]).all() and (got["eval"] == D[7]).all()


def test_roi_cells_views_refuses_what_it_must():
    """every refusal of haf_roi_cells, per view, plus the call's own; a refused call writes nothing"""
    L = capi.lib()
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input()          # (the search area around the origin: the frame's points fall into it)
    img = np.full((3, 4), 900, np.uint16)
    good = capi.depth_frame(img, fx=525.0, fy=525.0, cx=1.5, cy=1.0)      # (identity pose: the twelve points lie above the origin)
    mask = np.ones((3, 4), np.uint8)
    roi, ev = np.full((H, W), 7, np.uint8), np.full((H, W), 7, np.uint8)

    def R(m=mask.ctypes.data, stride=4, on_device=0):
        return capi.Roi(m, stride, on_device)

    def call(cfg_=cfg, inp_=inp, roll=0, frames=(good, good), rois=(R(), R()), n=None, null_frames=False, null_rois=False):
        fa = (capi.Frame * max(1, len(frames)))(*frames)
        ra = (capi.Roi * max(1, len(rois)))(*rois)
        return L.haf_roi_cells_views(C.byref(cfg_) if cfg_ else None, C.byref(inp_) if inp_ else None, roll, None if null_frames else fa,
                                     None if null_rois else ra, len(frames) if n is None else n, roi.ctypes.data, ev.ctypes.data)
    assert call() == capi.HAF_OK and set(np.unique(roi)) <= {0, 1} and roi.any() and set(np.unique(ev)) <= {0, 1}
    fa, ra = (capi.Frame * 2)(good, good), (capi.Roi * 2)(R(), R(m=None, stride=0, on_device=5))      # (a NULL mask's other fields are ignored)
    assert L.haf_roi_cells_views(C.byref(cfg), C.byref(inp), 0, fa, ra, 2, None, None) == capi.HAF_OK
    roi[:], ev[:] = 7, 7
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    for kw in (dict(cfg_=None), dict(inp_=None), dict(null_frames=True), dict(null_rois=True), dict(n=0), dict(n=-1), dict(frames=(good,) * 17, rois=(R(),) * 17),
               dict(roll=-1), dict(roll=cfg.n_rolls), dict(cfg_=capi.default_config(grid_h=0)), dict(cfg_=capi.default_config(grid_w=-3)),
               dict(cfg_=capi.default_config(n_rolls=0))):
        assert call(**kw) == A, kw
    for bad in (R(stride=3), R(stride=0), R(on_device=1), R(on_device=2)):
        assert call(rois=(bad, R())) == A and call(rois=(R(), bad)) == A      # (the second view is checked before the first is marked)
    assert call(frames=(dev, good)) == A and call(frames=(good, dev)) == A
    assert call(frames=(good, dev), rois=(R(), R(m=None))) == A             # (a view without a mask is still checked)
    seen = set()
    for name, frame, code, _ in fc.refusal_frames():
        assert call(frames=(good, frame)) == code and call(frames=(frame, good)) == code, name
        seen.add(code)
    assert seen == {A, CAP}
    assert (roi == 7).all() and (ev == 7).all()


def test_views_roi_names_exported_by_both_libraries():
    with open(os.path.join(ROOT, "include", "hafgrasp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert NEW_NAMES <= set(re.findall(r"\b(haf_[a-z_0-9]+)\s*\(", text))
    assert "#define HAF_ABI_VERSION 2" in text and re.search(r"HAF_DBG_ROI\s*=\s*9\b", text)
    assert capi.DBG_ROI == 9
    for L in (capi.lib(), capi.testlib()):
        for name in NEW_NAMES:
            assert hasattr(L, name), name
        assert L.haf_abi_version() == 2
    assert C.sizeof(capi.Roi) == 24                                          # (haf_roi itself is unchanged)
