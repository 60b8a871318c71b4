"""haf_score_objects without a GPU (include/hafgrasp.h): the name is declared and exported by both libraries, and the synthetic scene of
object_cases.py is not vacuous -- each listed object's own request through the oracle gives at least two of them a pick and at least
one none, and the cell sets the fused call has to mark differ between neighbouring objects.  The GPU suite (test_objects_gpu.py)
compares the device against exactly these expectations."""
import os
import re

import numpy as np

import object_cases as oc
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = {"haf_score_objects"}


def test_objects_name_exported_by_both_libraries():
    with open(os.path.join(ROOT, "include", "hafgrasp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert NEW_NAMES <= set(re.findall(r"\b(haf_[a-z_0-9]+)\s*\(", text))
    assert "#define HAF_ABI_VERSION 2" in text                          # the call only adds a symbol
    for L in (capi.lib(), capi.testlib()):
        for name in NEW_NAMES:
            assert hasattr(L, name), name
        assert L.haf_abi_version() == 2
    assert hasattr(capi.Engine, "score_objects")


def test_the_label_image_holds_what_the_scene_promises():
    lab, z = oc.labels_u8(), oc.scene_z()
    assert lab.shape == (oc.H, oc.W) and set(np.unique(lab)) == {0, 1, 2, 3, 4, 5, 6, oc.ABOVE_VALUE}
    assert oc.ABOVE_VALUE > oc.N_LABELS and oc.UNLISTED_LABEL not in oc.OBJECT_LABELS and (lab == oc.UNLISTED_LABEL).any()
    nan3 = np.isnan(z[lab == 3])
    assert nan3.any() and not nan3.all()                                # label 3: partly NaN points
    assert oc.W * oc.H > 4 * 256 * 4                                    # more than one workgroup of four-pixel lanes


def test_the_synthetic_scene_is_not_vacuous():
    """the oracle on each listed object's own input, then haf_label_best_ref on its grids: a condition, not a measurement"""
    e = oc.expectations("u16")
    picks = e["picks"]
    found = [l for l, p in zip(oc.OBJECT_LABELS, picks) if p["found"] and p["vote"] >= oc.MIN_VOTE]
    none = [l for l, p in zip(oc.OBJECT_LABELS, picks) if not p["found"]]
    print("found", found, "votes", [int(p["vote"]) for p in picks], "none", none)
    assert len(found) >= 2 and len(none) >= 1
    assert oc.FAR_LABEL in none                                         # listed, outside its own request's grid
    for l, p in zip(oc.OBJECT_LABELS, picks):
        if p["found"]:
            assert e["labels"][p["v"], p["u"]] == l and p["n_pixels"] >= 1


def test_expected_cell_sets_per_request():
    """haf_roi_cells under `labels == l` and the object's own input: the far object marks nothing in its own grid, every other object
    marks cells in every roll, and the sets of the two adjacent boxes differ while sharing cells under some roll -- a kernel that
    marked `labels != 0`, or the neighbour's pixels, would not reproduce them"""
    e = oc.expectations("u16")
    cfg = oc.engine_cfg()
    by_label = dict(zip(oc.OBJECT_LABELS, e["cells"]))
    for l, c in by_label.items():
        assert c.shape == (oc.CFG_KW["n_rolls"], oc.GRID, oc.GRID)
        per_roll = c.reshape(len(c), -1).sum(axis=1)
        assert (per_roll == 0).all() if l == oc.FAR_LABEL else (per_roll > 0).all(), l
    assert (by_label[1] != by_label[2]).any()
    # the same two label masks under ONE input: the boxes' common edge falls into common cells
    inp1 = e["inputs"][oc.OBJECT_LABELS.index(1)]
    shared = 0
    for r in range(oc.CFG_KW["n_rolls"]):
        a = capi.roi_cells(cfg, inp1, r, e["frame"], (e["labels"] == 1).astype(np.uint8), want=("roi",))["roi"]
        b = capi.roi_cells(cfg, inp1, r, e["frame"], (e["labels"] == 2).astype(np.uint8), want=("roi",))["roi"]
        shared += int((a & b).sum())
    assert shared > 0
    # and `labels != 0` is a different set for every listed object that marks anything
    any_mask = ((e["labels"] >= 1) & (e["labels"] <= oc.N_LABELS)).astype(np.uint8)
    for l, inp in zip(oc.OBJECT_LABELS, e["inputs"]):
        if l in (1, 2):
            whole = capi.roi_cells(cfg, inp, 0, e["frame"], any_mask, want=("roi",))["roi"]
            assert (whole != by_label[l][0]).any(), l
