"""haf_fit_openings_ref (include/hafgrasp.h; csrc/opening_host.cpp), the host definition of record of the smallest free opening, against
the independent mirror of opening_cases in EVERY field of every row, in order, info and every histogram word -- the mirror counts every
placement directly from the points without prefilter, histogram or prefix sums, so the agreement is also the empirical half of the
proofs in csrc/opening_rules.h; the relation to haf_check_grasps_ref on every found symmetric opening; the block's expected placements;
haf_apply_opening; the refusals; the ABI.  No device: these run without a GPU."""
import ctypes as C

import numpy as np
import pytest

import clearance_cases as cc
import frame_cases as fc
import opening_cases as oc
from haf_grasping_amd import capi
from test_clearance_cpu import gripper_refusals

CASES = oc.small_cases()
_REF = {}


def ref_of(case):
    """the reference's result of a case with its histograms, computed once and shared"""
    name, frame, image, kw, pkw, grasps, mask = case
    if name not in _REF:
        _REF[name] = capi.fit_openings_ref(frame, grasps, capi.gripper(**kw), capi.opening_params(**pkw), mask, hist=True)
    return _REF[name]


BY_NAME = {c[0]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_reference_equals_the_mirror_that_counts_every_placement(case):
    name, frame, image, kw, pkw, grasps, mask = case
    oc.same(ref_of(case), oc.mirror_fit(frame, image, capi.gripper(**kw), capi.opening_params(**pkw), grasps, mask), name)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rows_are_consistent_and_hist_is_optional(case):
    name, frame, image, kw, pkw, grasps, mask = case
    rows, order, info, hist = ref_of(case)
    assert order.tolist() == np.flatnonzero(rows["found"] == 1).tolist()
    void = rows["found"] == -1
    for f in capi.OPENING_DTYPE.names:
        if f != "found":
            assert not rows[f][void | (rows["found"] == 0) if f in ("j", "c", "n_between", "n_finger", "n_palm", "opening_m", "shift_m") else void].any(), f
    assert not hist[void].any()
    assert (hist[:, 0].sum(axis=1) == rows["n_finger_slab"]).all() and (hist[:, 1].sum(axis=1) == rows["n_palm_slab"]).all()
    hb = info["half_bins"]
    assert not hist[:, :, :64 - hb].any() and not hist[:, :, 64 + hb:].any()
    found = rows["found"] == 1
    assert (rows["j"][found] >= info["j_min"]).all() and (rows["j"][found] <= info["j_max"]).all() and (np.abs(rows["c"][found]) <= info["c_max"]).all()
    sym = rows["sym_j"] > 0
    assert (found | ~sym).all() and (rows["j"][sym] <= rows["sym_j"][sym]).all()       # a free (j, 0) is a free placement
    assert (rows["opening_m"] == 2 * rows["j"] * info["bin_m"]).all() and (rows["shift_m"] == rows["c"] * info["bin_m"]).all()
    plain = capi.fit_openings_ref(frame, grasps, capi.gripper(**kw), capi.opening_params(**pkw), mask)
    assert len(plain) == 3 and plain[0].tobytes() == rows.tobytes() and plain[1].tolist() == order.tolist() and plain[2] == info


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_relation_to_check_grasps_at_every_found_symmetric_opening(case):
    """with opening = sym_opening_m (exact in float32): the same n_between, n_finger[i] <= ours, n_palm <= ours, hence free = 1"""
    name, frame, image, kw, pkw, grasps, mask = case
    rows, order, info, hist = ref_of(case)
    p = capi.opening_params(**pkw)
    tb, pb = info["tb"], info["pb"]
    for sj in sorted(set(rows["sym_j"][rows["sym_j"] > 0].tolist())):
        idx = np.flatnonzero(rows["sym_j"] == sj)
        opening = float(rows["sym_opening_m"][idx[0]])
        assert float(np.float32(opening)) == opening
        g = capi.gripper(**dict(kw, opening=opening, max_hits=p.max_hits, min_between=p.min_between))
        clear, _ = capi.check_grasps_ref(frame, [grasps[i] for i in idx], g, mask)
        for r, i in zip(clear, idx):
            h = hist[i].astype(np.int64)
            ours = dict(between=h[0, 64 - sj:64 + sj].sum(), f0=h[0, 64 - sj - tb:64 - sj].sum(), f1=h[0, 64 + sj:64 + sj + tb].sum(),
                        palm=h[1, 64 - pb:64 + pb].sum())
            assert r["n_between"] == ours["between"], (name, i, sj)
            assert r["n_finger"][0] <= ours["f0"] and r["n_finger"][1] <= ours["f1"] and r["n_palm"] <= ours["palm"], (name, i, sj)
            assert r["free"] == 1, (name, i, sj)


def test_the_block_has_the_placements_the_definition_gives():
    """clearance_cases.block_scene(): the 3.9 cm block is +-20 B wide at shift 16 and its edge points lie exactly on bin edges"""
    rows, order, info, _ = ref_of(BY_NAME["block_default"])
    assert (info["shift"], info["tb"], info["pb"], info["j_min"], info["j_max"], info["c_max"]) == (16, 11, 62, 6, 40, 0) and info["half_bins"] == 63
    assert info["bin_m"] == 2.0 ** -10
    r = rows[0]
    assert (r["found"], r["j"], r["c"], r["sym_j"], r["n_between"]) == (1, 21, 0, 21, 441) and r["n_finger"].tolist() == [0, 0] and r["n_palm"] == 0
    assert r["opening_m"] == 42 / 1024 and r["sym_opening_m"] == 42 / 1024 and r["shift_m"] == 0.0 and order.tolist() == [0]
    rows, _, info, _ = ref_of(BY_NAME["block_dx30"])
    assert info["c_max"] == 0 and (rows[0]["found"], rows[0]["j"], rows[0]["c"]) == (1, 28, 0)
    rows, _, info, _ = ref_of(BY_NAME["block_dx30_shift1cm"])
    assert info["shift"] == 17 and (rows[0]["found"], rows[0]["j"], rows[0]["c"]) == (1, 11, -3)
    assert rows[0]["opening_m"] == 22 * 2.0 ** -9 and rows[0]["shift_m"] == -3 * 2.0 ** -9


def test_the_cases_hold_what_they_are_built_for():
    # edges on the aligned axes: an object side one word inside bin 19 is held at j = 20; on the edge s = 20 B or beyond it belongs to the
    # finger there, and from j = 21 on the neighbour in bin 31 is in finger 1 until it lies between the fingers at j = 32; the flipped
    # grasp has the same opening with the fingers exchanged
    for inner, j in ((-1, 20), (0, 32), (1, 32)):
        rows = ref_of(BY_NAME["edge_aligned_in%+d_out+1" % inner])[0]
        assert rows["found"].tolist() == [1, 1] and rows["j"].tolist() == [j, j], (inner, rows)
    # the neighbour ON the outer edge of finger 1 at j = 20 (s = 31 B) is outside it; one word inside it is a hit there
    assert ref_of(BY_NAME["edge_aligned_in-1_out+0"])[0]["j"].tolist() == [20, 20]
    assert ref_of(BY_NAME["edge_aligned_in-1_out-1"])[0]["j"][0] > 20
    h = ref_of(BY_NAME["edge_aligned_in+0_out+0"])[3]
    assert h[0, 0, 64 + 20] == 1 and h[0, 0, 64 - 21] == 1 and h[0, 0, 64 + 31] == 1            # s = +20 B, -20 B, +31 B
    assert h[1, 0, 64 - 21] == 1 and h[1, 0, 64 + 20] == 1 and h[1, 0, 64 - 32] == 1            # the flipped grasp sees them mirrored
    left = ref_of(BY_NAME["edge_aligned_left_only"])
    assert left[2]["shift"] == 17 and left[0]["found"].tolist() == [1, 1] and left[0]["c"][0] == -left[0]["c"][1]
    for a in cc.AXIS_SETS[1:]:
        rows, _, info, hist = ref_of(BY_NAME["edge_" + a[0]])
        assert info["shift"] == 17 and info["c_max"] == 1 and rows["found"].tolist() == [1, 1] and hist[0, 0].sum() == hist[1, 0].sum() == 9
    # packing carry: the sums pass 256 and 65535 nowhere wraps
    rows, _, _, hist = ref_of(BY_NAME["carry_600_600"])
    assert hist[0, 0, 64 + 7] == 600 and hist[0, 1, 64 - 8] == 600 and hist[0].sum() == 1200 and rows[0]["found"] == 1 and rows[0]["n_palm"] == 600
    rows = ref_of(BY_NAME["carry_600_600_hits"])[0]
    assert rows[0]["found"] == 0                              # 600 points in finger 1 or in the palm at every j: one above max_hits
    # the histogram's border
    rows, _, info, hist = ref_of(BY_NAME["hist_border"])
    assert info["half_bins"] == 63 and hist[0, 0, 64 + 62] == 2 and hist[0, 0, 64 - 63] == 2 and hist[0, 0, 0] == 0 and hist[0, 0, 127] == 0
    assert rows[0]["n_finger_slab"] == 5 and rows[0]["n_palm_slab"] == 1
    # params
    assert ref_of(BY_NAME["block_dx30_shift18"])[2]["shift"] == 18
    assert ref_of(BY_NAME["block_dx30_shift_one_bin"])[2]["c_max"] == 1 and ref_of(BY_NAME["block_dx30_shift_2cm"])[2]["c_max"] >= 10
    assert ref_of(BY_NAME["block_dx30_between50"])[0]["n_between"][0] >= 50
    assert ref_of(BY_NAME["block_dx30_min_open"])[2]["j_min"] == 26 and ref_of(BY_NAME["block_dx30_min_open"])[0]["j"][0] >= 26
    # no free placement, for two reasons
    r = ref_of(BY_NAME["inside_the_table"])[0][0]
    assert r["found"] == 0 and r["sym_j"] == 0 and r["n_finger_slab"] > 0
    r = ref_of(BY_NAME["nothing_between"])[0][0]
    assert r["found"] == 0 and r["n_finger_slab"] == 0
    # void grasps
    assert ref_of(BY_NAME["voids_amid_valid"])[0]["found"].tolist().count(-1) == 6
    assert ref_of(BY_NAME["only_void"])[0]["found"].tolist() == [-1] and ref_of(BY_NAME["only_void"])[1].size == 0
    assert ref_of(BY_NAME["edge_of_range"])[0]["found"][3] != -1
    # every size case finds something somewhere: the search is exercised
    assert sum(int((ref_of(c)[0]["found"] == 1).sum()) for c in CASES if c[0].startswith("cloud")) > 20


def test_apply_opening_moves_the_grasp_along_its_closing_axis():
    name, frame, image, kw, pkw, grasps, mask = BY_NAME["block_dx30_shift1cm"]
    rows = ref_of(BY_NAME[name])[0]
    got = capi.apply_opening(dict(grasps[0], eval=77, roll=1.5), rows[0])
    centre = np.array(grasps[0]["averaged_grasp_point"]) + np.array([rows[0]["shift_m"], 0.0, 0.0])
    assert np.allclose(got["averaged_grasp_point"], centre, atol=1e-15)
    assert np.allclose(got["grasp_point1"], centre - [rows[0]["opening_m"] / 2, 0, 0], atol=1e-15)
    assert np.allclose(got["grasp_point2"], centre + [rows[0]["opening_m"] / 2, 0, 0], atol=1e-15)
    assert got["approach_vector"] == grasps[0]["approach_vector"] and got["eval"] == 77 and got["roll"] == 1.5
    # the applied grasp, checked at its own opening, is free: the fingers are where the search put them
    g = capi.gripper(opening=float(rows[0]["opening_m"]))
    clear, order = capi.check_grasps_ref(frame, [got], g)
    assert clear[0]["free"] == 1 and clear[0]["n_between"] == rows[0]["n_between"]
    # an oblique grasp: the move is along c, perpendicular to the approach vector
    grasp = cc.grasp_of((0.1, 0.2, 0.3), (0.2, 0.1, 0.95), (0.04, 0.01, 0.03))
    rec = np.zeros(1, capi.OPENING_DTYPE)[0]
    rec["found"], rec["opening_m"], rec["shift_m"] = 1, 0.05, -0.01
    got = capi.apply_opening(grasp, rec)
    a, b, c, o = (np.array(v) for v in cc.mirror_axes(grasp))
    assert np.allclose(np.array(got["averaged_grasp_point"]) - o, -0.01 * c, atol=1e-15)
    assert np.allclose(np.array(got["grasp_point2"]) - np.array(got["grasp_point1"]), 0.05 * c, atol=1e-15)
    rec["found"] = 0
    with pytest.raises(capi.HafError):
        capi.apply_opening(grasp, rec)
    rec["found"] = 1
    with pytest.raises(capi.HafError):
        capi.apply_opening(cc.grasp_of((0, 0, 0), (0, 0, 1), (0, 0, 1)), rec)     # a void grasp


def test_defaults_the_python_front_and_the_abi():
    p = capi.opening_params()
    assert [round(x, 6) for x in (p.min_opening, p.max_opening, p.max_shift)] == [0.01, 0.08, 0.0] and (p.max_hits, p.min_between) == (0, 1)
    with pytest.raises(TypeError):
        capi.opening_params(opening=1.0)
    for L in (capi.lib(), capi.testlib()):
        assert L.haf_abi_version() == 2                              # the call only adds symbols
        for sym in ("haf_opening_default", "haf_fit_openings_ref", "haf_fit_openings", "haf_apply_opening", "haf_check_grasps", "haf_gripper_default"):
            assert hasattr(L, sym), sym
    assert C.sizeof(capi.OpeningParams) == 20 and C.sizeof(capi.GraspOpening) == 64 and C.sizeof(capi.OpeningInfo) == 40 and capi.OPEN_BINS == 128
    # the gripper's own opening, max_hits and min_between are not read
    case = BY_NAME["block_dx30_shift1cm"]
    name, frame, image, kw, pkw, grasps, mask = case
    other = capi.fit_openings_ref(frame, grasps, capi.gripper(opening=float("nan"), max_hits=-5, min_between=10 ** 6), capi.opening_params(**pkw), mask, hist=True)
    oc.same(other, ref_of(case), "the gripper's opening is not read")


def param_refusals():
    nan, inf = float("nan"), float("inf")
    out = [("%s_%s" % (d, tag), {d: v}) for d in ("min_opening", "max_opening", "max_shift") for tag, v in (("nan", nan), ("inf", inf), ("negative", -0.01))]
    return out + [("max_hits_negative", dict(max_hits=-1)), ("min_between_negative", dict(min_between=-1)), ("min_over_max", dict(min_opening=0.09)),
                  ("max_opening_0", dict(min_opening=0.0, max_opening=0.0)), ("no_whole_bin", dict(min_opening=0.0301, max_opening=0.0302)),
                  ("shift_too_far", dict(max_shift=0.99)), ("shift_huge", dict(max_shift=1e30))]


def refused(call, frame, roi, g, p, n, grasps, stride, code, with_out=True):
    """a refused call has its code and writes nothing"""
    out, order, nf = np.full(8, 0x77, np.uint8).repeat(64).view(capi.OPENING_DTYPE), np.full(8, -7, np.int32), C.c_int32(-7)
    info, hist = capi.OpeningInfo(shift=-7), np.full((8, 2, 128), 0x55, np.uint32)
    before = out.tobytes()
    rc = call(C.byref(frame) if frame is not None else None, C.byref(roi) if roi is not None else None, C.byref(g) if g is not None else None,
              C.byref(p) if p is not None else None, n, grasps, stride, out.ctypes.data if with_out else None, order.ctypes.data, C.byref(nf),
              C.byref(info), hist.ctypes.data)
    assert rc == code, (rc, code)
    assert out.tobytes() == before and (order == -7).all() and nf.value == -7 and info.shift == -7 and (hist == 0x55).all()


def every_refusal(call, ref_form):
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    img = np.full((3, 4), 650, np.uint16)
    good = capi.depth_frame(img, 500.0, 500.0, 2.0, 1.5)
    g, p = capi.gripper(), capi.opening_params()
    grasps, n, stride = capi._grasp_array([cc.grasp_of((0, 0, 0.65), (0, 0, 1), (1, 0, 0))] * 2)
    mask = np.ones((3, 4), np.uint8)
    for name, kw in gripper_refusals():
        if not name.startswith("opening_"):                          # (the gripper's opening is not read)
            refused(call, good, None, capi.gripper(**kw), p, n, grasps, stride, A)
    for name, kw in param_refusals():
        refused(call, good, None, g, capi.opening_params(**kw), n, grasps, stride, A)
    refused(call, None, None, g, p, n, grasps, stride, A)
    refused(call, good, None, None, p, n, grasps, stride, A)
    refused(call, good, None, g, None, n, grasps, stride, A)
    refused(call, good, None, g, p, n, None, stride, A)
    refused(call, good, None, g, p, n, grasps, stride, A, with_out=False)
    for bad_n in (0, -1, capi.MAX_CHECK_GRASPS + 1):
        refused(call, good, None, g, p, bad_n, grasps, stride, A)
    for bad_stride in (0, stride - 8, stride + 4):
        refused(call, good, None, g, p, n, grasps, bad_stride, A)
    for name, frame, code, _ in fc.refusal_frames():                 # everything check_frame refuses for a frame
        refused(call, frame, None, g, p, n, grasps, stride, code)
    refused(call, good, capi.Roi(mask.ctypes.data, 3, 0), g, p, n, grasps, stride, A)        # a mask stride smaller than the width
    refused(call, good, capi.Roi(mask.ctypes.data, 4, 2), g, p, n, grasps, stride, A)
    huge = capi.Frame.from_buffer_copy(good)
    huge.width, huge.height, huge.row_stride_bytes = 1 << 15, (1 << 13) + 1, 2 << 15
    refused(call, huge, None, g, p, n, grasps, stride, CAP)          # more than 2^28 pixels (refused before a pixel is read)
    if ref_form:
        dev = capi.Frame.from_buffer_copy(good)
        dev.on_device = 1
        refused(call, dev, None, g, p, n, grasps, stride, A)         # the _ref form touches no device
        refused(call, good, capi.Roi(mask.ctypes.data, 4, 1), g, p, n, grasps, stride, A)


def test_every_refusal_has_its_code_and_writes_nothing():
    every_refusal(capi.lib().haf_fit_openings_ref, True)
    img = np.full((3, 4), 650, np.uint16)
    good = capi.depth_frame(img, 500.0, 500.0, 2.0, 1.5)
    grasp = cc.grasp_of((0, 0, 0.65), (0, 0, 1), (1, 0, 0))
    rows, order, info = capi.fit_openings_ref(good, [grasp], mask=None)
    assert rows[0]["n_finger_slab"] == 12 and rows[0]["found"] == 1 and rows[0]["j"] == info["j_min"]
    out = np.zeros(1, capi.OPENING_DTYPE)                            # a NULL mask pointer: every pixel; order, n_found, info, hist may be NULL
    arr, n, stride = capi._grasp_array([grasp])
    assert capi.lib().haf_fit_openings_ref(C.byref(good), C.byref(capi.Roi(None, 0, 9)), C.byref(capi.gripper()), C.byref(capi.opening_params()), n,
                                           arr, stride, out.ctypes.data, None, None, None, None) == capi.HAF_OK
    assert out.tobytes() == rows.tobytes()
