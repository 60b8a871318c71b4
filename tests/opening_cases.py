"""Shared by tests/test_opening_cpu.py and tests/test_opening_gpu.py: an independent mirror of haf_fit_openings_ref (include/hafgrasp.h)
and the cases both suites run it on.  The points and a grasp's words are clearance_cases' mirrors (themselves independent of csrc/); the
integers of a call come from Python floats by the header's formulas; and every placement (j, c) is counted DIRECTLY from the s, t, u of
ALL usable points in 64-bit integers: no prefilter, no histogram, no prefix sums -- a bin set [lo, hi) is the interval of s it covers,
closed or open at each end as the header's bin rule says, and a count is the number of points inside it.  Nothing here shares code with
csrc/opening_rules.h, csrc/opening_host.cpp or csrc/opening.hip.

A case is (name, frame, image, gripper kw, params kw, grasps, mask or None)."""
import numpy as np

import clearance_cases as cc
import plane_cases as pc
from haf_grasping_amd import capi

ONE = cc.ONE
W = cc.W


def mirror_info(g, p):
    """the integers of a call, by the header's table -> dict (with the slabs' bounds), or None for what the call refuses"""
    w_open, w_thick, w_palm, w_shift = W(p.max_opening / 2), W(g.finger_thickness), W(g.palm_width / 2), W(p.max_shift)
    E = max(w_open + w_thick, w_palm) + w_shift
    shift = 0
    while (E >> shift) + 2 > 64:
        shift += 1
    B = 1 << shift
    info = dict(shift=shift, half_bins=(E >> shift) + 2, tb=(w_thick >> shift) + 1, pb=(w_palm >> shift) + 1, c_max=w_shift >> shift,
                j_min=max(1, (W(p.min_opening / 2) + B - 1) >> shift), j_max=w_open >> shift, bin_m=B / ONE)
    if info["j_max"] < info["j_min"]:
        return None
    u1 = W(g.finger_length - g.tip_depth)
    info.update(B=B, hb=W(g.finger_breadth / 2), u0=-W(g.tip_depth), u1=u1, hpb=W(g.palm_breadth / 2), u2=u1 + W(g.palm_height))
    return info


class Slab:
    """the s of a slab's points, sorted: counts of bin ranges by their intervals of s"""

    def __init__(self, s, B):
        self.s, self.B = np.sort(np.asarray(s, np.int64)), B

    def below(self, edge):
        """points in the bins below bin `edge`: s < edge B for edge >= 0 (bin edge starts AT edge B), s <= edge B for edge < 0 (bin
        edge - 1 ends AT edge B)"""
        return int(np.searchsorted(self.s, edge * self.B, side="left" if edge >= 0 else "right"))

    def count(self, lo, hi):
        return self.below(hi) - self.below(lo)


def mirror_fit(frame, image, gripper, params, grasps, mask=None):
    """haf_fit_openings_ref by the header's table -> (OPENING_DTYPE [n], order, info, hist uint32 [n, 2, 128])"""
    g = gripper if gripper is not None else capi.gripper()
    p = params if params is not None else capi.opening_params()
    I = mirror_info(g, p)
    assert I is not None
    q = cc.scene_words(frame, image, mask)
    out = np.zeros(len(grasps), capi.OPENING_DTYPE)
    hist = np.zeros((len(grasps), 2, 128), np.uint32)
    hbins, tb, pb = I["half_bins"], I["tb"], I["pb"]
    placements = [(j, c) for j in range(I["j_min"], I["j_max"] + 1) for c in sorted(range(-I["c_max"], I["c_max"] + 1), key=lambda c: (abs(c), c))]
    for i, grasp in enumerate(grasps):
        w = cc.mirror_words(grasp)
        r = out[i]
        if w is None:
            r["found"] = -1
            continue
        A, Bw, C, o = (np.array(v, np.int64) for v in w)
        d = q - o
        s, t, u = d @ C, d @ Bw, d @ A
        in_f = (np.abs(t) <= I["hb"]) & (u >= I["u0"]) & (u < I["u1"])
        in_p = (np.abs(t) <= I["hpb"]) & (u >= I["u1"]) & (u <= I["u2"])
        assert not (in_f & in_p).any()
        fs, ps = Slab(s[in_f], I["B"]), Slab(s[in_p], I["B"])
        r["n_finger_slab"], r["n_palm_slab"] = fs.count(-hbins, hbins), ps.count(-hbins, hbins)
        for k in range(-hbins, hbins):
            hist[i, 0, 64 + k], hist[i, 1, 64 + k] = fs.count(k, k + 1), ps.count(k, k + 1)

        def counts(j, c):
            return fs.count(c - j, c + j), fs.count(c - j - tb, c - j), fs.count(c + j, c + j + tb), ps.count(c - pb, c + pb)

        def free(n):
            return n[1] + n[2] + n[3] <= p.max_hits and n[0] >= p.min_between

        for j, c in placements:
            n = counts(j, c)
            if free(n):
                r["found"], r["j"], r["c"] = 1, j, c
                r["n_between"], r["n_finger"], r["n_palm"] = n[0], (n[1], n[2]), n[3]
                r["opening_m"], r["shift_m"] = 2 * j * I["B"] / ONE, c * I["B"] / ONE
                break
        for j in range(I["j_min"], I["j_max"] + 1):
            if free(counts(j, 0)):
                r["sym_j"], r["sym_opening_m"] = j, 2 * j * I["B"] / ONE
                break
    info = {k: I[k] for k in ("shift", "half_bins", "tb", "pb", "j_min", "j_max", "c_max", "bin_m")}
    return out, np.flatnonzero(out["found"] == 1).astype(np.int32), info, hist


def same(got, want, where=""):
    """two (rows, order, info, hist) results agree in every word"""
    (rows, order, info, hist), (wrows, worder, winfo, whist) = got, want
    assert rows.dtype == wrows.dtype == capi.OPENING_DTYPE and rows.shape == wrows.shape, (where, rows.shape, wrows.shape)
    if rows.tobytes() != wrows.tobytes():
        for f in capi.OPENING_DTYPE.names:
            bad = np.flatnonzero((rows[f] != wrows[f]).reshape(len(rows), -1).any(axis=1))
            assert bad.size == 0, (where, f, bad[:5], rows[f][bad[:5]], wrows[f][bad[:5]])
    assert rows.tobytes() == wrows.tobytes(), where
    assert order.tolist() == worder.tolist(), (where, "order")
    assert info == winfo, (where, info, winfo)
    assert hist.dtype == whist.dtype == np.uint32 and hist.shape == whist.shape, (where, hist.shape, whist.shape)
    bad = np.argwhere(hist != whist)
    assert bad.size == 0, (where, "histogram", bad[:5], hist[tuple(bad[0])], whist[tuple(bad[0])])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

ALIGNED = cc.AXIS_SETS[0]                                 # approach +z, closing +x: s = 16384 dx, so a bin of 2^16 is 4 coordinate words


def aligned_case(name, offsets, gripper_kw=None, params_kw=None, with_flipped=True):
    """points at the aligned grasp's origin + offsets (words: dx along the closing axis, dy across, dz along the approach vector)"""
    _, o_words, approach, closing = ALIGNED
    origin = np.array(o_words, np.float64) / 4096.0
    grasp = cc.grasp_of(origin, approach, closing)
    pts = (np.array(offsets, np.int64).reshape(-1, 3) + np.array(o_words, np.int64)) / 4096.0
    frame, image = cc.cloud_case(pts)
    return (name, frame, image, gripper_kw or {}, params_kw or {}, [grasp, cc.flipped(grasp)] if with_flipped else [grasp], None)


def edge_cases_aligned():
    """an object whose two sides lie dx words from the grasp point, around j = 20 bins (dx = 80), and a neighbour around the outer edge of
    finger 1 at that j (j + tb = 31 bins, dx = 124): each at the edge, one word inside and one word outside.  The neighbour is on the +
    side only, so the flipped grasp sees it at finger 0"""
    out = []
    for inner in (-1, 0, 1):
        for outer in (-1, 0, 1):
            offs = [(80 + inner, 0, 0), (-80 - inner, 2, -3), (124 + outer, -1, 2)]
            out.append(aligned_case("edge_aligned_in%+d_out%+d" % (inner, outer), offs))
    # the left side alone on an edge, the right one inside: the sides are told apart
    out.append(aligned_case("edge_aligned_left_only", [(-80, 0, 0), (79, 0, 0), (-124, 0, 0)], params_kw=dict(max_shift=0.004)))
    return out


def edge_case_rotated(axis_set):
    """on a rotated axis set no word of s is a round number: points whose s is EXACTLY a multiple of the call's B are found by search in the
    words around three places along the closing axis (the object's two sides, a neighbour by the outer finger edge), and each goes in with
    its two neighbours along the closing axis' largest component"""
    name, o_words, approach, closing = axis_set
    origin = np.array(o_words, np.float64) / 4096.0
    grasp = cc.grasp_of(origin, approach, closing)
    a, b, c, _ = (np.array(v) for v in cc.mirror_axes(grasp))
    A, Bw, C, o = (np.array(v, np.int64) for v in cc.mirror_words(grasp))
    pkw = dict(max_shift=0.003)
    info = mirror_info(capi.gripper(), capi.opening_params(**pkw))
    B = info["B"]
    r = np.arange(-50, 51)
    cube = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    step = np.zeros(3, np.int64)
    step[np.argmax(np.abs(C))] = 1
    offs = []
    for sm in (0.0195, -0.0195, 0.0195 + info["tb"] * B / ONE):
        d = np.rint(4096.0 * sm * c).astype(np.int64) + cube
        s, t, u = d @ C, d @ Bw, d @ A
        hit = np.flatnonzero((s % B == 0) & (np.abs(t) < 600000) & (np.abs(u) < 1800000))     # inside the finger slab (|t| <= 671089, |u| < 2013265)
        assert hit.size > 0, name
        best = d[hit[np.argmin(np.abs(t[hit]) + np.abs(u[hit]))]]
        offs += [best, best + step, best - step]
    pts = (np.array(offs, np.int64) + o) / 4096.0
    frame, image = cc.cloud_case(pts)
    return ("edge_%s" % name, frame, image, {}, pkw, [grasp, cc.flipped(grasp)], None)


def block_at(dx_words=0, dz_words=cc.BLOCK_GRASP_Z, name="block", gripper_kw=None, params_kw=None):
    """clearance_cases' block under a grasp whose origin is moved dx_words along x (the closing axis)"""
    pts, _ = cc.block_scene()
    frame, image = cc.cloud_case(pts / 4096.0)
    grasp = cc.grasp_of((dx_words / 4096.0, 0.0, dz_words / 4096.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), half=0.03)
    return (name, frame, image, gripper_kw or {}, params_kw or {}, [grasp], None)


def small_cases():
    out = edge_cases_aligned() + [edge_case_rotated(a) for a in cc.AXIS_SETS[1:]]
    # sizes: the tile, wave and slot borders
    rng = np.random.default_rng(20250921)
    for n_px in (1, 255, 256, 257, 1025):
        pts = np.array([0.3, -0.2, 0.5]) + rng.uniform(-0.04, 0.04, (n_px, 3))
        frame, image = cc.cloud_case(pts)
        for n_g in (1, 63, 64, 65, 257):
            out.append(("cloud%d_grasps%d" % (n_px, n_g), frame, image, {}, dict(max_hits=3 if n_g % 2 else 40, max_shift=0.005 if n_px % 2 else 0.0),
                        cc.random_grasps(rng, pts, n_g), None))
    # packing carry: 600 identical points in one finger-slab bin, 600 in one palm-slab bin of the same grasp -- two whole tiles of 256
    # points of one bin, and a tile that holds both slabs
    out.append(aligned_case("carry_600_600", [(30, 0, 0)] * 600 + [(-30, 0, 180)] * 600, params_kw=dict(max_hits=2000, min_between=600)))
    out.append(aligned_case("carry_600_600_hits", [(130, 0, 0)] * 600 + [(-30, 0, 180)] * 600 + [(3, 0, 0)], params_kw=dict(max_hits=599)))
    # the histogram's border at the defaults (half_bins = 63, B = 4 words): bins 62, 63 and -63, -64; s = +-63 B and -62 B exactly
    border = [(250, 0, 0), (254, 0, 0), (-250, 0, 0), (-254, 0, 0), (252, 0, 0), (-252, 0, 0), (-248, 0, 0), (248, 0, 0), (251, 0, 200), (-253, 0, 200),
              (2, 0, 0)]
    out.append(aligned_case("hist_border", border))
    # kinds, strides, masks
    for tag, frame, image, pose in cc.boxes_frames():
        anchors = cc.base_points(frame, image)
        up = np.array(pc.up_of(pose))
        grasps = [cc.grasp_of(anchors[rng.integers(len(anchors))] + 0.01 * up, up + rng.normal(scale=0.2, size=3), rng.normal(size=3)) for _ in range(65)]
        out.append(("boxes_%s" % tag, frame, image, {}, dict(max_hits=2), grasps, None))
        mask = (rng.random(image.shape[:2]) < 0.6).astype(np.uint8)
        out.append(("boxes_masked_%s" % tag, frame, image, dict(finger_thickness=0.006), dict(max_hits=3, max_shift=0.01), grasps, pc.padded_mask(mask, 5)))
    # params, on the block under an off-centre grasp
    one_bin = (1 << 16) / ONE
    for tag, gkw, pkw in (("hits0", {}, dict(max_hits=0)), ("hits3", {}, dict(max_hits=3)), ("between1", {}, dict(min_between=1, max_shift=0.01)),
                          ("between50", {}, dict(min_between=50, max_shift=0.01)), ("shift_one_bin", {}, dict(max_shift=one_bin)),
                          ("shift_2cm", {}, dict(max_shift=0.02)), ("shift18", dict(palm_width=0.26), dict(max_shift=0.01)),
                          ("min_open", {}, dict(min_opening=0.05, max_opening=0.075)), ("deep_tips", dict(tip_depth=0.05), dict(max_hits=3, max_shift=0.01))):
        out.append(block_at(30, name="block_dx30_" + tag, gripper_kw=gkw, params_kw=pkw))
    out.append(block_at(0, name="block_default"))
    out.append(block_at(30, name="block_dx30"))
    out.append(block_at(30, name="block_dx30_shift1cm", params_kw=dict(max_shift=0.01)))
    # no free placement: the fingers inside the table's points at every j; nothing between the fingers at any j
    out.append(block_at(300, dz_words=20, name="inside_the_table", params_kw=dict(max_shift=0.01)))
    out.append(block_at(0, dz_words=600, name="nothing_between", params_kw=dict(max_shift=0.01)))
    # void grasps, and the points at the edge of the range
    by_name = {c[0]: c for c in cc.small_cases()}
    for name in ("voids_amid_valid", "only_void", "edge_of_range", "far_origin"):
        _, frame, image, kw, grasps, mask = by_name[name]
        out.append((name, frame, image, kw, dict(max_hits=5, max_shift=0.004), grasps, mask))
    assert len({c[0] for c in out}) == len(out)
    return out
