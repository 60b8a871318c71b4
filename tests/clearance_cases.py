"""Shared by tests/test_clearance_cpu.py and tests/test_clearance_gpu.py: an independent mirror of haf_check_grasps_ref
(include/hafgrasp.h) and the cases both suites run it on.  The points are frame_cases.mirror_points'; a grasp's twelve words come from
Python floats in the header's order, the bounds from round(x * 2**26), and every region test runs over ALL usable points of the frame in
64-bit integers with NO prefilter -- only n_near itself uses reach_q.  Nothing here shares code with csrc/clearance_host.cpp or
csrc/clearance.hip.

The cases are synthetic: points placed by construction in the gripper frame of a given grasp and mapped back.  A FACE case builds the
gripper from the points: each bound's word is the exact integer coordinate (s, t or u) of one point, so that point lies exactly on the
face; delta = -1 / +1 moves every bound by one word of 2^-26 m, which puts the same points one word outside / inside.  A second grasp with
its two grasp points swapped (C and B negated) sees every such point on the opposite face."""
import math

import numpy as np

import frame_cases as fc
import plane_cases as pc
from haf_grasping_amd import capi

F = np.float32
ONE = 1 << 26
POSE_FIELDS = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector")


def W(x):
    return int(round(float(x) * ONE))                     # (x * 2^26 is exact in double; round() goes to the nearest even)


def mirror_bounds(g):
    ho, fo = g.opening / 2, g.opening / 2 + g.finger_thickness
    u1 = g.finger_length - g.tip_depth
    u2 = u1 + g.palm_height
    es, et = max(fo, g.palm_width / 2), max(g.finger_breadth, g.palm_breadth) / 2
    eu = max(g.tip_depth, abs(u1), abs(u2))
    reach = math.sqrt(es * es + et * et + eu * eu)
    return dict(ho=W(ho), fo=W(fo), hb=W(g.finger_breadth / 2), u0=-W(g.tip_depth), u1=W(u1), hpw=W(g.palm_width / 2), hpb=W(g.palm_breadth / 2),
                u2=W(u1) + W(g.palm_height), reach_q=int(math.ceil(reach * 4096.0)) + 3)


def mirror_axes(grasp):
    """-> (a, b, c, origin) as unit float triples, or None for a void grasp"""
    p1, p2, o, av = (tuple(float(x) for x in grasp[f]) for f in POSE_FIELDS)
    if not all(math.isfinite(x) for v in (p1, p2, o, av) for x in v):
        return None
    an = math.sqrt(av[0] * av[0] + av[1] * av[1] + av[2] * av[2])
    if not an >= 1e-6:
        return None
    a = [x / an for x in av]
    g = [p2[j] - p1[j] for j in range(3)]
    gn = math.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    if not gn >= 1e-6:
        return None
    ga = g[0] * a[0] + g[1] * a[1] + g[2] * a[2]
    c = [g[j] - ga * a[j] for j in range(3)]
    cn = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    if not cn >= 1e-3 * gn or any(abs(x) > 16.0 for x in o):
        return None
    c = [x / cn for x in c]
    b = [a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]]
    return a, b, c, o


def mirror_words(grasp):
    """-> (A, B, C, o) integer triples, or None for a void grasp"""
    ax = mirror_axes(grasp)
    if ax is None:
        return None
    a, b, c, o = ax
    return tuple([int(round(16384.0 * x)) for x in v] for v in (a, b, c)) + ([int(round(4096.0 * x)) for x in o], )


def scene_words(frame, image, mask=None):
    """the usable, admitted points of the frame as int64 [n, 3] coordinate words"""
    words = fc.mirror_points(frame, image)
    usable = ((words & 0x7FFFFFFF) <= 0x41800000).all(axis=1)
    if mask is not None:
        usable &= np.asarray(mask).reshape(-1) != 0
    return np.rint(words.view(F)[usable] * F(4096)).astype(np.int64)


def mirror_check(frame, image, gripper, grasps, mask=None):
    """haf_check_grasps_ref by the header's table -> (CLEARANCE_DTYPE [n], order)"""
    g = gripper if gripper is not None else capi.gripper()
    bd = mirror_bounds(g)
    q = scene_words(frame, image, mask)
    out = np.zeros(len(grasps), capi.CLEARANCE_DTYPE)
    for i, grasp in enumerate(grasps):
        w = mirror_words(grasp)
        r = out[i]
        if w is None:
            r["free"] = -1
            continue
        A, B, C, o = (np.array(v, np.int64) for v in w)
        d = q - o
        s, t, u = d @ C, d @ B, d @ A
        fing = (np.abs(t) <= bd["hb"]) & (u >= bd["u0"]) & (u < bd["u1"])
        between = fing & (s > -bd["ho"]) & (s < bd["ho"])
        f0 = fing & (s >= -bd["fo"]) & (s <= -bd["ho"])
        f1 = fing & (s >= bd["ho"]) & (s <= bd["fo"])
        palm = (np.abs(s) <= bd["hpw"]) & (np.abs(t) <= bd["hpb"]) & (u >= bd["u1"]) & (u <= bd["u2"])
        assert int(between.sum() + f0.sum() + f1.sum() + palm.sum()) == int((between | f0 | f1 | palm).sum()), "the regions are disjoint"
        r["n_near"] = int((np.abs(d) <= bd["reach_q"]).all(axis=1).sum())
        r["n_finger"] = (int(f0.sum()), int(f1.sum()))
        r["n_palm"], r["n_between"] = int(palm.sum()), int(between.sum())
        if between.any():
            smin, smax, umax = int(s[between].min()), int(s[between].max()), int(u[between].max())
            r["s_min"], r["s_max"], r["u_max"] = smin, smax, umax
            r["width_m"], r["offset_m"], r["top_m"] = (smax - smin) / ONE, (smax + smin) / ONE / 2, umax / ONE
        r["free"] = int(int(f0.sum() + f1.sum() + palm.sum()) <= g.max_hits and int(between.sum()) >= g.min_between)
    return out, np.flatnonzero(out["free"] == 1).astype(np.int32)


def same(got, want, where=""):
    """two (rows, order) results agree in every word"""
    (rows, order), (wrows, worder) = got, want
    assert rows.dtype == wrows.dtype == capi.CLEARANCE_DTYPE and rows.shape == wrows.shape, (where, rows.shape, wrows.shape)
    if rows.tobytes() != wrows.tobytes():
        for f in capi.CLEARANCE_DTYPE.names:
            bad = np.flatnonzero((rows[f] != wrows[f]).reshape(len(rows), -1).any(axis=1))
            assert bad.size == 0, (where, f, bad[:5], rows[f][bad[:5]], wrows[f][bad[:5]])
    assert rows.tobytes() == wrows.tobytes(), where
    assert order.tolist() == worder.tolist(), (where, "order")


# ---- grasps and scenes ----------------------------------------------------------------------------------------------------------------

def grasp_of(origin, approach, closing, half=0.02):
    """a grasp dict: the grasp points at origin -+ half * closing (closing need not be perpendicular to approach, nor of unit length)"""
    o, c = np.asarray(origin, np.float64), np.asarray(closing, np.float64)
    return dict(grasp_point1=tuple(o - half * c), grasp_point2=tuple(o + half * c), averaged_grasp_point=tuple(o), approach_vector=tuple(approach))


def flipped(grasp):
    return dict(grasp, grasp_point1=grasp["grasp_point2"], grasp_point2=grasp["grasp_point1"])


def cloud_case(points):
    """float [n, 3] -> (frame, image) of an N x 1 unorganised cloud"""
    xyz = np.ascontiguousarray(points, F)
    frame = capi.cloud_frame(xyz)
    return frame, xyz.reshape(1, -1, 3)


def random_grasps(rng, anchors, n):
    """n grasps at random anchors (+- 1 cm) with random approach and closing directions"""
    out = []
    for i in range(n):
        o = anchors[rng.integers(len(anchors))] + rng.uniform(-0.01, 0.01, 3)
        out.append(grasp_of(o, rng.normal(size=3), rng.normal(size=3)))
    return out


AXIS_SETS = [   # (name, origin in words, approach, closing)
    ("aligned", (1234, -2345, 3456), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
    ("rotated_a", (-777, 4001, 2222), (0.3, -0.5, 0.81), (0.7, 0.6, 0.2)),
    ("rotated_b", (30001, -15000, 8191), (-0.6, 0.35, 0.72), (0.25, -0.8, 0.45)),
    ("oblique", (5, 7, 4100), (0.2, 0.1, 0.95), (0.04, 0.01, 0.03)),          # gp2 - gp1 is far from perpendicular to the approach vector
]
# nominal (s, t, u) in metres of the point that DEFINES each bound: the other two coordinates lie well inside the region
FACE_POINTS = dict(ho=(0.04, 0.0, 0.0), fo=(0.05, 0.005, 0.01), hb=(0.01, 0.01, 0.0), u0=(0.0, 0.0, -0.03), u1=(0.01, 0.002, 0.03),
                   u2=(0.02, 0.0, 0.07), hpw=(0.06, 0.0, 0.05), hpb=(0.03, 0.02, 0.05))


def face_case(axis_set, delta):
    """-> (name, frame, image, gripper kw, grasps, mask, bounds by name): see the module's docstring"""
    name, o_words, approach, closing = axis_set
    origin = np.array(o_words, np.float64) / 4096.0       # exact
    grasp = grasp_of(origin, approach, closing)
    a, b, c, _ = (np.array(v) for v in mirror_axes(grasp))
    A, B, C, o = (np.array(v, np.int64) for v in mirror_words(grasp))
    assert o.tolist() == list(o_words)
    if name != "aligned":
        assert name == "oblique" or (np.concatenate([A, B, C]) != 0).all()
    d_of, coord = {}, {}
    for key, (sm, tm, um) in FACE_POINTS.items():
        d = np.rint(4096.0 * (sm * c + tm * b + um * a)).astype(np.int64)
        d_of[key] = d
        coord[key] = dict(s=int(d @ C), t=int(d @ B), u=int(d @ A))
    bd = dict(ho=coord["ho"]["s"], fo=coord["fo"]["s"], hb=coord["hb"]["t"], td=-coord["u0"]["u"], u1=coord["u1"]["u"], u2=coord["u2"]["u"],
              hpw=coord["hpw"]["s"], hpb=coord["hpb"]["t"])
    bd = {k: v + delta for k, v in bd.items()}
    kw = dict(opening=2 * bd["ho"] / ONE, finger_thickness=(bd["fo"] - bd["ho"]) / ONE, finger_breadth=2 * bd["hb"] / ONE, tip_depth=bd["td"] / ONE,
              finger_length=(bd["u1"] + bd["td"]) / ONE, palm_width=2 * bd["hpw"] / ONE, palm_breadth=2 * bd["hpb"] / ONE,
              palm_height=(bd["u2"] - bd["u1"]) / ONE)
    got = mirror_bounds(capi.gripper(**kw))               # every dimension is exact in float32, so the bounds are the words asked for
    assert (got["ho"], got["fo"], got["hb"], -got["u0"], got["u1"], got["u2"], got["hpw"], got["hpb"]) == \
           (bd["ho"], bd["fo"], bd["hb"], bd["td"], bd["u1"], bd["u2"], bd["hpw"], bd["hpb"]), (got, bd)
    rng = np.random.default_rng([77, delta + 1, len(name)])
    ds = [d for d in d_of.values()] + [-d for d in d_of.values()] + list(rng.integers(-400, 400, (20, 3)))
    pts = (np.array(ds, np.int64) + o) / 4096.0            # exact in float32: |word| < 2^24
    frame, image = cloud_case(pts)
    return ("face_%s_%+d" % (name, delta), frame, image, kw, [grasp, flipped(grasp)], None), coord


def block_scene():
    """a 160 x 400 x 200 word block (3.9 x 9.8 x 4.9 cm) of points, 10 words (2.4 mm) apart, on a plane of points z = 0 -> (points
    in words, the block's extent in words along x)"""
    step = 10
    gx, gy = np.meshgrid(np.arange(-600, 601, step), np.arange(-600, 601, step))
    under = (np.abs(gx) <= 80) & (np.abs(gy) <= 200)
    plane = np.stack([gx[~under], gy[~under], np.zeros((~under).sum(), np.int64)], axis=1)
    tx, ty = np.meshgrid(np.arange(-80, 81, step), np.arange(-200, 201, step))
    top = np.stack([tx.ravel(), ty.ravel(), np.full(tx.size, 200)], axis=1)
    sides = []
    for z in range(step, 200, step):
        for x in (-80, 80):
            sides += [(x, y, z) for y in range(-200, 201, step)]
        for y in (-200, 200):
            sides += [(x, y, z) for x in range(-80 + step, 80, step)]
    return np.concatenate([plane, top, np.array(sides, np.int64)]), 160


BLOCK_GRASP_Z = 160                                       # words: the grasp point's height over the plane, 3.9 cm


def block_case(**gripper_kw):
    pts, extent = block_scene()
    frame, image = cloud_case(pts / 4096.0)
    grasp = grasp_of((0.0, 0.0, BLOCK_GRASP_Z / 4096.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), half=0.03)
    return ("block_" + "_".join("%s%g" % kv for kv in sorted(gripper_kw.items())) if gripper_kw else "block_default",
            frame, image, gripper_kw, [grasp], None), extent


def boxes_frames():
    """pc's table with two boxes, 67 x 33, as every kind: padded rows, and 16- and 32-byte points for XYZ -> [(tag, frame, image, pose)]"""
    w, h = pc.SHAPES[0]
    rng = np.random.default_rng([20250607, w, h])
    tilted = fc.tilted_pose(rng)
    z = pc.boxes_z(w, h, rng, noise=0.002)
    out = []
    for kind, pad in (("u16", 3), ("f32", 5), ("u16", 0)):
        frame, img = pc.depth_frame_of(z, kind, tilted, pad)
        out.append(("%s_pad%d" % (kind, pad), frame, img, tilted))
    u, v = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    zf = z.astype(F)
    xyz = np.stack([(u - F((w - 1) / 2.0)) / F(pc.FX) * zf, (v - F((h - 1) / 2.0)) / F(pc.FX) * zf, zf], axis=2).astype(F)
    for floats in (4, 8):
        wide = np.full((h, w + 2, floats), 777.0, F)      # padded rows, padded points
        wide[:, :w, :3] = xyz
        img = wide[:, :w, :]
        out.append(("xyz_stride%d" % (4 * floats), capi.xyz_frame(img, sensor_to_base=tilted), img, tilted))
    return out


def base_points(frame, image):
    """the frame's usable points in the base frame, metres (float64 [n, 3])"""
    return scene_words(frame, image) / 4096.0


def small_cases():
    """-> [(name, frame, image, gripper kw, grasps, mask or None)]"""
    out = []
    # faces: strict against inclusive comparisons, on four axis sets
    for axis_set in AXIS_SETS:
        for delta in (-1, 0, 1):
            out.append(face_case(axis_set, delta)[0])
    # sizes: the tile, wave and workgroup borders
    rng = np.random.default_rng(20250608)
    for n_px in (1, 511, 512, 513, 1025):
        pts = np.array([0.3, -0.2, 0.5]) + rng.uniform(-0.08, 0.08, (n_px, 3))
        frame, image = cloud_case(pts)
        for n_g in (1, 63, 64, 65, 257):
            out.append(("cloud%d_grasps%d" % (n_px, n_g), frame, image, {}, random_grasps(rng, pts, n_g), None))
    z = 0.7 + 0.05 * rng.random((29, 37))
    frame, image = pc.depth_frame_of(z, "u16", pc.IDENTITY)
    anchors = base_points(frame, image)
    for n_g in (1, 65, 257):
        out.append(("u16_37x29_grasps%d" % n_g, frame, image, {}, random_grasps(rng, anchors, n_g), None))
    # kinds, strides, masks
    for tag, frame, image, pose in boxes_frames():
        anchors = base_points(frame, image)
        up = np.array(pc.up_of(pose))
        grasps = [grasp_of(anchors[rng.integers(len(anchors))] + 0.01 * up, up + rng.normal(scale=0.2, size=3), rng.normal(size=3)) for _ in range(65)]
        out.append(("boxes_%s" % tag, frame, image, {}, grasps, None))
        mask = (rng.random(image.shape[:2]) < 0.6).astype(np.uint8)
        out.append(("boxes_masked_%s" % tag, frame, image, dict(opening=0.05, max_hits=3), grasps, pc.padded_mask(mask, 5)))
    # unusable points: NaN, infinities, exactly 16 m (usable) and the next float above it (not), around an origin at the range's edge
    above = np.nextafter(F(16.0), F(32.0))
    pts = np.array([[16.0, 0.0, 0.0], [above, 0.0, 0.0], [15.99, 0.01, 0.0], [np.nan, 0.0, 0.0], [15.98, np.inf, 0.0], [15.99, 0.0, -np.inf],
                    [-16.0, 0.0, 0.0], [-above, 0.0, 0.0], [-15.99, 0.0, 0.01], [15.995, 0.005, 16.0], [15.995, 0.005, above],
                    [15.99, -0.01, 0.005], [16.0, 0.02, 0.0], [-16.0, -16.0, -16.0]], np.float64)
    edge = [grasp_of((15.99, 0.0, 0.0), (0, 0, 1), (1, 0, 0)), grasp_of((-15.99, 0.0, 0.0), (0, 0, 1), (0, 1, 0)),
            grasp_of((16.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0)), grasp_of((-16.0, -16.0, -16.0), (1, 1, 1), (1, -1, 0))]
    frame, image = cloud_case(pts)
    out.append(("edge_of_range", frame, image, {}, edge, None))
    zero = np.zeros((29, 37), np.uint16)
    zero[3, 5] = 700
    frame = capi.depth_frame(zero, 100.0, 100.0, 18.0, 14.0)
    out.append(("u16_zeros", frame, zero, {}, [grasp_of((-0.091, -0.077, 0.7), (0, 0, 1), (1, 0, 0)), grasp_of((0.1, 0.1, 0.7), (0, 0, 1), (1, 0, 0))], None))
    # origins: nothing near; void grasps of every kind amid valid ones
    pts = np.array([0.1, 0.1, 0.1]) + rng.uniform(-0.05, 0.05, (300, 3))
    frame, image = cloud_case(pts)
    ok = random_grasps(rng, pts, 6)
    nan_grasp = dict(ok[0], grasp_point2=(0.1, float("nan"), 0.1))
    voids = [grasp_of(pts[0], (0, 0, 1), (0, 0, 0)),                  # g = 0
             grasp_of(pts[1], (0, 0, 1), (0, 0, 1)),                  # g parallel to a
             nan_grasp,
             grasp_of((0.1, 16.5, 0.1), (0, 0, 1), (1, 0, 0)),        # origin beyond 16 m
             grasp_of(pts[2], (0, 0, 0), (1, 0, 0)),                  # no approach vector
             dict(ok[1], approach_vector=(0.0, float("inf"), 1.0))]
    out.append(("far_origin", frame, image, {}, [grasp_of((15.9, 0.1, 0.1), (0, 0, 1), (1, 0, 0)), ok[0]], None))
    out.append(("voids_amid_valid", frame, image, {}, [ok[0], voids[0], ok[1], voids[1], voids[2], ok[2], voids[3], ok[3], voids[4], voids[5], ok[4], ok[5]], None))
    out.append(("only_void", frame, image, {}, [voids[0]], None))
    # the block
    for kw in ({}, dict(opening=0.03), dict(tip_depth=0.05)):
        out.append(block_case(**kw)[0])
    # a mask that removes exactly the colliding points: free flips
    case, _ = block_case(opening=0.03)
    name, frame, image, kw, grasps, _ = case
    q = scene_words(frame, image)
    A, B, C, o = (np.array(v, np.int64) for v in mirror_words(grasps[0]))
    s = (q - o) @ C
    bd = mirror_bounds(capi.gripper(**kw))
    mask = (np.abs(s) < bd["ho"]).astype(np.uint8).reshape(1, -1)     # only what lies strictly between the fingers' inner faces
    out.append(("block_masked_free", frame, image, kw, grasps, mask))
    return out
