"""Shared by tests/test_space_cpu.py and tests/test_space_gpu.py: an independent mirror of haf_check_space_ref (include/hafgrasp.h;
csrc/space_rules.h) and the cases both suites run it on.  The mirror uses numpy int64 for the lattice, the sample points and the
projection (plain //), np.float32 operations one at a time for the twelve-step transform, as transfer_cases.restate does, and Python
integers for the constants.  It takes clearance_cases' mirror of a grasp's words and of the gripper's bounds, transfer_cases.rne and
capi.invert_pose's output as given; nothing here shares code with csrc/.

A case is a dict: name, views [(frame, image)], grasps (dicts), gripper kw, params kw, candidates (the grasps go in as a
haf_grasp_candidate[]), expect [(grasp, sample, state)] -- samples whose state the case's builder fixed by construction -- and merges,
the names of the merge rules its expectations exercise."""
import ctypes as C

import numpy as np

import clearance_cases as cc
import transfer_cases as tc
from haf_grasping_amd import capi

F = np.float32
UNSEEN, HIDDEN, FREE, HIT = range(4)
BETWEEN, FINGER0, FINGER1, PALM = range(4)
FAR_WORD = 1 << 20
CHUNK = 256                           # kSpaceChunk: samples per workgroup of k_space_samples
IDENTITY = np.eye(3, 4, dtype=F)
EXACT_SCALE = 2.0 ** -16              # depth_scale of the boundary cases: Zobs is the stored integer


# ---- the independent mirror -----------------------------------------------------------------------------------------------------------

def mirror_lattice(grip, params):
    """-> dict(S, n [4][3], N, region int64 [N], stu int64 [N, 3])"""
    bd = cc.mirror_bounds(grip)
    S = cc.W(params.sample_step)
    boxes = [((-bd["ho"], bd["ho"]), (-bd["hb"], bd["hb"]), (bd["u0"], bd["u1"])),
             ((-bd["fo"], -bd["ho"]), (-bd["hb"], bd["hb"]), (bd["u0"], bd["u1"])),
             ((bd["ho"], bd["fo"]), (-bd["hb"], bd["hb"]), (bd["u0"], bd["u1"])),
             ((-bd["hpw"], bd["hpw"]), (-bd["hpb"], bd["hpb"]), (bd["u1"], bd["u2"]))]
    ns, regions, points = [], [], []
    for r, box in enumerate(boxes):
        if any(hi - lo <= 0 for lo, hi in box):
            ns.append([0, 0, 0])
            continue
        n = [max(1, (hi - lo) // S) for lo, hi in box]
        ns.append(n)
        axes = [np.array([lo + ((2 * k + 1) * (hi - lo)) // (2 * n[a]) for k in range(n[a])], np.int64) for a, (lo, hi) in enumerate(box)]
        u, t, s = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")      # u slowest, s fastest
        points.append(np.stack([s.ravel(), t.ravel(), u.ravel()], axis=1))
        regions.append(np.full(s.size, r, np.int64))
    stu = np.concatenate(points) if points else np.zeros((0, 3), np.int64)
    region = np.concatenate(regions) if regions else np.zeros(0, np.int64)
    return dict(S=S, n=ns, N=len(stu), region=region, stu=stu)


def mirror_points(words, stu):
    """a grasp's (A, B, C, o) and the lattice -> Pq int64 [N, 3], words of 1/65536 m"""
    A, B, Cw, o = (np.array(v, np.int64) for v in words)
    P = o * (1 << 28) + stu[:, 0:1] * Cw + stu[:, 1:2] * B + stu[:, 2:3] * A
    assert (np.abs(P) < (1 << 45)).all()
    return (P + (1 << 23)) >> 24


def view_constants(frame, params):
    near = max(1, tc.rne(float(F(params.near_m)) * 65536.0))
    ta = min(tc.rne(float(F(params.tol_abs)) * 65536.0), tc.INT32_MAX)
    return dict(FX=tc.rne(float(F(frame.fx)) * 256.0), FY=tc.rne(float(F(frame.fy)) * 256.0), CX=tc.rne(float(F(frame.cx)) * 256.0),
                CY=tc.rne(float(F(frame.cy)) * 256.0), NEAR=near, TA=ta, TR=tc.rne(float(F(params.tol_rel)) * 65536.0))


def mirror_project(frame, params, Pq):
    """-> (projects bool [N], Qz, uc, vc int64 [N]) of the sample words in one view"""
    k = view_constants(frame, params)
    m = capi.invert_pose(np.array(list(frame.sensor_to_base), F))
    p = Pq.astype(F) * F(1.0 / 65536.0)
    assert (p.astype(np.float64) * 65536.0 == Pq).all()
    with np.errstate(all="ignore"):
        q = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], axis=1)
    assert q.dtype == F
    ok = np.isfinite(q).all(axis=1) & (np.abs(q) <= F(16.0)).all(axis=1)
    Q = np.rint(np.where(ok[:, None], q, 0).astype(np.float64) * 65536.0).astype(np.int64)
    Qx, Qy, Z = Q[:, 0], Q[:, 1], Q[:, 2]
    ok &= Z >= k["NEAR"]
    d = 256 * np.maximum(Z, 1)
    nu = k["FX"] * Qx + (k["CX"] + 128) * Z
    nv = k["FY"] * Qy + (k["CY"] + 128) * Z
    ok &= (nu >= 0) & (nu < frame.width * d) & (nv >= 0) & (nv < frame.height * d)
    nu, nv = np.where(ok, nu, 0), np.where(ok, nv, 0)
    return ok, Z, nu // d, nv // d


def mirror_observed(frame, image, uc, vc):
    """-> (valid bool, Zobs int64) of the pixels (uc, vc) by haf_frame's depth rule"""
    raw = np.asarray(image)[vc, uc]
    scale = F(frame.depth_scale)
    with np.errstate(all="ignore"):
        if raw.dtype == np.uint16:
            z = raw.astype(F) * scale
            ok = raw != 0
        else:
            z = raw * scale
            ok = np.isfinite(raw) & (raw > 0)
        ok &= np.isfinite(z)
        if frame.min_depth > 0:
            ok &= ~(z < F(frame.min_depth))
        if frame.max_depth > 0:
            ok &= ~(z > F(frame.max_depth))
        zobs = np.where(z > F(16.0), FAR_WORD, np.rint(np.where(ok, z, 0).astype(np.float64) * 65536.0)).astype(np.int64)
    return ok, zobs


def classify(k, Qz, zobs):
    tol = k["TA"] + ((k["TR"] * zobs) >> 16)
    D = Qz - zobs
    return np.where(D > tol, HIDDEN, np.where(D < -tol, FREE, HIT))


def mirror_view_states(frame, image, params, Pq):
    ok, Qz, uc, vc = mirror_project(frame, params, Pq)
    valid, zobs = mirror_observed(frame, image, uc, vc)
    return np.where(ok & valid, classify(view_constants(frame, params), Qz, zobs), UNSEEN)


def mirror_space(views, grasps, grip, params):
    """haf_check_space_ref by the header's table -> (SPACE_DTYPE [n], order, info, states uint8 [n, N])"""
    lat = mirror_lattice(grip, params)
    N = lat["N"]
    rows, states = np.zeros(len(grasps), capi.SPACE_DTYPE), np.zeros((len(grasps), N), np.uint8)
    for i, grasp in enumerate(grasps):
        words = cc.mirror_words(grasp)
        if words is None:
            rows[i]["clear"] = -1
            continue
        Pq = mirror_points(words, lat["stu"])
        st = np.zeros(N, np.int64)
        for frame, image in views:
            st = np.maximum(st, mirror_view_states(frame, image, params, Pq))
        states[i] = st
        n = np.zeros((4, 4), np.int64)
        np.add.at(n, (lat["region"], st), 1)
        rows[i]["n"] = n
        hit, unknown = int(n[1:, HIT].sum()), int(n[1:, HIDDEN].sum() + n[1:, UNSEEN].sum())
        rows[i]["clear"] = int(hit <= params.max_hit and unknown <= params.max_unknown and int(n[BETWEEN, HIT]) >= params.min_between_hit)
    info = dict(step=lat["S"], n=[list(map(int, r)) for r in lat["n"]], n_samples=N)
    return rows, np.flatnonzero(rows["clear"] == 1).astype(np.int32), info, states


def same(got, want, where=""):
    """two (rows, order, info, states) results agree in every word"""
    assert got[0].dtype == want[0].dtype == capi.SPACE_DTYPE and got[0].shape == want[0].shape, where
    for f in ("clear", "n", "reserved"):
        bad = np.flatnonzero((got[0][f] != want[0][f]).reshape(len(got[0]), -1).any(axis=1))
        assert bad.size == 0, (where, f, bad[:5], got[0][f][bad[:5]], want[0][f][bad[:5]])
    assert got[1].tolist() == want[1].tolist(), (where, "order")
    assert got[2] == want[2], (where, "info", got[2], want[2])
    assert got[3].shape == want[3].shape and got[3].dtype == np.uint8, (where, got[3].shape, want[3].shape)
    bad = np.argwhere(got[3] != want[3])
    assert bad.size == 0, (where, "states", bad[:5], [(int(got[3][tuple(b)]), int(want[3][tuple(b)])) for b in bad[:5]])


# ---- what the cases are made of -------------------------------------------------------------------------------------------------------

def case_of(name, views, grasps, gripper=None, params=None, candidates=False, expect=(), merges=()):
    return dict(name=name, views=views, grasps=grasps, gripper=dict(gripper or {}), params=dict(params or {}), candidates=candidates,
                expect=list(expect), merges=list(merges))


def grasp_arg(case):
    """the case's grasps as the entry points take them: dicts (a haf_grasp_output[]) or a haf_grasp_candidate[] with its own stride"""
    if not case["candidates"]:
        return case["grasps"]
    arr = (capi.GraspCandidate * len(case["grasps"]))()
    for o, g in zip(arr, case["grasps"]):
        for f in cc.POSE_FIELDS:
            setattr(o.grasp, f, (C.c_double * 3)(*[float(x) for x in g[f]]))
        o.run_length, o.h_locmax = 7, 0.25                # (never read: what lies between two grasps)
    return arr


def run(call, case, states=True):
    """call: capi.check_space_ref or an engine's check_space"""
    return call([f for f, _ in case["views"]], grasp_arg(case), capi.gripper(**case["gripper"]), capi.space_params(**case["params"]), states=states)


def mirror(case):
    return mirror_space(case["views"], case["grasps"], capi.gripper(**case["gripper"]), capi.space_params(**case["params"]))


def padded_image(h, w, dtype, pad):
    wide = np.zeros((h, w + pad), dtype)
    if pad:
        wide[:, w:] = 7                                   # a valid depth: a reader that strays into the padding sees a surface
    return wide[:, :w]


def look_at(eye, target, spin=0.0):
    """sensor_to_base (3 x 4) of a camera at `eye` whose z axis points at `target`, turned by `spin` about it"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    side = np.cross(z, [0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0])
    x = side / np.linalg.norm(side)
    y = np.cross(z, x)
    c, s = np.cos(spin), np.sin(spin)
    x, y = c * x + s * y, -s * x + c * y
    return np.concatenate([np.stack([x, y, z], axis=1), eye[:, None]], axis=1)


def scene_view(kind, w, h, pose, rng, pad=0, holes=True, zoom=0.9):
    """transfer_cases' random depth scene (a sloped far plane, near boxes) as a view of the given kind under `pose`"""
    z = tc.scene_depth(w, h, rng)
    k = dict(fx=zoom * max(w, 2), fy=zoom * max(w, 2), cx=(w - 1) / 2.0, cy=(h - 1) / 2.0)
    hole = (rng.random((h, w)) < 0.08) if holes else np.zeros((h, w), bool)
    if kind == "u16":
        img = padded_image(h, w, np.uint16, pad)
        img[:] = np.rint(z * 1000.0).astype(np.uint16)
        img[hole] = 0
    else:
        img = padded_image(h, w, F, pad)
        img[:] = z.astype(F)
        img[hole] = rng.choice(np.array([np.nan, 0.0, -1.0, np.inf], F), size=int(hole.sum()))
    return capi.depth_frame(img, sensor_to_base=pose, **k), img


# ---- set 1: boundaries, built from the mirror -----------------------------------------------------------------------------------------

EXACT_GRASP = cc.grasp_of((0.0, 0.0, 0.5), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0))      # axis words and Qz exact under the identity pose
DELTAS = ("hidden_edge", "near_hit", "exact", "far_hit", "free_edge", "invalid")


def solve_pixel(k, Qz, what):
    """the observed word that puts a sample of depth word Qz on the wanted side of a threshold -> (Zobs, the state it must give)"""
    if what == "exact":
        return Qz, HIT
    if what == "invalid":
        return 0, UNSEEN
    if k["TR"] == 0:
        tol = k["TA"]
        return {"hidden_edge": (Qz - tol - 1, HIDDEN), "near_hit": (Qz - tol, HIT), "far_hit": (Qz + tol, HIT), "free_edge": (Qz + tol + 1, FREE)}[what]
    tol_of = lambda z: k["TA"] + ((k["TR"] * z) >> 16)    # noqa: E731
    if what in ("far_hit", "free_edge"):                  # the largest Zobs with Zobs - Qz <= tol(Zobs), and the next one
        z = Qz
        while (z + 1) - Qz <= tol_of(z + 1):
            z += 1
        return (z, HIT) if what == "far_hit" else (z + 1, FREE)
    z = Qz                                                # the smallest Zobs with Qz - Zobs <= tol(Zobs), and the one before
    while Qz - (z - 1) <= tol_of(z - 1):
        z -= 1
    return (z, HIT) if what == "near_hit" else (z - 1, HIDDEN)


def exact_view(dtype, w=320, h=240, f=1000.0, pad=3):
    img = padded_image(h, w, dtype, pad)
    return capi.depth_frame(img, f, f, (w - 1) / 2.0 + 0.5, (h - 1) / 2.0 + 0.5, depth_scale=EXACT_SCALE, sensor_to_base=IDENTITY), img


def distinct_samples(views, params, Pq, count, among=None, taken=None):
    """`count` samples (of `among`, default all) that project inside every view and fall on pixels of their own in each -- none of
    `taken`, one set of pixels per view, which grows -- spread over the lattice"""
    chosen = []
    taken = [set() for _ in views] if taken is None else taken
    proj = [mirror_project(f, params, Pq) for f, _ in views]
    among = np.arange(len(Pq)) if among is None else np.asarray(among)
    order = among[np.random.default_rng(len(Pq)).permutation(len(among))]
    for j in order:
        if not all(p[0][j] for p in proj):
            continue
        px = [(int(p[2][j]), int(p[3][j])) for p in proj]
        if any(x in t for x, t in zip(px, taken)):
            continue
        for x, t in zip(px, taken):
            t.add(x)
        chosen.append(int(j))
        if len(chosen) == count:
            break
    assert len(chosen) == count, "the intrinsics are too small for that many samples on pixels of their own"
    return chosen, proj


def boundary_case(dtype, tol_rel):
    """every DELTA in every region: each chosen sample's pixel holds the word that puts it on one side of one threshold"""
    params_kw = dict(sample_step=0.01, tol_rel=tol_rel)
    params, grip = capi.space_params(**params_kw), capi.gripper()
    frame, img = exact_view(dtype)
    img[:] = 60000 if dtype == np.uint16 else F(60000.0)
    lat = mirror_lattice(grip, params)
    Pq = mirror_points(cc.mirror_words(EXACT_GRASP), lat["stu"])
    k = view_constants(frame, params)
    chosen, taken = [], [set()]
    for r in range(4):                                    # every DELTA in every region
        got, proj = distinct_samples([(frame, img)], params, Pq, len(DELTAS), np.flatnonzero(lat["region"] == r), taken)
        chosen += got
    expect, per_region = [], {r: 0 for r in range(4)}
    for j in chosen:
        r = int(lat["region"][j])
        what = DELTAS[per_region[r] % len(DELTAS)]
        per_region[r] += 1
        zobs, state = solve_pixel(k, int(proj[0][1][j]), what)
        assert 0 <= zobs < 65536
        img[int(proj[0][3][j]), int(proj[0][2][j])] = zobs
        expect.append((0, j, state, what))
    assert all(v >= len(DELTAS) for v in per_region.values()), per_region
    name = "boundary_%s_rel%g" % (np.dtype(dtype).name, tol_rel)
    return case_of(name, [(frame, img)], [EXACT_GRASP], {}, params_kw, expect=[(g, j, s) for g, j, s, _ in expect]), expect


def single_sample_case(name, Z, ox_words, fx, cx, width, pixel, state, axis="u", tol_rel=0.0):
    """a lattice of ONE sample whose depth word under the identity pose is exactly Z and whose x (or y) word is 16 * ox_words, in a
    width x 1 (or 1 x width) float view whose every pixel holds `pixel`"""
    oz, rem = Z // 16, Z % 16
    a, b = (1 << 20) + 2048 * rem, 1 << 20                # the sample's u = -1024 rem words: Pq_z = 16 oz + rem (approach vector -z)
    grip = dict(opening=0.02, finger_thickness=0.0, finger_breadth=0.02, tip_depth=a / cc.ONE, finger_length=(a + b) / cc.ONE, palm_height=0.0)
    side = ox_words / 4096.0
    origin = (side, 0.0, oz / 4096.0) if axis == "u" else (0.0, side, oz / 4096.0)
    grasp = cc.grasp_of(origin, (0.0, 0.0, -1.0), (1.0, 0.0, 0.0))
    shape = (1, width) if axis == "u" else (width, 1)
    img = np.full(shape, pixel, F)
    kw = dict(fx=fx, fy=1.0, cx=cx, cy=0.0) if axis == "u" else dict(fx=1.0, fy=fx, cx=0.0, cy=cx)
    frame = capi.depth_frame(img, depth_scale=EXACT_SCALE, sensor_to_base=IDENTITY, **kw)
    params_kw = dict(sample_step=1.0, tol_rel=tol_rel)
    lat = mirror_lattice(capi.gripper(**grip), capi.space_params(**params_kw))
    assert lat["N"] == 1
    Pq = mirror_points(cc.mirror_words(grasp), lat["stu"])
    assert int(Pq[0, 2]) == Z and int(Pq[0, 0 if axis == "u" else 1]) == 16 * ox_words, (Pq, Z)
    return case_of(name, [(frame, img)], [grasp], grip, params_kw, expect=[(0, 0, state)])


def edge_cases():
    """nu (nv) exactly at width d - 1 and at width d; Z = NEAR - 1 and Z = NEAR; a valid z above 16 m"""
    out = []
    near = tc.rne(float(F(0.05)) * 65536.0)
    ta = tc.rne(float(F(0.004)) * 65536.0)
    for axis in ("u", "v"):
        # FX = 256, CX = 256 width - 129: nu = 256 Qx + (256 width - 1) Z, so nu = width d - 1 when 256 Qx = Z - 1 and width d when 256 Qx = Z
        for width in (1, 3):
            cx = width - 129.0 / 256.0
            ox = 100
            out.append(single_sample_case("edge_%s_w%d_last" % (axis, width), 256 * 16 * ox + 1, ox, 1.0, cx, width, F(256 * 16 * ox + 1), HIT, axis))
            out.append(single_sample_case("edge_%s_w%d_outside" % (axis, width), 256 * 16 * ox, ox, 1.0, cx, width, F(256 * 16 * ox), UNSEEN, axis))
    out.append(single_sample_case("near_minus_one", near - 1, 0, 1.0, 1.0, 3, F(near - 1), UNSEEN))
    out.append(single_sample_case("near_exact", near, 0, 1.0, 1.0, 3, F(near), HIT))
    # the pixel says 16.6 m: counted as 16 m, a sample at 16 m - TA is a HIT and one word nearer is FREE
    out.append(single_sample_case("above_16m_hit", FAR_WORD - ta, 0, 1.0, 1.0, 3, F(FAR_WORD + 40000), HIT))
    out.append(single_sample_case("above_16m_free", FAR_WORD - ta - 1, 0, 1.0, 1.0, 3, F(FAR_WORD + 40000), FREE))
    return out


# ---- set 2: the axis sets and their mirror images under oblique views ------------------------------------------------------------------

def axis_cases():
    out = []
    for i, (name, o_words, approach, closing) in enumerate(cc.AXIS_SETS):
        rng = np.random.default_rng([20251020, i])
        origin = np.array(o_words, np.float64) / 4096.0
        grasp = cc.grasp_of(origin, approach, closing)
        views = [scene_view("u16", 64, 48, look_at(origin + np.array([0.35, -0.3, 0.5]), origin, 0.4), rng, pad=2),
                 scene_view("f32", 57, 41, look_at(origin + np.array([-0.45, 0.2, 0.48]), origin + 0.01, -1.1), rng, pad=1)]
        out.append(case_of("axes_" + name, views, [grasp, cc.flipped(grasp)], {}, dict(max_hit=40, max_unknown=4000)))
    return out


# ---- set 3: sizes ----------------------------------------------------------------------------------------------------------------------

STEP = 2.0 ** -10                     # its word is 65536: a box of n steps has exactly n samples along that axis


def between_only(ns, nt, nu, **more):
    """a gripper whose only region with samples is `between`, ns x nt x nu of them at sample_step = STEP"""
    return dict(dict(opening=ns * STEP, finger_thickness=0.0, finger_breadth=nt * STEP, tip_depth=0.0, finger_length=nu * STEP, palm_height=0.0), **more)


SIZES = {1: (1, 1, 1), 63: (7, 3, 3), 64: (4, 4, 4), 65: (13, 5, 1), CHUNK - 1: (17, 5, 3), CHUNK: (8, 8, 4), CHUNK + 1: (257, 1, 1),
         capi.MAX_SPACE_SAMPLES: (64, 32, 32)}
OVER_CAP = between_only(64, 32, 32, palm_width=STEP / 2, palm_breadth=STEP / 2, palm_height=STEP / 2)      # the cap, and one palm sample


def size_cases():
    out = []
    rng = np.random.default_rng(20251021)
    origin = np.array([0.2, -0.1, 0.05])
    pose = look_at(origin + np.array([0.1, 0.25, 0.6]), origin, 0.2)
    view = scene_view("u16", 64, 48, pose, rng, pad=3)
    for n, dims in SIZES.items():
        grasps = cc.random_grasps(rng, [origin], 2 if n < 1000 else 1)
        out.append(case_of("samples_%d" % n, [view], grasps, between_only(*dims), dict(sample_step=STEP, max_unknown=n)))
    out.append(case_of("no_palm", [view], cc.random_grasps(rng, [origin], 3), dict(palm_height=0.0), dict(sample_step=0.01)))
    for n_g, cand in ((1, True), (2, False), (2, True), (257, False), (257, True)):
        out.append(case_of("grasps_%d_%s" % (n_g, "candidates" if cand else "outputs"), [view], cc.random_grasps(rng, [origin], n_g),
                           between_only(13, 5, 1, finger_thickness=2 * STEP), dict(sample_step=STEP, max_unknown=50), candidates=cand))
    for (w, h), kind, pad in (((1, 1), "f32", 0), ((1, 1), "u16", 2), ((7, 5), "u16", 1), ((7, 5), "f32", 3), ((64, 48), "f32", 5)):
        v = scene_view(kind, w, h, pose, rng, pad=pad, holes=w > 1, zoom=0.9 if w > 1 else 0.5)
        out.append(case_of("frame_%dx%d_%s_pad%d" % (w, h, kind, pad), [v], cc.random_grasps(rng, [origin], 3), {}, dict(sample_step=0.008)))
    shapes = [(64, 48, "u16", 2), (7, 5, "f32", 1), (33, 20, "u16", 0), (1, 1, "f32", 0), (40, 31, "f32", 3), (16, 16, "u16", 5),
              (64, 48, "f32", 0), (21, 9, "u16", 1)]
    many = []
    for i, (w, h, kind, pad) in enumerate(shapes):
        eye = origin + np.array([0.5 * np.cos(0.8 * i), 0.5 * np.sin(0.8 * i), 0.45 + 0.02 * i])
        many.append(scene_view(kind, w, h, look_at(eye, origin, 0.3 * i), rng, pad=pad, zoom=0.8))
    for n_v in (1, 2, 8):
        out.append(case_of("views_%d" % n_v, many[:n_v], cc.random_grasps(rng, [origin], 5), {}, dict(sample_step=0.008, max_unknown=30)))
    return out


# ---- set 4: two views that disagree on purpose ----------------------------------------------------------------------------------------

MERGE_RULES = {"hit_over_free": (HIT, FREE), "free_over_hidden": (FREE, HIDDEN), "hidden_over_unseen": (HIDDEN, UNSEEN)}
STATE_WORD = {HIT: "exact", FREE: "free_edge", HIDDEN: "hidden_edge", UNSEEN: "invalid"}


def merge_case():
    params_kw = dict(sample_step=0.01, tol_rel=0.0)
    params, grip = capi.space_params(**params_kw), capi.gripper()
    views = [exact_view(np.uint16), exact_view(np.float32, w=300, h=200, f=900.0, pad=0)]
    for _, img in views:
        img[:] = 60000
    lat = mirror_lattice(grip, params)
    Pq = mirror_points(cc.mirror_words(EXACT_GRASP), lat["stu"])
    chosen, proj = distinct_samples(views, params, Pq, 2 * len(MERGE_RULES))
    expect = []
    for i, j in enumerate(chosen):
        rule = list(MERGE_RULES)[i % len(MERGE_RULES)]
        wins, loses = MERGE_RULES[rule]
        for v, state in enumerate((wins, loses) if i < len(MERGE_RULES) else (loses, wins)):      # either view may hold the winner
            zobs, got = solve_pixel(view_constants(views[v][0], params), int(proj[v][1][j]), STATE_WORD[state])
            assert got == state
            views[v][1][int(proj[v][3][j]), int(proj[v][2][j])] = zobs
        expect.append((0, j, wins))
    return case_of("merge_two_views", views, [EXACT_GRASP], {}, params_kw, expect=expect, merges=list(MERGE_RULES))


# ---- sets 5 and 6: void grasps; the three thresholds of `clear` ----------------------------------------------------------------------

NOTHING_FOUND = dict(grasp_point1=(0.0, 0.0, 0.0), grasp_point2=(0.0, 0.0, 0.0), averaged_grasp_point=(0.0, 0.0, 0.0), approach_vector=(0.0, 0.0, 0.0))


def void_cases():
    rng = np.random.default_rng(20251022)
    origin = np.array([0.0, 0.0, 0.1])
    view = scene_view("u16", 40, 30, look_at((0.1, 0.1, 0.8), origin), rng)
    ok = cc.random_grasps(rng, [origin], 4)
    voids = [NOTHING_FOUND, cc.grasp_of(origin, (0, 0, 1), (0, 0, 1)), dict(ok[0], grasp_point2=(0.1, float("nan"), 0.1)),
             cc.grasp_of((0.1, 16.5, 0.1), (0, 0, 1), (1, 0, 0))]
    kw = dict(sample_step=0.01, max_hit=10 ** 6, max_unknown=10 ** 6, min_between_hit=0)
    return [case_of("voids_amid_valid", [view], [ok[0], voids[0], voids[1], ok[1], voids[2], ok[2], voids[3], ok[3]], {}, kw),
            case_of("only_void", [view], [NOTHING_FOUND], {}, kw)]


def threshold_cases():
    """one scene, and for each of max_hit, max_unknown and min_between_hit the value that just admits a grasp and the one that just does
    not, all else wide open -> [(field, case that admits, case that refuses)]"""
    rng = np.random.default_rng(20251023)
    origin = np.array([0.0, 0.0, 0.05])
    view = scene_view("f32", 48, 36, look_at((0.05, -0.1, 0.72), origin), rng)
    hole = ~(view[1] > 0)
    view[1][:] = (0.60 + 0.16 * np.arange(48) / 47.0).astype(F)      # a slope through the gripper's depths: hidden, hit and free samples
    view[1][hole] = 0
    grasp = cc.grasp_of(origin, (0.1, 0.0, 1.0), (1.0, 0.2, 0.0))
    wide = dict(sample_step=0.008, max_hit=10 ** 6, max_unknown=10 ** 6, min_between_hit=0)
    n = mirror_space([view], [grasp], capi.gripper(), capi.space_params(**wide))[0][0]["n"]
    hit, unknown, between = int(n[1:, HIT].sum()), int(n[1:, HIDDEN].sum() + n[1:, UNSEEN].sum()), int(n[BETWEEN, HIT])
    assert hit > 0 and unknown > 0 and between > 0, (hit, unknown, between)
    out = []
    for field, yes, no in (("max_hit", hit, hit - 1), ("max_unknown", unknown, unknown - 1), ("min_between_hit", between, between + 1)):
        out.append((field, case_of("clear_by_%s" % field, [view], [grasp], {}, dict(wide, **{field: yes})),
                    case_of("refused_by_%s" % field, [view], [grasp], {}, dict(wide, **{field: no}))))
    return out


def cases():
    out = [boundary_case(dt, rel)[0] for dt in (np.uint16, np.float32) for rel in (0.0, 0.002)] + edge_cases() + axis_cases() + size_cases()
    out += [merge_case()] + void_cases()
    for _, yes, no in threshold_cases():
        out += [yes, no]
    return out


# ---- the occluded finger --------------------------------------------------------------------------------------------------------------

BOX = ((-0.03, -0.05, 0.0), (0.03, 0.05, 0.08))          # on the plane z = 0 of the base frame


def render(pose, w, h, f):
    """the depth image, metres along the camera's axis, of BOX on the plane z = 0 seen from `pose` (sensor_to_base, 3 x 4)"""
    v, u = np.mgrid[0:h, 0:w]
    d_cam = np.stack([(u - (w - 1) / 2.0) / f, (v - (h - 1) / 2.0) / f, np.ones((h, w))], axis=2)
    d = d_cam @ pose[:, :3].T
    eye = pose[:, 3]
    with np.errstate(all="ignore"):
        t = np.where(d[..., 2] < 0, -eye[2] / d[..., 2], np.inf)
        lo, hi = (np.array(BOX[0]) - eye) / d, (np.array(BOX[1]) - eye) / d
        t_in, t_out = np.minimum(lo, hi).max(axis=2), np.maximum(lo, hi).min(axis=2)
    box = (t_in <= t_out) & (t_in > 0)
    return np.where(box, np.minimum(t_in, t), t)


def occluded_scene():
    """-> (view from +x, view from -x, the grasp): a top-down grasp across the box, finger 0 on the -x side, behind the box as the first
    camera sees it.  640 x 480 would do no more: 160 x 120 U16 millimetres"""
    w, h, f = 160, 120, 150.0
    views = []
    for side in (1.0, -1.0):
        pose = look_at((0.5 * side, 0.0, 0.5), (0.0, 0.0, 0.04))
        z = render(pose, w, h, f)
        img = np.where(np.isfinite(z), np.rint(z * 1000.0), 0).astype(np.uint16)
        views.append((capi.depth_frame(img, f, f, (w - 1) / 2.0, (h - 1) / 2.0, sensor_to_base=pose), img))
    grasp = cc.grasp_of((0.0, 0.0, 0.06), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    return views[0], views[1], grasp
