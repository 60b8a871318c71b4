"""Cases of haf_transfer_labels (include/hafgrasp.h; csrc/transfer_rules.h), shared by test_transfer_cpu.py and test_transfer_gpu.py,
and `restate`: steps 1-6 of the header written once more, independently of the library -- numpy float32 for the two transforms, one
rounded operation per step, Python integers for everything behind them.

A case is (name, frame, image, camera, cam_labels, n_labels, params kw).  The depth images start one element past an aligned address,
so that a device copy's pixel groups are not 16-byte aligned; the wide ones are views into padded arrays."""
import numpy as np

from haf_grasping_amd import capi

F = np.float32
INT32_MAX = 2 ** 31 - 1
# a depth camera 0.8 m above the table, looking down; the label camera 6 cm to its side and a little turned
DEPTH_POSE = np.array([[1, 0, 0, 0.10], [0, -1, 0, 0.20], [0, 0, -1, 0.80]], np.float64)


def label_pose(baseline=0.06, yaw=0.03):
    c, s = np.cos(yaw), np.sin(yaw)
    turn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    m = DEPTH_POSE.copy()
    m[:, :3] = DEPTH_POSE[:, :3] @ turn
    m[:, 3] += DEPTH_POSE[:, :3] @ np.array([baseline, 0.01, 0.0])
    return m


def inverse_of(sensor_to_base):
    """base -> camera of a camera's sensor_to_base, in float64, rounded once (numpy's inverse, not the library's)"""
    m = np.eye(4)
    m[:3] = np.asarray(sensor_to_base, np.float64).reshape(3, 4)
    return np.linalg.inv(m)[:3].astype(F)


def offset_array(shape, dtype, pad=0):
    """a zeroed [h, w(, 3)] array whose first element lies one element past an aligned address; pad: unused elements behind every row"""
    h, w = shape[:2]
    tail = shape[2:]
    per = int(np.prod(tail)) if tail else 1
    flat = np.zeros(h * (w + pad) * per + 1 + 8, dtype)
    return flat[1:1 + h * (w + pad) * per].reshape((h, w + pad) + tail)[:, :w]


def scene_depth(w, h, rng, near_share=0.35):
    """metres [h, w]: a far plane with a slope, near boxes in front of it, a few holes"""
    v, u = np.mgrid[0:h, 0:w]
    z = 0.78 + 0.02 * (u / max(1, w - 1)) + 0.01 * (v / max(1, h - 1))
    for _ in range(3):
        u0, v0 = rng.integers(0, w), rng.integers(0, h)
        bw, bh = max(1, int(w * near_share * rng.random()) + 1), max(1, int(h * near_share * rng.random()) + 1)
        z[v0:v0 + bh, u0:u0 + bw] = 0.55 + 0.1 * rng.random()
    return z


def depth_case_frame(kind, w, h, rng, pad=0, holes=True):
    """-> (frame, image) of the scene under DEPTH_POSE with intrinsics that fit the size; holes: zero / NaN / negative samples"""
    z = scene_depth(w, h, rng)
    k = dict(fx=0.82 * max(w, 2), fy=0.82 * max(w, 2), cx=(w - 1) / 2.0, cy=(h - 1) / 2.0)
    hole = (rng.random((h, w)) < 0.08) if holes else np.zeros((h, w), bool)
    if kind == capi.FRAME_DEPTH_U16:
        img = offset_array((h, w), np.uint16, pad)
        img[:] = np.rint(z * 1000.0).astype(np.uint16)
        img[hole] = 0
        return capi.depth_frame(img, sensor_to_base=DEPTH_POSE, **k), img
    if kind == capi.FRAME_DEPTH_F32:
        img = offset_array((h, w), F, pad)
        img[:] = z.astype(F)
        img[hole] = rng.choice(np.array([np.nan, 0.0, -1.0, np.inf], F), size=int(hole.sum()))
        return capi.depth_frame(img, sensor_to_base=DEPTH_POSE, **k), img
    img = offset_array((h, w, 3), F, pad)
    v, u = np.mgrid[0:h, 0:w]
    img[..., 0] = ((u - k["cx"]) / k["fx"] * z).astype(F)
    img[..., 1] = ((v - k["cy"]) / k["fy"] * z).astype(F)
    img[..., 2] = z.astype(F)
    img[hole] = np.nan
    return capi.xyz_frame(img, sensor_to_base=DEPTH_POSE), img


def label_camera(wc, hc, pose=None, zoom=0.8):
    pose = label_pose() if pose is None else pose
    return capi.camera(wc, hc, zoom * max(wc, 2), zoom * max(wc, 2), (wc - 1) / 2.0, (hc - 1) / 2.0, base_to_camera=inverse_of(pose))


def label_image(wc, hc, dtype, rng, n_labels, pad=0):
    """blocks of labels 0..n_labels, and some values above n_labels, which count as background"""
    wide = np.zeros((hc, wc + pad), dtype)
    img = wide[:, :wc]
    bw, bh = max(1, wc // 5), max(1, hc // 4)
    top = min(n_labels + 3, np.iinfo(dtype).max)
    for v0 in range(0, hc, bh):
        for u0 in range(0, wc, bw):
            img[v0:v0 + bh, u0:u0 + bw] = rng.integers(0, top + 1)
    return img


KINDS = (capi.FRAME_DEPTH_U16, capi.FRAME_DEPTH_F32, capi.FRAME_XYZ_F32)
KIND_NAMES = {capi.FRAME_DEPTH_U16: "u16", capi.FRAME_DEPTH_F32: "f32", capi.FRAME_XYZ_F32: "xyz"}
CAMERA_SIZES = ((1, 1), (2, 2), (5, 3), (17, 9), (64, 48))


def size_cases():
    """depth 1 x 1 and widths 1..17 at height 3, over every camera size, splat and frame kind in turn"""
    rng = np.random.default_rng(2024)
    out = []
    for j, (w, h) in enumerate([(1, 1)] + [(w, 3) for w in range(1, 18)]):
        kind = KINDS[j % 3]
        wc, hc = CAMERA_SIZES[j % len(CAMERA_SIZES)]
        frame, image = depth_case_frame(kind, w, h, rng, holes=w > 2)
        n_labels = 7
        labels = label_image(wc, hc, np.uint8 if j % 2 else np.uint16, rng, n_labels)
        out.append(("size_%dx%d_%s_cam%dx%d_s%d" % (w, h, KIND_NAMES[kind], wc, hc, j % 3), frame, image, label_camera(wc, hc), labels, n_labels,
                    dict(splat=j % 3)))
    return out


def kind_cases():
    """all three kinds, uint8 and uint16 camera images, padded strides on both sides, a camera of another resolution"""
    rng = np.random.default_rng(77)
    out = []
    for kind in KINDS:
        for j, (cdt, n_labels) in enumerate(((np.uint8, 200), (np.uint16, 300))):
            frame, image = depth_case_frame(kind, 23, 11, rng, pad=3)
            labels = label_image(31, 17, cdt, rng, n_labels, pad=5)
            out.append(("kind_%s_%s" % (KIND_NAMES[kind], np.dtype(cdt).name), frame, image, label_camera(31, 17), labels, n_labels,
                        dict(splat=1 + j)))
    return out


def hostile_case():
    """an XYZ frame under the identity pose into a camera under the identity pose, so that q = p in every bit: points that are not finite,
    behind and on the camera plane, nearer than near_m, at exactly 16 m and just beyond, on the last column and just outside it, above the
    first row and just outside it, and two pixels with equal Qz on one camera pixel"""
    pts = [
        # 0-5: not finite, behind the plane, on it, nearer than near_m, at near_m (pixel (2, 0): x / z = -0.375, y / z = -0.625)
        (np.nan, 0.0, 1.0), (0.0, np.inf, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.04), (-0.375 * 0.05, -0.625 * 0.05, 0.05),
        # 6-10: 16 m deep at pixel (5, 0); 16 m deep and 16 m to the side (outside the image); just beyond 16 m in z, in x; -16 in x and y
        (6.0, -10.0, 16.0), (16.0, 0.0, 16.0), (0.0, 0.0, 16.000002), (16.000002, 0.0, 1.0), (-16.0, -16.0, 16.0),
        # 11-15: the last column (7, 3), just outside it, the first column (0, 3), just outside it
        (0.9974, 0.0, 1.0), (1.0, 0.0, 1.0), (0.99999994, 0.0, 1.0), (-1.0, 0.0, 1.0), (-1.00002, 0.0, 1.0),
        # 16-19: the first row (4, 0), just outside it, just outside the last row
        (0.0, -0.75, 1.0), (0.0, -0.75002, 1.0), (0.0, 0.74999994, 1.0), (0.0, 0.75, 1.0),
        # 20-22: equal Qz on pixel (4, 3); 23-26: pixel (2, 4): the nearest, a hidden one, one within the tolerance, one just beyond it
        (0.1, 0.1, 2.0), (0.1001, 0.1001, 2.0), (0.1, 0.1, 2.0000002),
        (-0.375, 0.375, 1.0), (-0.375 * 1.5, 0.375 * 1.5, 1.5), (-0.375 * 1.004, 0.375 * 1.004, 1.004), (-0.375 * 1.03, 0.375 * 1.03, 1.03),
    ]
    w, h = 9, 3
    img = offset_array((h, w, 3), F)
    img.reshape(-1, 3)[:len(pts)] = np.array(pts, F)
    assert len(pts) == w * h
    frame = capi.xyz_frame(img)
    cam = capi.camera(8, 6, 4.0, 4.0, 3.5, 2.5)
    labels = (np.arange(48, dtype=np.uint16).reshape(6, 8) % 5 + 1).astype(np.uint16)
    return ("hostile_identity", frame, img, cam, labels, 5, dict(splat=0, near_m=0.05))


def contention_cases():
    """64 x 48 into a 2 x 2 camera with fx = fy = 1: every point competes for at most four words; 64 x 48 into 64 x 48 with splat 2; a
    window larger than the camera image"""
    rng = np.random.default_rng(5)
    out = []
    frame, image = depth_case_frame(capi.FRAME_DEPTH_U16, 64, 48, rng)
    cam = capi.camera(2, 2, 1.0, 1.0, 0.5, 0.5, base_to_camera=inverse_of(label_pose()))
    out.append(("contention_2x2", frame, image, cam, np.array([[1, 2], [3, 4]], np.uint8), 4, dict(splat=0)))
    frame, image = depth_case_frame(capi.FRAME_DEPTH_F32, 64, 48, rng)
    out.append(("contention_splat2", frame, image, label_camera(64, 48), label_image(64, 48, np.uint16, rng, 40), 40, dict(splat=2)))
    frame, image = depth_case_frame(capi.FRAME_XYZ_F32, 64, 48, rng)
    out.append(("window_over_image", frame, image, label_camera(3, 2, zoom=0.4), label_image(3, 2, np.uint8, rng, 3), 3, dict(splat=2)))
    return out


def cases():
    return size_cases() + kind_cases() + [hostile_case()] + contention_cases()


def occlusion_scene(w=48, h=36):
    """a far plane at 0.8 m and a near box at 0.5 m in its middle, seen by a depth camera looking down and by a label camera 12 cm to its
    side -> (frame, image, camera, cam_labels, the box's depth pixels); the label image says 1 where the label camera sees the box,
    painted generously, 0 elsewhere"""
    img = offset_array((h, w), np.uint16)
    img[:] = 800
    box = np.zeros((h, w), bool)
    box[h // 3:2 * h // 3, w // 3:2 * w // 3] = True
    img[box] = 500
    k = dict(fx=0.9 * w, fy=0.9 * w, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0)
    frame = capi.depth_frame(img, sensor_to_base=DEPTH_POSE, **k)
    side = DEPTH_POSE.copy()
    side[:, 3] += DEPTH_POSE[:, :3] @ np.array([0.12, 0.0, 0.0])
    cam = capi.camera(w, h, k["fx"], k["fy"], k["cx"], k["cy"], base_to_camera=inverse_of(side))
    # where the box's top projects in the label camera: the box's pixels shifted by fx * baseline / depth
    shift = int(round(k["fx"] * 0.12 / 0.5))
    labels = np.zeros((h, w), np.uint8)
    labels[h // 3 - 1:2 * h // 3 + 1, max(0, w // 3 - shift - 1):max(0, 2 * w // 3 - shift + 1)] = 1
    return frame, img, cam, labels, box


# ---- the independent restatement ----------------------------------------------------------------------------------------------------

def rne(x):
    """round to nearest even of a Python float (exact here: every argument is a float32 times a power of two)"""
    return int(round(x))


def constants(cam, p):
    near = max(1, rne(float(F(p.near_m)) * 65536.0))
    ta = min(rne(float(F(p.tol_abs)) * 65536.0), INT32_MAX)
    return dict(FX=rne(float(F(cam.fx)) * 256.0), FY=rne(float(F(cam.fy)) * 256.0), CX=rne(float(F(cam.cx)) * 256.0),
                CY=rne(float(F(cam.cy)) * 256.0), NEAR=near, TA=ta, TR=rne(float(F(p.tol_rel)) * 65536.0))


def restate(frame, cam, cam_labels, n_labels, p):
    """-> (labels: int64 [height, width], stats: five ints, Z: int64 [cam.height, cam.width])"""
    pts = capi.frame_points(frame)                        # step 1: haf_frame_points' words
    m = np.array(list(cam.base_to_camera), F).reshape(3, 4)
    with np.errstate(all="ignore"):
        q = np.stack([((m[r, 0] * pts[:, 0] + m[r, 1] * pts[:, 1]) + m[r, 2] * pts[:, 2]) + m[r, 3] for r in range(3)], axis=1)
    assert q.dtype == F
    k = constants(cam, p)
    wc, hc, splat = cam.width, cam.height, p.splat
    Z = [[INT32_MAX] * wc for _ in range(hc)]
    proj = {}
    stats = [len(pts), 0, 0, 0, 0]
    for i in range(len(pts)):
        if not (np.isfinite(pts[i]).all() and np.isfinite(q[i]).all() and (np.abs(q[i]) <= F(16.0)).all()):
            continue
        Qx, Qy, Qz = (rne(float(x) * 65536.0) for x in q[i])
        if Qz < k["NEAR"]:
            continue
        stats[1] += 1
        d = 256 * Qz
        nu = k["FX"] * Qx + (k["CX"] + 128) * Qz
        nv = k["FY"] * Qy + (k["CY"] + 128) * Qz
        if not (0 <= nu < wc * d and 0 <= nv < hc * d):
            continue
        stats[2] += 1
        uc, vc = nu // d, nv // d
        proj[i] = (Qz, uc, vc)
        for v in range(max(0, vc - splat), min(hc - 1, vc + splat) + 1):
            for u in range(max(0, uc - splat), min(wc - 1, uc + splat) + 1):
                Z[v][u] = min(Z[v][u], Qz)
    out = np.zeros(len(pts), np.int64)
    for i, (Qz, uc, vc) in proj.items():
        z = Z[vc][uc]
        assert z <= Qz
        if Qz - z <= k["TA"] + ((k["TR"] * z) >> 16):
            stats[3] += 1
            lab = int(cam_labels[vc, uc])
            out[i] = lab if lab <= n_labels else 0
    stats[4] = int((out != 0).sum())
    return out.reshape(frame.height, frame.width), stats, np.array(Z, np.int64).reshape(hc, wc)


def same(got, want):
    """(labels, stats, zbuffer) of one entry point against another's, or against restate's"""
    return (np.asarray(got[0]).astype(np.int64) == np.asarray(want[0]).astype(np.int64)).all() and list(got[1]) == list(want[1]) and \
        (np.asarray(got[2]).astype(np.int64) == np.asarray(want[2]).astype(np.int64)).all()
