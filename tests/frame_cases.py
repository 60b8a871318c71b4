"""Shared by tests/test_frames_cpu.py and tests/test_frames_gpu.py: an independent numpy-fp32 mirror of the arithmetic of haf_frame
(include/hafgrasp.h) and the frames both suites run it on.  numpy float32 arithmetic rounds every operation, so the mirror and
haf_frame_points must agree word for word; the device kernel must agree with haf_frame_points likewise."""
import ctypes as C

import numpy as np

from haf_grasping_amd import capi

F = np.float32
NAN_WORD = np.uint32(0x7FC00000)
SHAPES = [(1, 1), (7, 3), (61, 5), (640, 480)]          # (width, height); 61 x 5 carries row padding


def mirror_points(frame, image):
    """The header's arithmetic on `image` ([H, W] uint16 / float32, or [H, W, >= 3] float32) with `frame`'s parameters -> uint32 [H*W, 3]"""
    t = np.array(list(frame.sensor_to_base), dtype=F).reshape(3, 4)
    H, W = image.shape[:2]
    with np.errstate(all="ignore"):
        if frame.kind == capi.FRAME_XYZ_F32:
            xc, yc, z = (np.ascontiguousarray(image[:, :, k], dtype=F) for k in range(3))
            valid = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(z)
        else:
            scale, mn, mx = F(frame.depth_scale), F(frame.min_depth), F(frame.max_depth)
            if frame.kind == capi.FRAME_DEPTH_U16:
                valid = image != 0
                z = image.astype(F) * scale
            else:
                d = image.astype(F)
                valid = np.isfinite(d) & ~(d <= F(0))
                z = d * scale
            valid &= np.isfinite(z)
            if mn > 0:
                valid &= ~(z < mn)
            if mx > 0:
                valid &= ~(z > mx)
            ifx, ify = F(1) / F(frame.fx), F(1) / F(frame.fy)
            u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
            v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
            xc = ((u - F(frame.cx)) * ifx) * z
            yc = ((v - F(frame.cy)) * ify) * z
        out = np.empty((H, W, 3), np.uint32)
        for r in range(3):
            p = ((t[r, 0] * xc + t[r, 1] * yc) + t[r, 2] * z) + t[r, 3]
            assert p.dtype == F
            w = p.view(np.uint32).copy()
            w[np.isnan(p) | ~valid] = NAN_WORD
            out[:, :, r] = w
    return out.reshape(-1, 3)


def tilted_pose(rng):
    """a general rotation (three Euler angles) and a translation, as 12 floats"""
    a, b, c = rng.uniform(-np.pi, np.pi, 3)
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    m = np.concatenate([rz @ ry @ rx, rng.uniform(-1.5, 1.5, (3, 1))], axis=1)
    return m.astype(F).reshape(-1)


def padded(image, pad):
    """the same pixels as a view into an array whose rows are `pad` elements longer (row_stride_bytes > width * element size)"""
    wide = np.zeros((image.shape[0], image.shape[1] + pad) + image.shape[2:], image.dtype)
    if image.dtype == np.uint16:
        wide[:] = 0x5A5A
    else:
        wide[:] = 12345.0
    wide[:, :image.shape[1]] = image
    return wide[:, :image.shape[1]]


def _intrinsics(rng, w, h):
    return dict(fx=float(rng.uniform(300, 700)) * (-1 if rng.random() < 0.1 else 1), fy=float(rng.uniform(300, 700)),
                cx=float(rng.uniform(0, w)), cy=float(rng.uniform(0, h)))


def u16_image(rng, w, h):
    img = rng.integers(300, 4000, (h, w)).astype(np.uint16)
    img[rng.random((h, w)) < 0.3] = 0
    flat = img.reshape(-1)
    for k, v in enumerate((0, 1, 65535)):
        flat[(k * 7) % flat.size] = v                     # (a 1 x 1 frame ends up with 65535)
    return img


F32_SPECIALS = [np.nan, np.inf, -np.inf, -1.25, -0.0, 0.0, 1e-41, 1.4e-45, 3.0e38]


def f32_image(rng, w, h, limits=None):
    img = rng.uniform(0.3, 4.0, (h, w)).astype(F)
    img[rng.random((h, w)) < 0.2] = np.nan
    flat = img.reshape(-1)
    special = [F(x) for x in F32_SPECIALS]
    for lim in limits or ():
        lim = F(lim)
        special += [lim, np.nextafter(lim, F(0)), np.nextafter(lim, F(np.inf))]
    for k, v in enumerate(special):
        flat[(k * 5 + 1) % flat.size] = v
    return img


def xyz_image(rng, w, h, floats=3):
    img = rng.uniform(-2.0, 2.0, (h, w, floats)).astype(F)
    img[rng.random((h, w)) < 0.2] = np.nan
    flat = img.reshape(-1, floats)
    for k in range(3):                                    # one NaN component, each position once; an infinity
        flat[(k * 3 + 1) % flat.shape[0], :3] = rng.uniform(-1, 1, 3).astype(F)
        flat[(k * 3 + 1) % flat.shape[0], k] = np.nan
    flat[(11) % flat.shape[0], :3] = (F(0.5), F(np.inf), F(1.0))
    return img


def cases(seed=20240611):
    """-> list of (name, frame, image): every kind on every shape of SHAPES with random intrinsics and tilted poses; the 61 x 5 frames are
    views into wider arrays; F32 frames carry the special values and the depth limits with their neighbours; XYZ frames with 12-, 16- and
    32-byte points"""
    rng = np.random.default_rng(seed)
    out = []
    for (w, h) in SHAPES:
        pad = 3 if (w, h) == (61, 5) else 0
        img = padded(u16_image(rng, w, h), pad) if pad else u16_image(rng, w, h)
        out.append(("u16_%dx%d" % (w, h), capi.depth_frame(img, sensor_to_base=tilted_pose(rng), **_intrinsics(rng, w, h)), img))
        out.append(("u16_range_%dx%d" % (w, h), capi.depth_frame(img, depth_scale=0.00025, min_depth=0.2, max_depth=0.8,
                                                                  sensor_to_base=tilted_pose(rng), **_intrinsics(rng, w, h)), img))
        lim = (0.5, 2.5)
        img = f32_image(rng, w, h, lim)
        img = padded(img, pad) if pad else img
        out.append(("f32_%dx%d" % (w, h), capi.depth_frame(img, min_depth=lim[0], max_depth=lim[1], sensor_to_base=tilted_pose(rng),
                                                           **_intrinsics(rng, w, h)), img))
        out.append(("f32_scaled_%dx%d" % (w, h), capi.depth_frame(img, depth_scale=0.37, sensor_to_base=tilted_pose(rng),
                                                                  **_intrinsics(rng, w, h)), img))
        for floats in (3, 4, 8):
            img = xyz_image(rng, w, h, floats)
            img = padded(img, pad) if pad else img
            out.append(("xyz%d_%dx%d" % (floats * 4, w, h), capi.xyz_frame(img, sensor_to_base=tilted_pose(rng)), img))
    return out


def words(points):
    return np.ascontiguousarray(points, dtype=F).view(np.uint32).reshape(-1, 3)


def _refusals():
    """(name, field overrides on a valid 4 x 3 frame of each kind it applies to, expected code)"""
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    nan, inf = float("nan"), float("inf")
    both = [("null_data", dict(data=None), A), ("kind_3", dict(kind=3), A), ("kind_negative", dict(kind=-1), A),
            ("on_device_2", dict(on_device=2), A), ("on_device_negative", dict(on_device=-1), A),
            ("width_0", dict(width=0), A), ("height_0", dict(height=0), A), ("width_negative", dict(width=-4), A),
            ("row_stride_small", dict(row_stride_bytes="row-1elem"), A), ("row_stride_misaligned", dict(row_stride_bytes="row+1"), A),
            ("data_misaligned", dict(data="+1"), A), ("matrix_nan", dict(sensor_to_base=[1, 0, 0, nan, 0, 1, 0, 0, 0, 0, 1, 0]), A),
            ("matrix_inf", dict(sensor_to_base=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, inf, 0]), A),
            ("too_many_pixels", dict(width=65536, height=32768, row_stride_bytes="huge"), CAP)]
    depth = [("fx_0", dict(fx=0.0), A), ("fy_0", dict(fy=0.0), A), ("fx_nan", dict(fx=nan), A), ("fy_inf", dict(fy=inf), A),
             ("cx_nan", dict(cx=nan), A), ("cy_inf", dict(cy=-inf), A), ("min_depth_nan", dict(min_depth=nan), A),
             ("max_depth_inf", dict(max_depth=inf), A), ("scale_0", dict(depth_scale=0.0), A), ("scale_negative", dict(depth_scale=-0.001), A),
             ("scale_nan", dict(depth_scale=nan), A), ("scale_inf", dict(depth_scale=inf), A)]
    xyz = [("point_stride_8", dict(point_stride_bytes=8), A), ("point_stride_14", dict(point_stride_bytes=14), A)]
    return both, depth, xyz


def refusal_frames():
    """-> list of (name, frame, expected code, arrays to keep alive): shared with the GPU suite (haf_score_frames refuses the same)"""
    both, depth, xyz = _refusals()
    out = []
    for kind, dtype, shape in ((capi.FRAME_DEPTH_U16, np.uint16, (3, 4)), (capi.FRAME_DEPTH_F32, np.float32, (3, 4)),
                               (capi.FRAME_XYZ_F32, np.float32, (3, 4, 3))):
        for name, over, code in both + (xyz if kind == capi.FRAME_XYZ_F32 else depth):
            arr = np.ones(shape, dtype)
            f = capi.depth_frame(arr, 500.0, 500.0, 2.0, 1.5) if kind != capi.FRAME_XYZ_F32 else capi.xyz_frame(arr)
            elem = arr.itemsize if kind != capi.FRAME_XYZ_F32 else 12
            over = dict(over)
            if over.get("row_stride_bytes") == "row-1elem":
                over["row_stride_bytes"] = 4 * elem - (elem if kind != capi.FRAME_XYZ_F32 else 4)
            elif over.get("row_stride_bytes") == "row+1":
                over["row_stride_bytes"] = 4 * elem + 1
            elif over.get("row_stride_bytes") == "huge":
                over["row_stride_bytes"] = 65536 * elem
            if over.get("data") == "+1":
                over["data"] = arr.ctypes.data + 1
            for k, v in over.items():
                if k == "sensor_to_base":
                    v = (C.c_float * 12)(*v)
                setattr(f, k, v)
            out.append(("%s_kind%d" % (name, kind), f, code, arr))
    return out


def write_pgm16(path, image, maxval=65535, comment=True):
    h, w = image.shape
    head = b"P5\n" + (b"# depth in millimetres\n" if comment else b"") + b"%d %d\n" % (w, h) + \
           (b"#another comment\n" if comment else b"") + b"%d\n" % maxval
    with open(path, "wb") as f:
        f.write(head + image.astype(">u2").tobytes())
    return head
