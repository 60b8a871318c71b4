"""Shared by tests/test_segment_cpu.py and tests/test_segment_gpu.py: an independent numpy mirror of haf_segment_ref (include/hafgrasp.h)
and the frames both suites run it on.  The points are frame_cases.mirror_points'; h and d2 are numpy float32 arithmetic, one rounded
operation each; the components come from min-label propagation with pointer jumping, the numbering and the infos from sorting and
recounting -- nothing here shares code or method with csrc/segment_host.cpp (a sequential union-find) or csrc/segment.hip."""
import numpy as np

import frame_cases as fc
from haf_grasping_amd import capi

F = np.float32
# (width, height): one pixel; a few; padded rows; one 64 x 16 tile exactly; one pixel over each way; more than two tiles each way, twice
SHAPES = [(1, 1), (7, 3), (61, 5), (64, 16), (65, 17), (130, 35), (200, 50)]
VGA = (640, 480)
FX = 500.0
TABLE, LOW, HIGH = 0.700, 0.050, 0.120          # depth of the support, and the two object heights above it (a 7 cm step: no link)


def link_graph(frame, image, p):
    """-> (fg [H, W], right [H, W - 1], down [H - 1, W]): the definition's two predicates in numpy float32"""
    H, W = image.shape[:2]
    pts = fc.mirror_points(frame, image).view(F).reshape(H, W, 3)
    x, y, z = pts[:, :, 0], pts[:, :, 1], pts[:, :, 2]
    a, b, c, d = (F(v) for v in p.plane)
    with np.errstate(all="ignore"):
        h = ((a * x + b * y) + c * z) + d
        assert h.dtype == F
        fg = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~np.isnan(h) & (h >= F(p.min_height))
        if F(p.max_height) > 0:
            fg &= h <= F(p.max_height)
        gap2 = F(p.max_gap) * F(p.max_gap)
        assert type(gap2) is F

        def near(s, t):
            dx, dy, dz = x[t] - x[s], y[t] - y[s], z[t] - z[s]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            return fg[s] & fg[t] & np.isfinite(d2) & (d2 <= gap2)
        right = near((slice(None), slice(0, -1)), (slice(None), slice(1, None)))
        down = near((slice(0, -1), slice(None)), (slice(1, None), slice(None)))
    return fg, right, down


def components(fg, right, down):
    """-> int64 [H, W]: the lowest pixel index of every foreground pixel's connected component, -1 for background"""
    H, W = fg.shape
    n = H * W
    lab = np.where(fg, np.arange(n).reshape(H, W), n)
    while True:
        new = lab.copy()
        m = np.minimum(lab[:, :-1], lab[:, 1:])
        new[:, :-1] = np.where(right, np.minimum(new[:, :-1], m), new[:, :-1])
        new[:, 1:] = np.where(right, np.minimum(new[:, 1:], m), new[:, 1:])
        m = np.minimum(lab[:-1, :], lab[1:, :])
        new[:-1, :] = np.where(down, np.minimum(new[:-1, :], m), new[:-1, :])
        new[1:, :] = np.where(down, np.minimum(new[1:, :], m), new[1:, :])
        flat = np.append(new.reshape(-1), n)              # (the background's label points at itself)
        while True:                                       # pointer jumping: a label is the index of a pixel of the same component
            nxt = flat[flat]
            if (nxt == flat).all():
                break
            flat = nxt
        new = flat[:n].reshape(H, W)
        if (new == lab).all():
            break
        lab = new
    return np.where(fg, lab, -1)


def number(roots, p, dtype):
    """-> (labels, infos, stats, partition key) from the components' lowest indices, as the definition numbers them"""
    H, W = roots.shape
    flat = roots.reshape(-1)
    anchors, inverse, sizes = np.unique(flat[flat >= 0], return_inverse=True, return_counts=True)      # (ascending)
    passes = sizes >= p.min_pixels
    num = np.cumsum(passes) * passes
    num[num > p.max_labels] = 0
    labels = np.zeros(H * W, np.int64)
    labels[flat >= 0] = num[inverse]
    kept = int(passes.sum())
    n_labels = min(kept, p.max_labels)
    infos = np.zeros(n_labels, capi.SEGMENT_INFO_DTYPE)
    img = labels.reshape(H, W)
    vs, us = np.nonzero(img)
    ls = img[vs, us] - 1
    for name, src, fn, init in (("u_min", us, np.minimum, W), ("u_max", us, np.maximum, -1), ("v_min", vs, np.minimum, H), ("v_max", vs, np.maximum, -1)):
        acc = np.full(n_labels, init, np.int64)
        fn.at(acc, ls, src)
        infos[name] = acc
    chosen = anchors[(num > 0)]
    infos["n_pixels"] = sizes[num > 0]
    infos["anchor_u"], infos["anchor_v"] = chosen % W, chosen // W
    stats = [H * W, int((flat >= 0).sum()), int(anchors.size), kept]
    return img.astype(dtype), infos, stats


def mirror_segment(frame, image, p, dtype=np.uint8):
    """haf_segment_ref in numpy -> (labels [H, W] of dtype, infos, stats)"""
    return number(components(*link_graph(frame, image, p)), p, dtype)


# ---- the frames -------------------------------------------------------------------------------------------------------------------

def _height_maps(name, w, h, rng, min_pixels):
    """-> height above the table per pixel in metres (0: the table itself, i.e. background; nan: an invalid pixel), or None when the
    pattern does not apply to the shape"""
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    hm = np.zeros((h, w))
    if name == "random":                                  # ~55 % foreground on 9 x 7 blocks of two heights (planted depth steps), holes, too-high pixels
        step = np.where((u // 9 + v // 7) % 2 == 0, LOW, HIGH)
        r = rng.random((h, w))
        hm = np.where(r < 0.55, step, 0.0)
        hm[(r >= 0.55) & (r < 0.60)] = np.nan
        hm[(r >= 0.60) & (r < 0.63)] = 0.300             # above max_height
    elif name == "serpentine":                            # one pixel wide through every row: even rows whole, odd rows one pixel at alternating ends
        hm[0::2, :] = LOW
        hm[1::4, w - 1] = LOW
        hm[3::4, 0] = LOW
    elif name == "comb":                                  # vertical bars joined only by the last row
        hm[:, 0::2] = LOW
        hm[h - 1, :] = LOW
    elif name == "checker":
        hm[(u + v) % 2 == 0] = LOW
    elif name == "background":
        pass
    elif name == "foreground":
        hm[:] = LOW
    elif name == "size_rule":                             # runs of min_pixels - 1 and min_pixels pixels side by side, on two rows
        if w < 2 * min_pixels + 1:
            return None
        for row in (0, h - 1):
            hm[row, 0:min_pixels - 1] = LOW
            hm[row, min_pixels:2 * min_pixels] = LOW
    else:
        raise KeyError(name)
    return hm


PATTERNS = ["random", "serpentine", "comb", "checker", "background", "foreground", "size_rule"]
KINDS = ["u16", "f32", "xyz"]


def params_for(name, pose):
    """the support plane of the patterns in the base frame of `pose` (12 floats): in the sensor frame h = TABLE - z"""
    m = np.asarray(pose, np.float64).reshape(3, 4)
    nb = m[:, :3] @ np.array([0.0, 0.0, -1.0])
    plane = list(nb) + [TABLE - float(nb @ m[:, 3])]
    kw = dict(plane=plane, min_height=0.01, max_height=0.2, max_gap=0.02, min_pixels=3, max_labels=255)
    if name == "checker":
        kw.update(min_pixels=1)
    if name == "size_rule":
        kw.update(min_pixels=5)
    if name == "serpentine":
        kw.update(max_height=0.0)
    return kw


IDENTITY = np.eye(3, 4, dtype=F).reshape(-1)


def make_case(pattern, kind, shape, tilted, seed=0):
    """-> (frame, image, params kw) or None when the pattern does not apply.  (61, 5) is a view into padded rows"""
    w, h = shape
    rng = np.random.default_rng([seed, PATTERNS.index(pattern), KINDS.index(kind), w, h, int(tilted)])
    pose = fc.tilted_pose(rng) if tilted else IDENTITY
    kw = params_for(pattern, pose)
    hm = _height_maps(pattern, w, h, rng, kw["min_pixels"])
    if hm is None:
        return None
    z = TABLE - hm                                        # metres; nan = invalid
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    pad = 3 if shape == (61, 5) else 0
    if kind == "u16":
        img = np.where(np.isnan(z), 0, np.round(np.nan_to_num(z) * 1000)).astype(np.uint16)
    elif kind == "f32":
        img = z.astype(F)
    else:
        u, v = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
        zf = z.astype(F)
        img = np.stack([(u - F(cx)) / F(FX) * zf, (v - F(cy)) / F(FX) * zf, zf], axis=2).astype(F)
    if pad:
        img = fc.padded(img, pad)
    if kind == "xyz":
        frame = capi.xyz_frame(img, sensor_to_base=pose)
    else:
        frame = capi.depth_frame(img, FX, FX, cx, cy, sensor_to_base=pose)
    return frame, img, kw


def small_cases(shapes=None):
    """-> [(name, frame, image, params kw)]: every pattern x kind x pose on every small shape it applies to"""
    out = []
    for shape in shapes or SHAPES:
        for pattern in PATTERNS:
            for kind in KINDS:
                for tilted in (False, True):
                    c = make_case(pattern, kind, shape, tilted)
                    if c is not None:
                        out.append(("%s_%s_%dx%d_%s" % (pattern, kind, shape[0], shape[1], "tilted" if tilted else "identity"),) + c)
    return out


def vga_cases():
    """the one 640 x 480: all foreground (one component of 307 200 pixels) and the ragged random pattern under a tilted pose"""
    out = []
    for pattern, kind, tilted in (("foreground", "u16", False), ("random", "f32", True)):
        out.append(("%s_%s_640x480" % (pattern, kind),) + make_case(pattern, kind, VGA, tilted))
    return out


def tie_cases():
    """Exact ties on `<=`: XYZ frames with an identity pose, so the points are the stored floats.  -> [(name, frame, image, params kw,
    expected labels)]: neighbours at distance exactly 5 (offsets 3, 4, 0) link with max_gap = 5 and not with the float below; a point
    at h == min_height and at h == max_height is foreground, its float neighbour outside is not"""
    below5 = float(np.nextafter(F(5), F(0)))
    row = np.array([[[0, 0, 1], [3, 4, 1], [6, 8, 1]]], F)                       # three points in a row, 5 apart
    col = np.ascontiguousarray(row.transpose(1, 0, 2))
    base = dict(plane=[0, 0, 1, 0], min_height=0.5, max_height=0.0, min_pixels=1, max_labels=255)
    out = []
    for name, img in (("row", row), ("col", col)):
        f = capi.xyz_frame(img)
        one = np.ones(img.shape[:2], np.uint8)
        out.append(("gap_tie_links_" + name, f, img, dict(base, max_gap=5.0), one))
        out.append(("gap_below_tie_splits_" + name, f, img, dict(base, max_gap=below5), np.arange(1, 4, dtype=np.uint8).reshape(one.shape)))
    lo, hi = F(0.25), F(0.75)
    zs = [np.nextafter(lo, F(0)), lo, np.nextafter(lo, F(1)), np.nextafter(hi, F(0)), hi, np.nextafter(hi, F(1))]
    img = np.zeros((1, 6, 3), F)
    img[0, :, 2] = zs
    img[0, :, 0] = np.arange(6) * 10.0                                            # far apart: no links
    want = np.array([[0, 1, 2, 3, 4, 0]], np.uint8)
    out.append(("height_ties", capi.xyz_frame(img), img, dict(plane=[0, 0, 1, 0], min_height=float(lo), max_height=float(hi), max_gap=1.0,
                                                              min_pixels=1, max_labels=255), want))
    return out


def checker_cap_cases():
    """the checkerboard against the caps: 130 x 35 gives 2 275 singletons, under HAF_MAX_LABELS; 200 x 50 gives 5 000, over it: uint16
    keeps 4 096, uint8 keeps 255.  -> [(name, frame, image, params kw, dtype, expected n_labels, expected stats[3])]"""
    out = []
    for shape, comps in (((130, 35), 2275), ((200, 50), 5000)):
        for dtype, cap in ((np.uint16, capi.MAX_LABELS), (np.uint8, 255)):
            frame, img, kw = make_case("checker", "u16", shape, False)
            kw.update(max_labels=cap)
            out.append(("checker_cap_%dx%d_%s" % (shape[0], shape[1], np.dtype(dtype).name), frame, img, kw, dtype, min(comps, cap), comps))
    return out


def same(a, b):
    """two (labels, infos, stats) triples agree in every word, field and count"""
    return a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
