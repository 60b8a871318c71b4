"""Shared by tests/test_depth_filter_cpu.py and tests/test_depth_filter_gpu.py: an independent numpy-fp32 mirror of the two stages of
haf_filter_depth (include/hafgrasp.h) and the exposure stacks both suites run it on.  numpy float32 arithmetic rounds every operation,
and the mirror's median is a plain sort, so the mirror and haf_filter_depth_ref must agree word for word; the device kernel must agree
with haf_filter_depth_ref likewise."""
import numpy as np

import frame_cases as fc
from haf_grasping_amd import capi

F = np.float32
NAN_WORD = np.uint32(0x7FC00000)
# (width, height): one tile of the kernel exactly (64 x 16), one pixel over in both directions, more than two tiles each way; 61 x 5
# is a view into wider rows
SHAPES = [(1, 1), (7, 3), (61, 5), (64, 16), (65, 17), (130, 33)]
STACKS = [1, 2, 3, 8]                                    # 2 and 8: the lower median of an even count
K = dict(fx=525.0, fy=525.0, cx=30.5, cy=8.5)


def words(image):
    """an output image as what is compared: uint16 samples as they are, float32 samples as their words"""
    return image if image.dtype == np.uint16 else np.ascontiguousarray(image).view(np.uint32)


def mirror_filter(frame, images, p):
    """The header's two stages on `images` ([H, W] uint16 / float32 exposures) with `frame`'s scale and limits and the DepthFilter `p`
    -> (image of the exposures' dtype, [pixels, valid after stage T, kept])"""
    u16 = frame.kind == capi.FRAME_DEPTH_U16
    scale, mn, mx = F(frame.depth_scale), F(frame.min_depth), F(frame.max_depth)
    H, W = images[0].shape
    with np.errstate(all="ignore"):
        samples = []
        for img in images:
            if u16:
                valid = img != 0
                z = img.astype(F) * scale
            else:
                d = np.ascontiguousarray(img, dtype=F)
                valid = np.isfinite(d) & (d > F(0))
                z = d * scale
            valid = valid & np.isfinite(z)
            if mn > 0:
                valid &= ~(z < mn)
            if mx > 0:
                valid &= ~(z > mx)
            # an invalid sample sorts behind every valid one: U16 as integers, F32 as floats
            samples.append(np.where(valid, img.astype(np.int64), 1 << 20) if u16 else np.where(valid, np.ascontiguousarray(img, dtype=F), F(np.inf)))
        stack = np.sort(np.stack(samples), axis=0)
        c = (stack != ((1 << 20) if u16 else F(np.inf))).sum(axis=0)
        rank = np.maximum(c - 1, 0) // 2
        M = np.take_along_axis(stack, rank[None], axis=0)[0]
        valid_t = (c >= p.min_valid) & (c > 0)
        z = np.where(valid_t, (M.astype(np.uint16).astype(F) if u16 else M.astype(F)) * scale, F(np.nan)).astype(F)
        t = F(p.tol_abs) + F(p.tol_rel) * z
        assert z.dtype == F and t.dtype == F
        R = p.radius
        wide = np.full((H + 2 * R, W + 2 * R), np.nan, F)
        wide[R:R + H, R:R + W] = z
        support = np.zeros((H, W), np.int64)
        for dv in range(-R, R + 1):
            for du in range(-R, R + 1):
                if dv or du:
                    zq = wide[R + dv:R + dv + H, R + du:R + du + W]
                    diff = zq - z
                    assert diff.dtype == F
                    support += np.abs(diff) <= t
        keep = valid_t & (support >= p.min_support)
        if u16:
            out = np.where(keep, M, 0).astype(np.uint16)
        else:
            out = np.where(keep, M.astype(F).view(np.uint32), NAN_WORD).astype(np.uint32).view(F)
    return out, [H * W, int(valid_t.sum()), int(keep.sum())]


def _frame(img, kind_kw):
    return capi.depth_frame(img, **K, **kind_kw)


U16_KW = dict(depth_scale=0.001, min_depth=0.35, max_depth=3.9)
F32_KW = dict(depth_scale=1.0, min_depth=0.5, max_depth=2.5)


def _exposure(rng, kind, w, h, dead=False):
    if kind == "u16":
        img = fc.u16_image(rng, w, h)
        img[rng.random((h, w)) < 0.3] = 0                   # per-exposure drop-outs on top of the image's own
        if dead:
            img[:] = 0
    else:
        # (a fifth of its samples are NaN and the limits cut another 46 % of the rest: more than 30 % drop-outs per exposure as it is)
        img = fc.f32_image(rng, w, h, (F32_KW["min_depth"], F32_KW["max_depth"]))
        if dead:
            img[:] = -1.0
    return fc.padded(img, 3) if (w, h) == (61, 5) else img


def stacks(seed=20241018):
    """-> list of (name, frames, images): both kinds on every shape of SHAPES with 1, 2, 3 and 8 independent exposures -- so that the
    number of valid samples of a pixel takes every value 0..n -- and, per kind, one stack of three whose second exposure is all invalid"""
    rng = np.random.default_rng(seed)
    out = []
    for kind, kw in (("u16", U16_KW), ("f32", F32_KW)):
        for (w, h) in SHAPES:
            for n in STACKS:
                imgs = [_exposure(rng, kind, w, h) for _ in range(n)]
                out.append(("%s_%dx%d_n%d" % (kind, w, h, n), [_frame(i, kw) for i in imgs], imgs))
        imgs = [_exposure(rng, kind, 65, 17, dead=(j == 1)) for j in range(3)]
        out.append(("%s_65x17_n3_one_dead" % kind, [_frame(i, kw) for i in imgs], imgs))
    return out


def sweep(n):
    """the parameter sweep of a stack of n: radius 1, 2, 3; min_valid 1 and n; min_support 0, a middle value and (2 R + 1)^2 - 1.  The
    tolerances are wide (0.3 m + 10 %) because the exposures are independent images over 0.3..4 m: a neighbour then supports with a
    probability near a quarter and the support counts spread around the middle value"""
    out = []
    for radius in (1, 2, 3):
        full = (2 * radius + 1) ** 2 - 1
        for min_valid in sorted({1, n}):
            for min_support in (0, full // 4, full):
                out.append(capi.depth_filter(radius=radius, min_support=min_support, tol_abs=0.3, tol_rel=0.1, min_valid=min_valid))
    return out


def param_id(p):
    return "r%d_s%d_v%d" % (p.radius, p.min_support, p.min_valid)


def tie_cases():
    """-> list of (name, frames, images, params, expected image): depth_scale 1, tol_rel 0 and an integer tol_abs = k on a 7 x 3 image that
    is invalid but for p = 1000 at (3, 1), one neighbour at exactly p + k (supports p, and p it) and one at p + k + 1 on the other side
    (does not); k = 0: only equal depths support"""
    out = []
    for dt, name in ((np.uint16, "u16"), (np.float32, "f32")):
        for k in (0, 1, 5):
            img = np.zeros((3, 7), dt)
            img[1, 3], img[1, 2], img[1, 4] = 1000, 1000 + k, 1000 + k + 1
            for min_support, kept in ((1, [(1, 3), (1, 2)]), (2, [])):
                want = np.zeros((3, 7), dt) if dt == np.uint16 else np.full((3, 7), NAN_WORD, np.uint32).view(F)
                for rc in kept:
                    want[rc] = img[rc]
                p = capi.depth_filter(radius=1, min_support=min_support, tol_abs=float(k), tol_rel=0.0, min_valid=1)
                out.append(("%s_tie_k%d_s%d" % (name, k, min_support), [capi.depth_frame(img, **K, depth_scale=1.0)], [img], p, want))
    return out


def flying_pixel_scene(seed=7):
    """-> (exposures: three uint16 [64, 96] images in millimetres, planted: bool [64, 96]).  A background at 1000 and a box at 800 on rows
    16..47 and columns 30..60, Gaussian noise of sigma 1.5 (rounded), a flying pixel on every second row 16, 18, .., 46 in columns 29
    and 61 (32 in all) with a depth uniform in [840, 960], the same pixels in every exposure; the second exposure has 30 % drop-outs"""
    rng = np.random.default_rng(seed)
    planted = np.zeros((64, 96), bool)
    planted[16:48:2, 29] = planted[16:48:2, 61] = True
    exposures = []
    for j in range(3):
        img = np.full((64, 96), 1000.0)
        img[16:48, 30:61] = 800.0
        img = np.rint(img + rng.normal(0.0, 1.5, img.shape))
        img[planted] = rng.integers(840, 961, int(planted.sum()))
        if j == 1:
            img[rng.random(img.shape) < 0.3] = 0
        exposures.append(img.astype(np.uint16))
    return exposures, planted
