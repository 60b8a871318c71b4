"""Shared by tests/test_views_roi_cpu.py and tests/test_views_roi_gpu.py: the masks of a two-camera request of haf_score_views_roi
(include/hafgrasp.h) -- a rectangle in the first view and, in every other view, the valid pixels whose base-frame (x, y) lies in the
bounding box of the first view's masked points: what a second camera without a segmenter of its own can be given -- and the numpy mirror
of the request's ROI cell sets, the union of roi_cases.mirror_roi over the masked views."""
import numpy as np

import roi_cases as rc

F = np.float32


def points(words):
    return np.ascontiguousarray(words, dtype=np.uint32).view(F).reshape(-1, 3)


def bbox_mask(words_a, mask_a, words_b, height, width):
    """uint8 [height, width]: the pixels of view B whose point is finite and has min <= x <= max and min <= y <= max of the finite points
    of view A's masked pixels (all zeros when A has none)"""
    pa, pb = points(words_a), points(words_b)
    sel = (np.asarray(mask_a).reshape(-1) != 0) & np.isfinite(pa).all(axis=1)
    if not sel.any():
        return np.zeros((height, width), np.uint8)
    lo, hi = pa[sel, :2].min(axis=0), pa[sel, :2].max(axis=0)
    ok = np.isfinite(pb).all(axis=1)
    with np.errstate(invalid="ignore"):
        inside = ok & (pb[:, 0] >= lo[0]) & (pb[:, 0] <= hi[0]) & (pb[:, 1] >= lo[1]) & (pb[:, 1] <= hi[1])
    return inside.astype(np.uint8).reshape(height, width)


def rect_mask(rect, height, width):
    v0, v1, u0, u1 = rect
    m = np.zeros((height, width), np.uint8)
    m[v0:v1, u0:u1] = 1
    return m


def mirror_union(Ms, words, masks, H, W):
    """Ms [R, 16]; per view its points' words and its mask (None: the view selects nothing) -> bool [R, H, W]"""
    S = np.zeros((len(Ms), H, W), bool)
    for w, m in zip(words, masks):
        if m is not None:
            S |= rc.mirror_roi(Ms, w, m, H, W)
    return S
