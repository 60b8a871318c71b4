"""Shared by tests/test_labels_cpu.py and tests/test_labels_gpu.py: the instance-label images and an independent numpy expectation of
the best pixel per label (include/hafgrasp.h: haf_label_best_ref, haf_grasp_map_labels).  Per label the expectation is
grasp_map_cases.key_argmax over the mask `labels == l` plus a count of the qualifying pixels; the order of the found labels is a lexsort
of (vote descending, roll, pixel index ascending)."""
import numpy as np

import grasp_map_cases as gm
from haf_grasping_amd import capi

NO_CELL = gm.NO_CELL
FIELDS = ("found", "u", "v", "vote", "roll", "cell", "n_pixels")


def blocks80(width=640, height=480):
    """48 blocks of 80 x 80 pixels: (v // 80) * 8 + u // 80 + 1, uint8"""
    v, u = np.mgrid[0:height, 0:width]
    return ((v // 80) * 8 + u // 80 + 1).astype(np.uint8)


def interleave(L, width=640, height=480):
    """(v * width + u) % L + 1: neighbouring pixels carry different labels, uint16"""
    v, u = np.mgrid[0:height, 0:width]
    return ((v * width + u) % L + 1).astype(np.uint16)


def padded_view(labels, pad):
    """the same labels as a view into an array whose rows are `pad` elements longer, the padding full of a label that must never be read"""
    wide = np.full((labels.shape[0], labels.shape[1] + pad), 3, labels.dtype)
    wide[:, :labels.shape[1]] = labels
    view = wide[:, :labels.shape[1]]
    assert view.strides[0] > labels.shape[1] * labels.itemsize
    return view


def expect(vote, roll, cell, labels, n_labels, min_vote):
    """vote / roll / cell: [height, width] images of a grasp map; labels: [height, width] -> (picks capi.LABEL_PICK_DTYPE [n_labels],
    order: the found labels, best first)"""
    h, w = labels.shape
    vote, roll, cell = (np.asarray(a).reshape(h, w) for a in (vote, roll, cell))
    picks = np.zeros(n_labels, capi.LABEL_PICK_DTYPE)
    picks["u"] = picks["v"] = picks["roll"] = picks["cell"] = -1
    picks["vote"] = NO_CELL
    lab = labels.astype(np.int64)
    ok = (roll.astype(np.int64) >= 0) & (vote.astype(np.int64) >= min_vote) & (lab >= 1) & (lab <= n_labels)
    count = np.bincount(lab[ok], minlength=n_labels + 1)
    for l in np.flatnonzero(count[1:n_labels + 1]) + 1:
        u, v = gm.key_argmax(vote, roll, labels == l, min_vote)
        picks[l - 1] = (1, u, v, vote[v, u], roll[v, u], cell[v, u], count[l])
    assert all(gm.key_argmax(vote, roll, labels == l, min_vote) is None for l in range(1, min(n_labels, 64) + 1) if not count[l])
    found = np.flatnonzero(picks["found"])
    p = picks[found]
    rank = np.lexsort((p["v"].astype(np.int64) * w + p["u"], p["roll"], -p["vote"].astype(np.int64)))
    return picks, [int(x) + 1 for x in found[rank]]


def assert_picks_equal(got, want, name):
    """got: a dict of label_best_ref / best_per_label, want: expect()'s tuple"""
    picks, order = want
    assert got["picks"].shape == picks.shape, (name, got["picks"].shape, picks.shape)
    for f in FIELDS:
        bad = np.flatnonzero(got["picks"][f] != picks[f])
        assert bad.size == 0, (name, f, bad.size, bad[:5] + 1, got["picks"][f][bad[:5]], picks[f][bad[:5]])
    assert got["order"] == order, (name, got["order"][:8], order[:8])


def small_frames(depth, cam, u0, v0, width=13, height=7, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    """the width x height window of a 16UC1 image at (u0, v0) as frames of all three kinds that see the same scene (the principal point
    moves with the window): a partial last group for G = 8 and G = 4 -> list of (name, frame, image)"""
    crop = np.ascontiguousarray(depth[v0:v0 + height, u0:u0 + width])
    k = dict(fx=fx, fy=fy, cx=cx - u0, cy=cy - v0)
    metres = crop.astype(np.float32) * np.float32(0.001)
    pts = capi.frame_points(capi.depth_frame(crop, **k)).reshape(height, width, 3).copy()
    return [("u16_%dx%d" % (width, height), capi.depth_frame(crop, sensor_to_base=cam, **k), crop),
            ("f32_%dx%d" % (width, height), capi.depth_frame(metres, sensor_to_base=cam, **k), metres),
            ("xyz_%dx%d" % (width, height), capi.xyz_frame(pts, sensor_to_base=cam), pts)]
