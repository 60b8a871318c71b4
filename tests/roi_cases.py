"""Shared by tests/test_roi_cpu.py and tests/test_roi_gpu.py: an independent numpy mirror of haf_score_frames_roi's definition
(include/hafgrasp.h) -- the ROI cells S_r of the masked pixels (frame_cases.mirror_points + grasp_map_cases.mirror_cells on the oracle's
roll transforms), their dilation by the 29 taps of the vote, the record rule on a vote grid (first-wins argmax, longest-run centring,
9 x 8 z window) -- and the masks both suites run it on."""
import numpy as np

import grasp_map_cases as gm

F = np.float32
# the footprint of the vote (server.cpp:873-878): |dr| <= 2 and |dc| <= 2, plus dr = 0 and |dc| = 3, 4
TAPS = [(dr, dc) for dr in range(-2, 3) for dc in range(-2, 3)] + [(0, -4), (0, -3), (0, 3), (0, 4)]
assert len(TAPS) == 29 and set(TAPS) == {(-a, -b) for a, b in TAPS}


def mirror_roi(Ms, words, mask, H, W):
    """Ms [R, 16], words uint32 [N, 3] of the pixels' points (frame_cases.mirror_points), mask uint8 [height, width] -> bool [R, H, W]"""
    pts = np.ascontiguousarray(words, dtype=np.uint32).view(F).reshape(-1, 3)
    sel = (np.asarray(mask).reshape(-1) != 0) & np.isfinite(pts).all(axis=1)
    S = np.zeros((len(Ms), H * W), bool)
    for r in range(len(Ms)):
        c, _ = gm.mirror_cells(Ms[r], pts[sel], H, W)
        S[r, c[c >= 0]] = True
    return S.reshape(len(Ms), H, W)


def dilate(S):
    """bool [..., H, W] -> the cells c with c + t set for some tap t, tap by tap"""
    H, W = S.shape[-2:]
    out = np.zeros_like(S)
    for dr, dc in TAPS:
        r0, r1, c0, c1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
        out[..., r0:r1, c0:c1] |= S[..., r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def key_max(vals):
    """max under the ordered-int key of a float (-0.0 below +0.0), start -10"""
    b = np.concatenate([np.array([-10.0], F), vals.astype(F)]).view(np.int32)
    k = np.where(b >= 0, b, b ^ 0x7FFFFFFF)
    m = int(k.max())
    return np.array([m if m >= 0 else m ^ 0x7FFFFFFF], np.int32).view(F)[0]


def mirror_record(ev, heights=None):
    """The reference's record of one roll from its vote grid (server.cpp:882-932): the top vote, then the longest horizontal run of it
    -- the first longest in row-major order -- and col = run end - len / 2; with `heights` the maximum above -10 of rows row-4..row+4,
    cols col-4..col+3 (1342-1351) -> (vote, row, col[, h_locmax])"""
    ev = np.asarray(ev).astype(np.int64)
    H, W = ev.shape
    top = int(ev.max())
    best = (0, 0, 0)                                       # (length, row, col)
    for row in np.flatnonzero((ev == top).any(axis=1)):
        cur = 0
        for col in range(W):
            cur = cur + 1 if ev[row, col] == top else 0
            if cur > best[0]:
                best = (cur, int(row), col - cur // 2)
    _, row, col = best
    if heights is None:
        return top, row, col
    win = heights[max(0, row - 4):min(H, row + 5), max(0, col - 4):min(W, col + 4)].ravel()
    return top, row, col, key_max(win[win > -10.0])


def masks(words, height, width, rect=None, seed=11):
    """-> list of (name, uint8 [height, width] mask) for a frame whose pixels' points are `words`: a rectangle (rect = (v0, v1, u0, u1),
    default the central third), ~200 scattered single pixels, all ones, all zeros, only invalid pixels, one valid pixel, and the
    rectangle once more as a view into a wider array (a padded stride) with values other than 1"""
    pts = np.ascontiguousarray(words, dtype=np.uint32).view(F).reshape(-1, 3)
    valid = np.isfinite(pts).all(axis=1).reshape(height, width)
    rng = np.random.default_rng(seed)
    v0, v1, u0, u1 = rect if rect is not None else (height // 3, max(height // 3 + 1, 2 * height // 3), width // 3, max(width // 3 + 1, 2 * width // 3))
    box = np.zeros((height, width), np.uint8)
    box[v0:v1, u0:u1] = 1
    scattered = np.zeros(height * width, np.uint8)
    pool = np.flatnonzero(valid.reshape(-1)) if valid.any() else np.arange(height * width)
    scattered[rng.choice(pool, size=min(200, pool.size), replace=False)] = 255
    one = np.zeros(height * width, np.uint8)
    inside = np.flatnonzero((valid & (box != 0)).reshape(-1))
    one[inside[inside.size // 2] if inside.size else pool[pool.size // 2]] = 7
    wide = np.full((height, width + 5), 9, np.uint8)       # (the padding is NOT zero: reading it would select pixels)
    wide[:, :width] = box * 200
    return [("rect", box), ("scattered", scattered.reshape(height, width)), ("ones", np.ones((height, width), np.uint8)),
            ("zeros", np.zeros((height, width), np.uint8)), ("invalid_only", (~valid).astype(np.uint8)), ("one_pixel", one.reshape(height, width)),
            ("rect_padded", wide[:, :width])]


def oracle_transforms(cfg_kw, in_kw, roll_first, count):
    """the CPU oracle's own 4x4 roll transforms (hafo_transform): [count, 16] float32"""
    import ctypes as C
    from oracle import oracle as O
    from test_engine_gpu import oracle_input
    ocfg = O.make_cfg(**{k: v for k, v in cfg_kw.items() if k in ("n_rolls", "roll_step_deg")}, H=cfg_kw.get("grid_h", 56), W=cfg_kw.get("grid_w", 56))
    oin = oracle_input(in_kw)
    out = np.zeros((count, 16), F)
    for r in range(count):
        O.lib().hafo_transform(C.byref(ocfg), C.byref(oin), roll_first + r, 0, out[r].ctypes.data)
    return out


# table1 rendered from CAM_A at C3: a rectangle over one object (rows 200..279, columns 280..359 of the 640 x 480 image).  On the CPU
# oracle's grids it selects 3 800 ROI cells and 6 368 of the full request's 31 093 evaluations, with a best vote of 93
C3_RECT = (200, 280, 280, 360)
