"""Shared by tests/test_top_grasps_gpu.py and tests/test_vote_gpu.py: a numpy mirror of haf_top_grasps' contract (include/hafgrasp.h,
steps 1-6), built from the engine's own grids of the last scored batch -- votes from haf_get_roll_grid, heights from
haf_debug_fetch(HEIGHTS), poses from haf_roll_pose on a synthesised record array -- and the comparison of two candidate lists."""
import numpy as np

from haf_grasping_amd import capi


def _key_max(vals):
    """max under k_vote_record's ordered-int key (-0.0 below +0.0), start -10"""
    b = np.concatenate([np.array([-10.0], np.float32), vals.astype(np.float32)]).view(np.int32)
    k = np.where(b >= 0, b, b ^ 0x7FFFFFFF)
    m = int(k.max())
    return np.array([m if m >= 0 else m ^ 0x7FFFFFFF], np.int32).view(np.float32)[0]


def _h_locmax(h, row, col):
    H, W = h.shape
    win = h[max(0, row - 4):min(H, row + 5), max(0, col - 4):min(W, col + 4)].ravel()
    return _key_max(win[win > -10.0])


def _roll_sequence(ev, h, min_vote, radius):
    """steps 1-3 for one grid: generator of (vote, row, col, len, h_locmax) of the in-roll greedy sequence"""
    ev = ev.astype(np.int64)
    H, W = ev.shape
    start = np.ones((H, W), bool)
    start[:, 1:] = ev[:, 1:] != ev[:, :-1]
    s = np.flatnonzero(start.ravel())
    e = np.append(s[1:], H * W) - 1
    vote = ev.ravel()[s]
    keep = vote >= min_vote
    s, e, vote = s[keep], e[keep], vote[keep]
    row, endc = e // W, e % W
    ln = e - s + 1
    col = endc - ln // 2
    order = np.lexsort((col, row, -ln, -vote))
    kr, kc = [], []
    for i in order:
        r, c = int(row[i]), int(col[i])
        if kr:
            ar, ac = np.asarray(kr), np.asarray(kc)
            if (np.maximum(np.abs(ar - r), np.abs(ac - c)) <= radius).any():
                continue
        kr.append(r)
        kc.append(c)
        yield int(vote[i]), r, c, int(ln[i]), _h_locmax(h, r, c)


def mirror(eng, gi, cloud, roll_first, R, n_evals, k=8, min_vote=None, cell_radius=7, roll_window=1, min_dist_m=0.02):
    """steps 1-6 for one cloud of the engine's last batch -> list of candidate dicts"""
    if min_vote is None:
        min_vote = eng.cfg.graspval_th + 1
    if int(gi.max_calculation_time) < 0:
        return []
    nr = eng.cfg.n_rolls
    circular = nr * eng.cfg.roll_step_deg == 180
    seqs, heads = [], []
    for i in range(R):
        roll = roll_first + i
        ev, _ = eng.roll_grid(cloud, roll)
        h = eng.debug(capi.DBG_HEIGHTS, cloud, roll)
        g = _roll_sequence(ev, h, min_vote, cell_radius)
        seqs.append(g)
        heads.append(next(g, None))
    kept = []
    while len(kept) < k:
        best = None
        for i in range(R):
            if heads[i] is not None and (best is None or heads[i][0] > heads[best][0]):
                best = i
        if best is None:
            break
        vote, r, c, ln, hl = heads[best]
        heads[best] = next(seqs[best], None)
        roll = roll_first + best
        rec = np.zeros(nr, capi.ROLL_RECORD_DTYPE)
        rec[roll] = (vote, r, c, hl, n_evals[best])
        d, _ = eng.roll_pose(gi, rec, roll)
        d["eval"] = vote - 20
        d.update(run_length=ln, h_locmax=float(hl))
        drop = False
        if roll_window > 0 and min_dist_m > 0:
            for q in kept:
                dr = abs(q["best_roll"] - roll)
                if circular:
                    dr = min(dr, nr - dr)
                if q["best_roll"] == roll or not 1 <= dr <= roll_window:
                    continue
                a, b = d["averaged_grasp_point"], q["averaged_grasp_point"]
                dx, dy, dz = np.float64(a[0]) - b[0], np.float64(a[1]) - b[1], np.float64(a[2]) - b[2]
                if dx * dx + dy * dy + dz * dz <= np.float64(min_dist_m) * np.float64(min_dist_m):
                    drop = True
                    break
        if not drop:
            kept.append(d)
    return kept


FIELDS = ("eval", "best_row", "best_col", "best_roll", "best_vote", "rolls_done", "n_evals", "n_rechecked", "run_length")
POSE = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector")


def assert_same(got, want, ctx=""):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert g[f] == w[f], (ctx, i, f, g[f], w[f])
        for f in POSE:
            assert tuple(g[f]) == tuple(w[f]), (ctx, i, f)
        assert g["roll"] == w["roll"] and np.float32(g["h_locmax"]).tobytes() == np.float32(w["h_locmax"]).tobytes(), (ctx, i)
