"""The synthetic grids of tests/vote_cases.py on the CPU: every case has the property it is named for, read from the numpy mirror alone
-- so a case that stops exercising its edge fails here -- and the CPU oracle's hafo_vote / hafo_vote_f equal the mirror on every case
at every size: the vote grid bit for bit and (row, col, top).  Also the label grids of models whose labels are not +-1."""
import os
import subprocess

import numpy as np
import pytest

import models
import pcdio
import roi_cases as rc
import vote_cases as vc
from oracle import oracle as O
from oracle_inputs import oracle_input

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _weight(dr, dc):
    return {(r, c): w for w, r, c in vc.WEIGHTS}.get((dr, dc), 0)


def test_weights_are_the_sources():
    """server.cpp:873-878 spelt out once more, row by row"""
    rows = {-2: (0, 0, 1, 2, 3, 2, 1, 0, 0), -1: (0, 0, 2, 3, 4, 3, 2, 0, 0), 0: (2, 2, 3, 4, 55, 4, 3, 2, 2), 1: (0, 0, 2, 3, 4, 3, 2, 0, 0),
            2: (0, 0, 1, 2, 3, 2, 1, 0, 0)}
    for dr, ws in rows.items():
        assert tuple(_weight(dr, dc) for dc in range(-4, 5)) == ws


@pytest.mark.parametrize("N", vc.SIZES)
def test_int_cases_have_their_properties(N):
    families = {fam for fam, _ in vc.int_cases(N)}
    assert families == set(vc.FAMILIES) - (set() if N >= 129 else {"block_seams"})
    for fam, c in vc.int_cases(N):
        g = c.grid
        assert g.dtype == np.int8 and g.shape == (N, N) and g.min() >= -9 and g.max() <= 99, c
        ev = vc.vote_int(g)
        st = vc.stats(ev)
        for k in st:
            if k in c.claim:
                assert st[k] == c.claim[k], (c, k, st[k], c.claim[k])
        assert (ev[g < 0] == 0).all() and (ev[:2] == 0).all() and (ev[-2:] == 0).all() and (ev[:, :4] == 0).all() and (ev[:, -4:] == 0).all()
        if N <= 61:                                          # the vectorised record against roi_cases' loop
            assert rc.mirror_record(ev) == vc.record_int(ev), c
        if c.claim.get("negative"):
            assert st["vmin"] < 0, c
        if "over" in c.claim:                                # the run starts before and ends after that column (a run of 1 lies on it)
            L, m = c.claim["run"], c.claim["over"]
            _, c0, ln = vc.runs_of(ev, st["top"])
            assert ln.tolist() == [L] and (c0[0] < m <= c0[0] + L - 1 if L > 1 else c0[0] == m), c
        if "seam" in c.claim:                                # the seam lies inside a grid row: two workgroups share that row
            r, col = c.claim["seam"]
            assert (r * N + col) % vc.BLOCK == 0 and 0 < col < N and (r * N) // vc.BLOCK != (r * N + N - 1) // vc.BLOCK, c
        if c.claim.get("wide"):                              # more than two 8-bit digits of k_top_grasps' sort key
            for min_vote in (1, 71):
                lbits, vbits = N.bit_length(), (st["top"] - min_vote).bit_length()
                assert lbits + vbits > 16, (c, lbits, vbits)
            if c.name != "all 99" and N >= 56:               # ... and runs whose keys differ above the second digit
                vals = np.unique(ev[ev >= 71])
                assert vals.size > 10 and (st["top"] - vals.min()) << lbits >= 1 << 16, c
        if c.heights is not None:
            h = c.heights
            assert h.dtype == F and h.shape == (N, N)
            zk, zs = vc.z_key(h, st["row"], st["col"]), vc.z_seq(h, st["row"], st["col"])
            assert zk == zs and zk == rc.mirror_record(ev, h)[3], c          # the two forms agree as values ...
            if "z" in c.claim:
                assert zk == c.claim["z"], (c, zk)
            if c.claim.get("zero_signs"):                    # ... and differ only in the sign of a zero: the key form gives +0.0,
                first = h[st["row"], st["col"] - 1]          # the sequential form whichever zero comes first
                assert _bits(zk) == _bits(F(0.0)) and _bits(zs) == _bits(first), c
            else:
                assert _bits(zk) == _bits(zs), c
    # the clipped windows: each side of the grid is touched by some case's window
    if N >= 15:
        wins = [(c.claim["row"], c.claim["col"]) for fam, c in vc.int_cases(N) if fam == "heights"]
        assert any(r - 4 < 0 for r, _ in wins) and any(r + 4 > N - 1 for r, _ in wins) and any(c - 4 == 0 for _, c in wins) and \
            any(c + 3 == N - 2 for _, c in wins)


@pytest.mark.parametrize("N", vc.SIZES)
def test_border_cases_have_their_properties(N):
    """a label on the border scores 0 itself; on the +1 background the interior cells whose footprint reaches it move by weight x (value - 1)
    and nothing else moves -- stated here from the weights, not through the mirror's own loop"""
    base = vc.vote_int(np.ones((N, N), np.int8))
    walk = vc.border_walk(N)
    assert {(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (1, 3), (N // 2, 3), (N // 2, N - 4)} <= set(walk)
    for c in vc.border(N, -1):
        assert not vc.vote_int(c.grid).any() and (c.grid >= 0).sum() == 1 and c.claim["at"] in walk, c
    moved = 0
    cases = vc.border(N, +1)
    assert [c.claim["at"] for c in cases] == walk
    for c in cases:
        r0, c0 = c.claim["at"]
        v = int(c.grid[r0, c0])
        want = base.copy()
        for w, dr, dc in vc.WEIGHTS:
            r, q = r0 - dr, c0 - dc
            if 2 <= r < N - 2 and 4 <= q < N - 4:
                want[r, q] += w * (v - 1)
        ev = vc.vote_int(c.grid)
        assert ev[r0, c0] == 0 and (ev == want).all(), c
        moved += int((ev != base).any())
    assert moved > len(cases) // 2


@pytest.mark.parametrize("N", vc.SIZES)
def test_oracle_equals_mirror_int(N):
    cases = [c for _, c in vc.int_cases(N)] + vc.border(N, -1) + vc.border(N, +1)
    for c in cases:
        ev, rec = vc.oracle_vote(c.grid)
        want = vc.vote_int(c.grid)
        assert (_bits(ev) == _bits(want.astype(F))).all(), c
        assert rec == vc.record_int(want), (c, rec, vc.record_int(want))


@pytest.mark.parametrize("N", vc.SIZES)
def test_gated_mirror(N):
    """the gate zeroes before the argmax: S full is the ungated grid, S empty is all zero, and a gated-away top no longer wins"""
    c = vc.ties(N)[-1]
    ev = vc.vote_int(c.grid)
    sets = dict(vc.roi_sets(N))
    assert (vc.vote_int(c.grid, sets["full"]) == ev).all() and not vc.vote_int(c.grid, sets["empty"]).any()
    top, row, col = vc.record_int(ev)
    S = np.ones((N, N), bool)
    S[row] = False
    gated = vc.vote_int(c.grid, S)
    assert (gated[row] == 0).all() and vc.record_int(gated)[:2] == (top, row + 1)
    words = vc.roi_words(np.stack([s for _, s in vc.roi_sets(N)]))
    assert words.shape == (len(sets), N, (N + 63) // 64) and words.dtype == np.uint64
    for k, (_, s) in enumerate(vc.roi_sets(N)):
        back = (words[k][:, np.arange(N) >> 6] >> (np.arange(N, dtype=np.uint64) & np.uint64(63))) & np.uint64(1)
        assert (back.astype(bool) == s).all()


@pytest.mark.parametrize("N", vc.FLOAT_SIZES)
def test_float_cases_have_their_properties_and_oracle_equals_mirror(N):
    branches = set()
    for c in vc.float_cases(N):
        g = c.grid
        assert g.dtype == F and g.shape == (N, N)
        evf = vc.vote_f32(g)
        top, row, col, branch = vc.record_f32(evf)
        branches.add(branch)
        if "branch" in c.claim:
            assert branch in c.claim["branch"], (c, branch)
            if branch != "run":                              # no cell equals the truncated top
                assert not (evf == F(top)).any() and (np.trunc(evf) == top).any(), c
            if branch == "later":
                first = np.flatnonzero(np.trunc(evf).ravel() == top)[0]
                assert row * N + col > first and evf[row, col] > top, c
        for k, v in (("top", top), ("row", row), ("col", col)):
            if k in c.claim:
                assert c.claim[k] == v, (c, k, v)
        if c.claim.get("integer"):                           # integer-valued floats: the int rule
            gi = g.astype(np.int8)
            assert (gi.astype(F) == g).all()
            evi = vc.vote_int(gi)
            assert (evf == evi.astype(F)).all() and (top, row, col) == vc.record_int(evi) and branch == "run", c
        ev, rec = vc.oracle_vote(g)
        assert (_bits(ev) == _bits(evf)).all(), c
        assert rec == (top, row, col), (c, rec, (top, row, col, branch))
    assert branches == {"run", "first", "later"}


def test_float_rule_against_the_oracle_on_random_grids():
    """both branches occur, and the oracle settles every one of them"""
    rng = np.random.RandomState(3)
    seen = set()
    for i in range(300):
        N = int(rng.choice([15, 23, 40]))
        kind = i % 3
        if kind == 0:
            g = rng.randint(-4, 5, size=(N, N)) * 0.25
        elif kind == 1:
            g = rng.uniform(-1, 1, size=(N, N))
        else:
            g = np.where(rng.uniform(size=(N, N)) < 0.5, rng.randint(0, 3, size=(N, N)), rng.uniform(-1, 2, size=(N, N)))
        g = g.astype(F)
        evf = vc.vote_f32(g)
        top, row, col, branch = vc.record_f32(evf)
        ev, rec = vc.oracle_vote(g)
        assert (_bits(ev) == _bits(evf)).all() and rec == (top, row, col), (i, rec, (top, row, col, branch))
        seen.add(branch)
    assert seen == {"run", "first", "later"}


# ---- models whose labels are not +-1 ----

def _files(data_dir):
    return os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")


def test_label_grid_values():
    for (a, b), (ga, gb) in vc.LABEL_PAIRS.items():
        assert (O.lib().hafo_label_gridval(a), O.lib().hafo_label_gridval(b)) == (ga, gb)
        for lab, gv in ((a, ga), (b, gb)):
            assert int(("%g" % lab)[:2]) == gv and -9 <= gv <= 99


def _label_run(data_dir, tmp_path, pair):
    f, r = _files(data_dir)
    rq = vc.LABEL_REQUESTS[56]
    path = models.write_random_model(str(tmp_path / "m.model"), vc.LABEL_NSV, seed=rq["seed"], balanced=True, labels=pair)
    o = O.Oracle(f, r, path)
    xyz = pcdio.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    cfg, inp = O.make_cfg(n_rolls=rq["cfg"]["n_rolls"]), oracle_input(rq["inp"])
    return path, o, xyz, cfg, inp, o.run(xyz, cfg, inp)


@pytest.mark.parametrize("pair", list(vc.LABEL_PAIRS), ids=lambda p: "%d_%d" % p)
def test_oracle_label_grid_holds_the_pairs_grid_values(data_dir, tmp_path, pair):
    """the oracle's label grid holds exactly gridval(a) / gridval(b) on masked cells and -1 elsewhere, both classes present, and the votes
    are the mirror's"""
    path, o, xyz, cfg, inp, want = _label_run(data_dir, tmp_path, pair)
    ga, gb = vc.LABEL_PAIRS[pair]
    lab, m = want["labels"], want["mask"] == 1
    assert (lab[~m] == -1).all() and set(np.unique(lab[m]).tolist()) == {ga, gb}
    assert (lab[m] == ga).sum() > 50 and (lab[m] == gb).sum() > 50
    assert ((lab[m] == ga) == (want["dec"][m] > 0)).all()
    for roll in range(cfg.n_rolls):
        ev = vc.vote_int(lab[roll])
        assert (want["graspseval"][roll] == ev.astype(F)).all(), roll


@pytest.mark.skipif(not os.path.exists(os.path.join(O.ref_dir(), "svm-predict")), reason="oracle/_ref not built")
@pytest.mark.parametrize("pair", list(vc.LABEL_PAIRS), ids=lambda p: "%d_%d" % p)
def test_reference_svm_predict_prints_the_pairs_grid_values(data_dir, tmp_path, pair):
    """the first two characters of the label text the REAL svm-predict prints for such a model parse to the oracle's grid values (live)"""
    path, o, xyz, cfg, inp, want = _label_run(data_dir, tmp_path, pair)
    r = _files(data_dir)[1]
    lab, m = want["labels"], want["mask"] == 1
    feat = str(tmp_path / "f.txt")
    n = o.dump_feature_file(xyz, cfg, inp, 1, feat)
    assert n == m[1].sum()
    with open(feat + ".scale", "w") as out:
        subprocess.run([os.path.join(O.ref_dir(), "svm-scale"), "-r", r, feat], stdout=out, check=True)
    subprocess.run([os.path.join(O.ref_dir(), "svm-predict"), feat + ".scale", path, feat + ".out"], stdout=subprocess.DEVNULL, check=True)
    with open(feat + ".out") as fh:
        lines = fh.read().splitlines()
    assert [int(line[:2]) for line in lines] == lab[1][m[1]].tolist()
