"""The screening feature kernel's slot loop (csrc/feature_device.h: screen_group) may be re-scheduled, never re-computed: what
k_features_serial<2, true> writes for one fixed request -- the fp16 operand images, the raw band sums, a_x -- and the tier counts behind
it have to come out bit for bit as tests/golden/slot_loop_sums.json records them (tools/record_slot_loop_sums.py wrote it on an MI355X
from the commit BEFORE the loop was re-scheduled).  A corner read issued without its wait state after the M0 write, a register of a
read or scalar load in flight that the compiler moved, a counted wait that is one short: each returns wrong corners silently, and each
changes these sums."""
import hashlib
import json
import os

import numpy as np
import pytest

import models
from haf_grasping_amd import capi

GRID, ROLLS, NSV, SEED = 256, 8, 4096, 42
TILE_EVALS, TILE_BYTES, BAND_FLOATS = 32, 20480, 8      # csrc/kernels.h: kTile, kS0MatBytes, kBandFloats
FIXTURE = "slot_loop_sums.json"


def _sum64(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).hexdigest()


def slot_loop_sums(data_dir, model_path):
    """One 256 x 256 request of 8 rolls (468 512 evaluation slots: the thread-per-evaluation kernel, low-rank form) in the testing library ->
    per roll a 64-bit checksum of the operand image tiles that hold the roll's evaluations, of its band floats and of its a_x, as the
    feature kernel left them (Engine.snapshot_screen), plus the lengths of the tier lists and the counts of the request."""
    f, r = os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures")
    xyz = models.synthetic_cloud(grid=GRID, k=2, seed=0)
    eng = capi.Engine(f, r, model_path, testing=True, grid_h=GRID, grid_w=GRID, n_rolls=ROLLS, roll_step_deg=5, max_points=1 << 20)
    try:
        eng.snapshot_screen(True)
        inp = capi.default_input(grasp_area_length_x=GRID, grasp_area_length_y=GRID)
        eng.score_rolls([xyz], [inp], 0, ROLLS)
        assert eng.screen_low_rank()["last_used"], "the request did not take the low-rank form of the screening pass"
        cells = eng.fetch_list(0)
        n = len(cells)
        roll = cells // (GRID * GRID)
        assert n > 0 and cells.min() >= 0 and cells.max() < ROLLS * GRID * GRID
        X = eng.fetch_snapshot(0)
        X = X[:len(X) // TILE_BYTES * TILE_BYTES].reshape(-1, TILE_BYTES)
        gb = eng.fetch_snapshot(1).view(np.float32).reshape(-1, BAND_FLOATS)
        ax = eng.fetch_snapshot(2).view(np.float32)
        out = dict(request=dict(grid=GRID, rolls=ROLLS, nsv=NSV, seed=SEED, cloud="synthetic_cloud(grid=256, k=2, seed=0)"),
                   n_evals=int(n), screen_form=eng.screen_form(), counts=eng.last_counts(), exact_tiers=eng.last_exact_tiers(),
                   list_lengths=[int(len(eng.fetch_list(w))) for w in (1, 2, 3, 4)], rolls=[])
        for k in range(ROLLS):
            idx = np.flatnonzero(roll == k)                                     # (whatever the order of the evaluation list)
            tiles = np.unique(idx // TILE_EVALS)                                # every tile that holds an evaluation of the roll
            out["rolls"].append(dict(evals=int(len(idx)), cells=_sum64(cells[idx]), X=_sum64(X[tiles]), band=_sum64(gb[idx]), ax=_sum64(ax[idx])))
        return out
    finally:
        eng.close()


@pytest.mark.gpu
def test_screening_feature_kernel_reproduces_the_recorded_bits(data_dir, golden_dir, tmp_path):
    want = json.load(open(os.path.join(golden_dir, FIXTURE)))
    mp = str(tmp_path / "seed42.model")
    models.write_random_model(mp, NSV, D=323, seed=SEED, balanced=True)
    got = slot_loop_sums(data_dir, mp)
    assert got["n_evals"] == want["n_evals"] and got["screen_form"] == want["screen_form"]
    for k, (g, w) in enumerate(zip(got["rolls"], want["rolls"])):
        assert g == w, "roll %d: %r != %r" % (k, g, w)
    assert len(got["rolls"]) == len(want["rolls"]) == ROLLS
    assert got["counts"] == want["counts"] and got["exact_tiers"] == want["exact_tiers"] and got["list_lengths"] == want["list_lengths"]
