#!/usr/bin/env python3
"""Writes the checksums tests/test_slot_loop_gpu.py compares against (GPU box): per roll of one fixed 256 x 256 request the 64-bit sums of
what the screening feature kernel wrote, and the tier counts.  Run it on the commit whose bits are the reference -- or with HAF_TESTLIB
naming a variant build of it (python -m haf_grasping_amd.build --variant NAME) -- and commit the file:
    python tools/record_slot_loop_sums.py [OUT.json]        (default: tests/golden/slot_loop_sums.json)"""
import json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import models
import test_slot_loop_gpu as T
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", T.FIXTURE)
mp = os.path.join(tempfile.mkdtemp(), "seed42.model")
models.write_random_model(mp, T.NSV, D=323, seed=T.SEED, balanced=True)
sums = T.slot_loop_sums(os.path.join(ROOT, "tests", "golden", "data"), mp)
with open(out, "w") as f:
    json.dump(sums, f, indent=1, sort_keys=True)
    f.write("\n")
print(out, sums["n_evals"], sums["counts"], sums["rolls"][0])
