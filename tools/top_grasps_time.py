"""Timing of haf_top_grasps (ranked top-K candidates of the last scored batch) on the bench's C5 workload and the C2 / C3 requests.

  python tools/top_grasps_time.py [--calls 50] [--out profiles/top_grasps_time.json]
      scores each workload once, then times haf_top_grasps (host wall clock, median of --calls calls) for a few parameter sets
  python tools/top_grasps_time.py --trace-only
      the same requests with 5 calls each and no output file: the body of a `rocprofv3 --kernel-trace --stats -- python ...` run
      (k_top_grasps' device time per call from its kernel_stats.csv)

C5: 512 x 512, 36 rolls of 5 degrees, the bench's synthetic cloud and its seeded random model (seed 42, 4096 SVs).  C2: pcd2.pcd,
32 x 32 cm, 12 rolls, surrogate model.  C3: table1_mult_obj, 56 x 56 cm, 20 rolls of 9 degrees, surrogate model.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from haf_grasping_amd import capi  # noqa: E402
import models  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
FEAT, RANGE = os.path.join(DATA, "Features.txt"), os.path.join(DATA, "range21062012_allfeatures")
SURROGATE = os.path.join(ROOT, "tests", "golden", "surrogate.model")
PARAMS = {"k32": dict(k=32), "k8": dict(k=8), "k1": dict(k=1), "k256_wide": dict(k=256, roll_window=2, min_dist_m=0.03)}


def workloads(tmp):
    model42 = os.path.join(tmp, "seed42.model")
    models.write_random_model(model42, 4096, D=323, seed=42, balanced=True)
    yield ("C5", dict(grid_h=512, grid_w=512, n_rolls=36, roll_step_deg=5, max_points=1 << 20), model42,
           models.synthetic_cloud(grid=512, k=2, seed=0), capi.default_input(grasp_area_length_x=512, grasp_area_length_y=512))
    yield ("C2", dict(max_points=1 << 18), SURROGATE, capi.load_pcd(os.path.join(DATA, "pcd2.pcd")),
           capi.default_input(grasp_area_length_x=32, grasp_area_length_y=32))
    yield ("C3", dict(n_rolls=20, roll_step_deg=9, max_points=1 << 18), SURROGATE,
           capi.load_pcd(os.path.join(DATA, "table1_mult_obj_rcs_1428580506606673.pcd")),
           capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    calls = 5 if a.trace_only else max(50, a.calls)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, cfg, model, xyz, inp in workloads(tmp):
            eng = capi.Engine(FEAT, RANGE, model, **cfg)
            out = eng.score(xyz, inp)
            t0 = time.perf_counter()
            first = eng.top_grasps(k=32)
            first_ms = 1e3 * (time.perf_counter() - t0)          # includes the lazy allocation of the scratch
            row = dict(best_vote=out["best_vote"], n_evals=out["n_evals"], first_call_ms=first_ms, found_k32=len(first[0]))
            for pname, p in PARAMS.items():
                eng.top_grasps(**p)
                ts = []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    got = eng.top_grasps(**p)
                    ts.append(time.perf_counter() - t0)
                row[pname] = dict(ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)), found=len(got[0]))
            eng.close()
            res[name] = row
            print(name, json.dumps(row), flush=True)
    if a.out and not a.trace_only:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
        res["build"] = dict(commit=commit, lib_mtime=os.path.getmtime(capi.LIB_PATH), calls=calls)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
