#!/usr/bin/env python3
"""What a per-pixel grasp map of the last scored request costs (haf_grasp_map), next to what a caller had to do without it.

One 640 x 480 U16 depth frame, two engines: C3 (56 x 56 grid, 20 rolls of 9 degrees, surrogate model, the frame rendered from the
table1 cloud) and C5 (512 x 512, 36 rolls of 5 degrees, random 256-SV model, the frame rendered from the synthetic cloud 4 m below
the camera).  Each engine scores its cloud once; then, after a warm-up, the host wall clock of synchronised calls, the variants
alternating within one run so that drift hits them alike:
  map_host        haf_grasp_map, frame in host memory, the three images returned to host memory
  map_device      haf_grasp_map, frame resident in device memory, the three images left in device memory
  baseline        what a build without haf_grasp_map offers: R x haf_get_roll_grid, then haf_grasp_map_ref on the host (the
                  transform of every pixel under every roll and R gathers per pixel)
  baseline_ref    haf_grasp_map_ref alone on grids fetched before (the host arithmetic without the R device reads)
On a GPU box:
  python tools/grasp_map_latency.py --calls 200 --out profiles/grasp_map_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/c3 -o map -- python tools/grasp_map_latency.py --trace-only --configs c3
                  # the kernel's own time (map_device calls only), one run per config; then hand the runs' stats to the measuring run:
  python tools/grasp_map_latency.py --kernel-stats c3=DIR/c3/.../map_kernel_stats.csv --kernel-stats c5=... --out profiles/grasp_map_time.json
From the kernel's time the JSON derives the achieved bytes per second against the floor DESIGN.md 5 states: the pixel read (2 bytes),
the three images written (8 bytes) and R two-byte gathers per pixel.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--baseline-calls", type=int, default=20, help="the host baseline takes tens of milliseconds: fewer calls of it")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default="")
ap.add_argument("--trace-only", action="store_true", help="map_device alone on both engines, nothing written: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="CONFIG=CSV", help="the *_kernel_stats.csv of such a run with --configs CONFIG")
ap.add_argument("--configs", default="c3,c5")
a = ap.parse_args()

import models  # noqa: E402
import pcdio  # noqa: E402
from render import render_depth  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
FEAT, RNG = os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def setup(name):
    if name == "c3":
        cfg = dict(n_rolls=20, roll_step_deg=9)
        inp = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
        xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
        pose = np.array([1, 0, 0, 0.13, 0, -1, 0, 0.2, 0, 0, -1, 0.9], np.float32)
        model = os.path.join(ROOT, "tests", "golden", "surrogate.model")
        what = "C3: 56 x 56 grid, 20 rolls x 9 deg, surrogate model, table1 from 0.9 m above (0.13, 0.2)"
    else:
        cfg = dict(grid_h=512, grid_w=512, n_rolls=36, roll_step_deg=5)
        inp = capi.default_input(grasp_area_length_x=512, grasp_area_length_y=512)
        xyz = models.synthetic_cloud(grid=512, k=2, seed=0)
        pose = np.array([1, 0, 0, 0.0, 0, -1, 0, 0.0, 0, 0, -1, 4.0], np.float32)
        import tempfile
        model = os.path.join(tempfile.mkdtemp(prefix="haf_map_"), "rand256.model")
        models.write_random_model(model, 256, seed=4, balanced=True)
        what = "C5: 512 x 512 grid, 36 rolls x 5 deg, random 256-SV model, the synthetic cloud from 4 m above its centre"
    depth = render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
    eng = capi.Engine(FEAT, RNG, model, max_points=1 << 20, **cfg)
    out = eng.score(xyz, inp)
    return eng, inp, depth, capi.depth_frame(depth, sensor_to_base=pose, **K), out, what


hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def dev_alloc(nbytes, src=None):
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), nbytes) != 0 or (src is not None and hip.hipMemcpy(p, src.ctypes.data, nbytes, 1) != 0) or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy failed")
    return p


doc = {"tool": "tools/grasp_map_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each, %d of the "
               "baselines, after %d warm-up rounds)" % (a.calls, a.baseline_calls, a.warmup),
       "frame": "640 x 480 U16, f = 525", "library": os.path.relpath(capi.LIB_PATH, ROOT), "configs": {}}
for name in a.configs.split(","):
    eng, inp, depth, frame, out, what = setup(name)
    R, n = eng.cfg.n_rolls, W * H
    gH, gW = eng.cfg.grid_h, eng.cfg.grid_w
    d_frame = capi.Frame.from_buffer_copy(frame)
    d_pix = dev_alloc(depth.nbytes, depth)
    d_frame.data, d_frame.on_device = d_pix.value, 1
    d_out = dict(vote=dev_alloc(2 * n).value, roll=dev_alloc(2 * n).value, cell=dev_alloc(4 * n).value)
    grids = np.empty((R, gH, gW), np.float32)

    def fetch_grids():
        for r in range(R):
            eng._check(eng._L.haf_get_roll_grid(eng._h, 0, r, grids[r].ctypes.data, None))

    def baseline():
        fetch_grids()
        return capi.grasp_map_ref(eng.cfg, inp, 0, grids, frame)

    variants = {"map_host": lambda: eng.grasp_map(0, frame), "map_device": lambda: eng.grasp_map(0, d_frame, device_out=d_out),
                "baseline": baseline, "baseline_ref": lambda: capi.grasp_map_ref(eng.cfg, inp, 0, grids, frame)}
    if a.trace_only:
        for _ in range(a.warmup + a.calls):
            variants["map_device"]()
        eng.close()
        continue
    got, want = variants["map_host"](), variants["baseline"]()
    assert all((got[k] == want[k]).all() for k in want), name                  # the two routes compute the same map
    for _ in range(a.warmup):
        variants["map_host"]()
        variants["map_device"]()
    times = {k: [] for k in variants}
    for i in range(a.calls):
        for k, call in variants.items():
            if k.startswith("baseline") and i >= a.baseline_calls:
                continue
            t0 = time.perf_counter_ns()
            call()
            times[k].append(time.perf_counter_ns() - t0)
    eng.close()
    host = {k: stats(t) for k, t in times.items()}
    doc["configs"][name] = {"request": what, "n_evals": out["n_evals"], "best_vote": out["best_vote"], "rolls": R, "pixels": n,
                            "pixels_with_a_cell": int((got["roll"] >= 0).sum()), "pixels_with_a_positive_vote": int((got["vote"] > 0).sum()),
                            "host_us": host, "floor_bytes": n * (2 + 8 + 2 * R),
                            "baseline_over_map_host": host["baseline"]["median_us"] / host["map_host"]["median_us"],
                            "map_host_beats_baseline": bool(host["map_host"]["median_us"] < host["baseline"]["median_us"])}
if a.trace_only:
    sys.exit(0)
for spec in a.kernel_stats:
    import csv
    name, _, path = spec.partition("=")
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "k_grasp_map" in r["Name"] and name in doc["configs"]:
                c = doc["configs"][name]
                c["kernel_trace_us"] = dict(kernel=r["Name"].split("(")[0].strip(), calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3,
                                            min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3,
                                            note="rocprofv3 --kernel-trace --stats of a --trace-only run of this config (map_device calls)")
                c["achieved_GBps_against_floor_bytes"] = c["floor_bytes"] / (float(r["AverageNs"]) * 1e-9) / 1e9
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
