#!/usr/bin/env python3
"""What the gripper's clearance costs: haf_check_grasps on the device against haf_check_grasps_ref, the same definition on one host
thread.

table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad; the C3 request on
it (56 x 56 grid, 20 rolls); the candidates of haf_top_grasps with k = 32 and with k = 1024 -- and, because its suppression leaves
this scene only a few dozen, with k = 1024, min_vote 1 and the suppression off -- handed over as haf_grasp_candidate arrays built once; the library's default (nominal) gripper.  After a warm-up, the host wall clock of synchronised calls through the Python
binding, the variants alternating within one run so that drift hits them alike -- per candidate set:
  host_ref       haf_check_grasps_ref: the BASELINE, what a caller without the device call runs (one host thread)
  host_frame     haf_check_grasps, host frame (staged and uploaded again by the call: that cost is shown, not hidden)
  device_frame   haf_check_grasps, device-resident frame
On a GPU box:
  python tools/clearance_latency.py --calls 200 --out profiles/grasp_clearance_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o clear -- python tools/clearance_latency.py --trace-only device_frame
                    --set k32        # the two kernels' own times, one trace per candidate set; then hand the stats to the measuring run:
  python tools/clearance_latency.py --kernel-stats k32=DIR/.../clear_kernel_stats.csv --out profiles/grasp_clearance_time.json
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
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default="")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone (both candidate sets) and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--set", default="", metavar="k32|k1024|k1024_unsuppressed", help="this candidate set alone (with --trace-only: one trace per set)")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="SET=CSV", help="the *_kernel_stats.csv of such a run of that set; may be given once per set")
a = ap.parse_args()

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)
POSE_FIELDS = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector")


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the clearance kernels from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_clear_points(<[^>]*>)?|k_grasp_clear)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def device_array(hip, arr):
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), arr.nbytes) != 0 or hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy failed")
    return p.value


def candidate_array(cands):
    arr = (capi.GraspCandidate * len(cands))()
    for c, d in zip(arr, cands):
        for f in POSE_FIELDS:
            setattr(c.grasp, f, (C.c_double * 3)(*d[f]))
    return arr


xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
pose = tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9))
depth = render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 20)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
inp = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)
gripper = capi.gripper()
eng.score_frames([frame], [inp])
# (the suppression of haf_top_grasps leaves this scene a few dozen candidates whatever k is: the third set switches it off, to show a long list)
sets = {"k32": candidate_array(eng.top_grasps(k=32)[0]), "k1024": candidate_array(eng.top_grasps(k=1024)[0]),
        "k1024_unsuppressed": candidate_array(eng.top_grasps(k=1024, min_vote=1, cell_radius=0, roll_window=0, min_dist_m=0.0)[0])}
if a.set:
    sets = {a.set: sets[a.set]}
seen = {}


def key_of(result):
    rows, order = result
    return rows.tobytes() + order.tobytes()


routes = {"host_ref": lambda c: capi.check_grasps_ref(frame, c, gripper), "host_frame": lambda c: eng.check_grasps(frame, c, gripper),
          "device_frame": lambda c: eng.check_grasps(d_frame, c, gripper)}
if a.trace_only:
    routes = {a.trace_only: routes[a.trace_only]}
variants = {(route, name): (lambda call=call, cands=cands: call(cands)) for name, cands in sets.items() for route, call in routes.items()}
for (route, name), call in variants.items():
    seen.setdefault(name, set()).add(key_of(call()))
assert all(len(v) == 1 for v in seen.values()), "the routes give the same rows"
for _ in range(a.warmup):
    for call in variants.values():
        call()
times = {key: [] for key in variants}
for _ in range(a.calls):
    for key, call in variants.items():
        t0 = time.perf_counter_ns()
        call()
        times[key].append(time.perf_counter_ns() - t0)
if a.trace_only:
    eng.close()
    sys.exit(0)
host = {}
for name, cands in sets.items():
    rows, order = capi.check_grasps_ref(frame, cands, gripper)
    block = {route: stats(times[route, name]) for route in routes}
    for route in ("host_frame", "device_frame"):
        block[route]["below_host_ref_by_more_than_its_spread"] = bool(block["host_ref"]["median_us"] - block[route]["median_us"] > block["host_ref"]["spread_p10_p90_us"])
    host[name] = dict(n_grasps=len(cands), n_free=int(order.size), near_points_per_grasp=float(rows["n_near"].mean()), host_us=block)
doc = {"tool": "tools/clearance_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "table1 from camera A as a 640 x 480 U16 frame; candidates of haf_top_grasps(k = 32 / 1024, and k = 1024 with min_vote 1 and no suppression) of the C3 request (56 x 56 grid, 20 rolls) as haf_grasp_candidate arrays built once; the default nominal gripper",
       "not_measured": "other frame kinds and sizes, a mask, the cost of building the candidate array from Python dicts, more than one host thread for the baseline",
       "sets": host}
hip.hipFree(d_frame.data)
eng.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict({spec.split("=", 1)[0]: kernel_stats(spec.split("=", 1)[1]) for spec in a.kernel_stats},
                                  note="rocprofv3 --kernel-trace --stats of a --trace-only device_frame --set run per candidate set (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
