#!/usr/bin/env python3
"""What conditioning a depth image costs: haf_filter_depth on the device against haf_filter_depth_ref, the same rules on the host.

table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad -- with 1 mm of
uniform noise per exposure and 2 % drop-outs; stacks of N = 1, 3 and 8 exposures, the default parameters (radius 2, support 6).  After a
warm-up, the host wall clock of synchronised calls, the variants alternating within one run so that drift hits them alike:
  host_ref         haf_filter_depth_ref: the BASELINE, what a caller without the device call runs (one host thread)
  host_to_host     haf_filter_depth, host exposures, host output image
  host_to_engine   haf_filter_depth, host exposures, the engine's own device image (what haf_score_frames then reads)
  device_to_engine haf_filter_depth, device-resident exposures, the engine's own device image
On a GPU box:
  python tools/filter_latency.py --calls 200 --out profiles/depth_filter_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o filt -- python tools/filter_latency.py --trace-only device_to_engine --stacks 3
                    # the kernel's own time; then hand the run's stats to the measuring run:
  python tools/filter_latency.py --kernel-stats DIR/.../filt_kernel_stats.csv --out profiles/depth_filter_time.json
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
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--stacks", default="1,3,8", help="the stack sizes N to measure")
ap.add_argument("--out", default="")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", default="", metavar="CSV", help="the *_kernel_stats.csv of such a run")
a = ap.parse_args()

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the filter kernel from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_depth_filter<[^>]*>)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def device_array(hip, arr):
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), arr.nbytes) != 0 or hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy failed")
    return p.value


xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
pose = tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9))
depth = render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
rng = np.random.default_rng(1)
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 22)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
params = capi.depth_filter()

doc = {"tool": "tools/filter_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "table1 from camera A as 640 x 480 U16 exposures (1 mm uniform noise, 2 % drop-outs each), default parameters: radius 2, support 6, 0.004 + 0.01 z, min_valid 1",
       "stacks": {}}
for n in [int(x) for x in a.stacks.split(",")]:
    exposures = []
    for _ in range(n):
        img = depth.copy()
        img[img > 0] += rng.integers(0, 2, int((img > 0).sum())).astype(np.uint16)
        img[rng.random(img.shape) < 0.02] = 0
        exposures.append(img)
    frames = [capi.depth_frame(img, sensor_to_base=pose, **K) for img in exposures]
    d_frames = [capi.depth_frame(device_array(hip, img), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K) for img in exposures]
    host_image = np.empty((H, W), np.uint16)
    seen = {}

    def host_ref():
        seen["host_ref"] = capi.filter_depth_ref(frames, params, out=host_image)[1]

    def host_to_host():
        seen["host_to_host"] = eng.filter_depth(frames, params, host_out=host_image)[1]

    def host_to_engine():
        seen["host_to_engine"] = eng.filter_depth(frames, params)[1]

    def device_to_engine():
        seen["device_to_engine"] = eng.filter_depth(d_frames, params)[1]

    variants = {"host_ref": host_ref, "host_to_host": host_to_host, "host_to_engine": host_to_engine, "device_to_engine": device_to_engine}
    if a.trace_only:
        variants = {a.trace_only: variants[a.trace_only]}
    for call in variants.values():
        call()
    assert len({tuple(s) for s in seen.values()}) == 1, seen                     # the four routes count the same pixels
    for _ in range(a.warmup):
        for call in variants.values():
            call()
    times = {key: [] for key in variants}
    for _ in range(a.calls):
        for key, call in variants.items():
            t0 = time.perf_counter_ns()
            call()
            times[key].append(time.perf_counter_ns() - t0)
    for f in d_frames:
        hip.hipFree(f.data)
    if a.trace_only:
        continue
    host = {key: stats(t) for key, t in times.items()}
    base = host["host_ref"]
    for key in host:
        if key != "host_ref":
            host[key]["below_baseline_by_more_than_its_spread"] = bool(base["median_us"] - host[key]["median_us"] > base["spread_p10_p90_us"])
    doc["stacks"][str(n)] = {"stats": [int(x) for x in seen["host_ref"]], "host_us": host}
eng.close()
if a.trace_only:
    sys.exit(0)
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only device_to_engine run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
