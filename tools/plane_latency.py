#!/usr/bin/env python3
"""What fitting the support plane costs: haf_fit_plane on the device against haf_fit_plane_ref, the same definition on one host
thread, and the whole chain fit -> segment -> score under the image -> best grasp per object with the device fit and with the host fit.

table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad; the library's
default parameters (tol 5 mm, 256 hypotheses); the segmentation over the fitted plane with min_height 0.03, max_gap 0.02, min_pixels 50.
After a warm-up, the host wall clock of synchronised calls through the Python binding, the variants alternating within one run so that
drift hits them alike:
  host_ref       haf_fit_plane_ref: the BASELINE, what a caller without the device call runs (one host thread)
  host_frame     haf_fit_plane, host frame (staged and uploaded by the call)
  device_frame   haf_fit_plane, device-resident frame
  chain_device   haf_fit_plane + haf_segment_frame over its plane (engine image) + haf_score_frames_roi under that image +
                 haf_grasp_map_labels on it
  chain_host     the same chain with haf_fit_plane_ref in the first place
On a GPU box:
  python tools/plane_latency.py --calls 200 --out profiles/plane_fit_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o plane -- python tools/plane_latency.py --trace-only device_frame
                    # the kernels' own times; then hand the run's stats to the measuring run:
  python tools/plane_latency.py --kernel-stats DIR/.../plane_kernel_stats.csv --out profiles/plane_fit_time.json
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
    """{kernel: calls, avg / min / max us} of the plane kernels from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_plane_\w+(<[^>]*>)?)", r["Name"])
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
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 20)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
params = capi.plane_params()
over_fit = dict(min_height=0.03, max_gap=0.02, min_pixels=50)
inp = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)
seen, picks = {}, {}


def key_of(fit):
    return (fit["plane"].tobytes(), fit["n_inliers"], fit["winner"], tuple(fit["stats"]))


def host_ref():
    seen["host_ref"] = key_of(capi.fit_plane_ref(frame, params))


def host_frame():
    seen["host_frame"] = key_of(eng.fit_plane(frame, params))


def device_frame():
    seen["device_frame"] = key_of(eng.fit_plane(d_frame, params))


def chain(fit, name):
    seen[name] = key_of(fit)
    img, infos, st = eng.segment(frame, capi.segment_params(plane=fit["plane"], **over_fit), device_out=True)
    eng.score_frames_roi([frame], [(img.data, img.row_stride_bytes)], [inp])
    picks[name] = eng.best_per_label(0, frame, img, n_labels=len(infos))["picks"].tobytes()


def chain_device():
    chain(eng.fit_plane(frame, params), "chain_device")


def chain_host():
    chain(capi.fit_plane_ref(frame, params), "chain_host")


variants = {"host_ref": host_ref, "host_frame": host_frame, "device_frame": device_frame, "chain_device": chain_device, "chain_host": chain_host}
if a.trace_only:
    variants = {a.trace_only: variants[a.trace_only]}
for call in variants.values():
    call()
assert len(set(seen.values())) == 1 and len(set(picks.values())) <= 1, seen      # the routes fit the same plane and pick the same grasps
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
host = {key: stats(t) for key, t in times.items()}
for key, base in (("host_frame", "host_ref"), ("device_frame", "host_ref"), ("chain_device", "chain_host")):
    host[key]["below_%s_by_more_than_its_spread" % base] = bool(host[base]["median_us"] - host[key]["median_us"] > host[base]["spread_p10_p90_us"])
fit = capi.fit_plane_ref(frame, params)
doc = {"tool": "tools/plane_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "table1 from camera A as a 640 x 480 U16 frame; tol 0.005, 256 hypotheses; the chains segment over the fitted plane (min_height 0.03, max_gap 0.02, min_pixels 50) and score a 56 x 56 grid, 20 rolls",
       "fit": dict(plane=[float(x) for x in fit["plane"]], n_inliers=fit["n_inliers"], rms=fit["rms"], stats=fit["stats"]), "host_us": host}
hip.hipFree(d_frame.data)
eng.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only device_frame run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
