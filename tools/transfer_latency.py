#!/usr/bin/env python3
"""What carrying another camera's label image over to a depth frame costs: haf_transfer_labels on the device against
haf_transfer_labels_ref, the same definition on one host thread.

table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad -- and the label
image of camera B -- 0.85 m above (0.04, 0.34), tilted by (-0.25, 0.20, -0.8) rad, the same intrinsics: that view's own pixel
segmentation (plane z = 0, min_height 0.03), the stand-in for an instance segmenter's output; default transfer parameters.  After a
warm-up, the host wall clock of synchronised calls through the Python binding, the variants alternating within one run so that drift
hits them alike:
  frame_host         haf_transfer_labels, the host frame and the host label image, into the engine's own device image
  frame_device       haf_transfer_labels, the frame and the label image device-resident, into the engine's own device image
  frame_ref          haf_transfer_labels_ref: the BASELINE of both, what a caller without the device call runs
On a GPU box:
  python tools/transfer_latency.py --calls 200 --out profiles/transfer_labels_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o transfer -- python tools/transfer_latency.py --trace-only frame_device
                    # the kernels' own times; then hand the run's stats to the measuring run:
  python tools/transfer_latency.py --kernel-stats DIR/.../transfer_kernel_stats.csv --out profiles/transfer_labels_time.json
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
    """{kernel: calls, avg / min / max us} of the call's kernels from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_transfer_\w+(<[^>]*>)?)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def device_array(hip, arr):
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), arr.nbytes) != 0 or hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy failed")
    return p.value


xyz = np.ascontiguousarray(pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))[:, :3], np.float32)
pose_a, pose_b = tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9)), tilted_pose((-0.25, 0.20, -0.8), (0.04, 0.34, 0.85))
depth = render_depth(xyz, pose_a, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
frame_b = capi.depth_frame(render_depth(xyz, pose_b, W, H, K["fx"], K["fy"], K["cx"], K["cy"]), sensor_to_base=pose_b, **K)
labels, infos, _ = capi.segment_ref(frame_b, capi.segment_params(plane=[0, 0, 1, 0], min_height=0.03))
n_labels = max(1, len(infos))
cam = capi.camera(W, H, K["fx"], K["fy"], K["cx"], K["cy"], sensor_to_base=pose_b)
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 20)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
params = capi.transfer_params()
frame = capi.depth_frame(depth, sensor_to_base=pose_a, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose_a, **K)
d_labels = (device_array(hip, labels), 1, W)
image = np.empty((H, W), np.uint8)
seen = {}


def v_frame_host():
    seen["frame_host"] = eng.transfer_labels(frame, cam, labels, n_labels, params, device_out=True)[1]


def v_frame_device():
    seen["frame_device"] = eng.transfer_labels(d_frame, cam, d_labels, n_labels, params, device_out=True)[1]


def v_frame_ref():
    seen["frame_ref"] = capi.transfer_labels_ref(frame, cam, labels, n_labels, params, out=image)[1]


variants = {"frame_host": v_frame_host, "frame_device": v_frame_device, "frame_ref": v_frame_ref}
if a.trace_only:
    variants = {a.trace_only: variants[a.trace_only]}
for call in variants.values():
    call()
if not a.trace_only:                                      # the device sees what the definition sees
    assert seen["frame_host"] == seen["frame_device"] == seen["frame_ref"], seen
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
for key in ("frame_host", "frame_device"):
    host[key]["below_frame_ref_by_more_than_its_spread"] = bool(host["frame_ref"]["median_us"] - host[key]["median_us"] > host["frame_ref"]["spread_p10_p90_us"])
doc = {"tool": "tools/transfer_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "table1 from camera A as a 640 x 480 U16 frame; the labels of camera B's own pixel segmentation (640 x 480 uint8, %d labels; plane z = 0, min_height 0.03); near_m 0.05, tol_abs 0.01, tol_rel 0.01, splat 1; into the engine's own uint8 image" % n_labels,
       "stats": {"frame_ref": [int(x) for x in seen["frame_ref"]]}, "host_us": host}
hip.hipFree(d_frame.data)
hip.hipFree(d_labels[0])
eng.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only frame_device run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
