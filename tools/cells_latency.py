#!/usr/bin/env python3
"""What clustering a cloud by top-down cells costs: haf_segment_cells on the device against haf_segment_cells_ref, the same definition on
one host thread, and against haf_segment_frame -- the pixel segmenter -- on the frame both can take.

table1 as the unorganised cloud of its .pcd (an N x 1 XYZ frame under the identity pose), and rendered as a 640 x 480 U16 frame from
camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad; plane z = 0 of the base frame, min_height 0.03, the default
1024 x 1024 grid of 1 cm cells, 8-connectivity, min_points 50.  After a warm-up, the host wall clock of synchronised calls through the
Python binding, the variants alternating within one run so that drift hits them alike:
  cloud              haf_segment_cells, the host cloud, the engine's own device image
  frame_host         haf_segment_cells, the rendered host frame, the engine's own device image
  frame_device       haf_segment_cells, the rendered frame device-resident, the engine's own device image
  cloud_ref          haf_segment_cells_ref on the cloud: the BASELINE of `cloud`, what a caller without the device call runs
  frame_ref          haf_segment_cells_ref on the rendered frame: the baseline of frame_host and frame_device
  pixels_host        haf_segment_frame on the rendered host frame (max_gap 0.02, min_pixels 50), the engine's own device image
On a GPU box:
  python tools/cells_latency.py --calls 200 --out profiles/cell_segment_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cells -- python tools/cells_latency.py --trace-only frame_device
                    # the kernels' own times; then hand the run's stats to the measuring run:
  python tools/cells_latency.py --kernel-stats DIR/.../cells_kernel_stats.csv --out profiles/cell_segment_time.json
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
            m = re.search(r"\b(k_(cell|segment)_\w+(<[^>]*>)?)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


def device_array(hip, arr):
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), arr.nbytes) != 0 or hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy failed")
    return p.value


xyz = np.ascontiguousarray(pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))[:, :3], np.float32)
pose = tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9))
depth = render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 20)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
params = capi.cell_segment_params(plane=[0, 0, 1, 0], min_height=0.03)
pixel_params = capi.segment_params(plane=[0, 0, 1, 0], min_height=0.03, max_gap=0.02, min_pixels=50)
cloud = capi.cloud_frame(xyz)
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)
cloud_image, frame_image = np.empty((1, len(xyz)), np.uint8), np.empty((H, W), np.uint8)
seen = {}


def v_cloud():
    seen["cloud"] = eng.segment_cells(cloud, params, device_out=True)[2]


def v_frame_host():
    seen["frame_host"] = eng.segment_cells(frame, params, device_out=True)[2]


def v_frame_device():
    seen["frame_device"] = eng.segment_cells(d_frame, params, device_out=True)[2]


def v_cloud_ref():
    seen["cloud_ref"] = capi.segment_cells_ref(cloud, params, out=cloud_image)[2]


def v_frame_ref():
    seen["frame_ref"] = capi.segment_cells_ref(frame, params, out=frame_image)[2]


def v_pixels_host():
    seen["pixels_host"] = eng.segment(frame, pixel_params, device_out=True)[2]


variants = {"cloud": v_cloud, "frame_host": v_frame_host, "frame_device": v_frame_device, "cloud_ref": v_cloud_ref, "frame_ref": v_frame_ref,
            "pixels_host": v_pixels_host}
if a.trace_only:
    variants = {a.trace_only: variants[a.trace_only]}
for call in variants.values():
    call()
if not a.trace_only:                                      # the device sees what the definition sees
    assert seen["cloud"] == seen["cloud_ref"] and seen["frame_host"] == seen["frame_device"] == seen["frame_ref"], seen
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
for key, base in (("cloud", "cloud_ref"), ("frame_host", "frame_ref"), ("frame_device", "frame_ref")):
    host[key]["below_%s_by_more_than_its_spread" % base] = bool(host[base]["median_us"] - host[key]["median_us"] > host[base]["spread_p10_p90_us"])
doc = {"tool": "tools/cells_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "table1 as its cloud of %d points and from camera A as a 640 x 480 U16 frame; plane z = 0, min_height 0.03, 1024 x 1024 cells of 1 cm, 8-connectivity, min_points 50; pixels_host: haf_segment_frame, max_gap 0.02, min_pixels 50" % len(xyz),
       "stats": {key: [int(x) for x in seen[key]] for key in ("cloud_ref", "frame_ref", "pixels_host")}, "host_us": host}
hip.hipFree(d_frame.data)
eng.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only frame_device run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
