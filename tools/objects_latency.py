#!/usr/bin/env python3
"""What the fused per-object call saves: CalcGraspPointsServer.execute_frame_per_object with fused=False (one haf_score_frames_roi batch
per chunk under the mask `labels != 0`, one haf_grasp_map_labels call per object) against fused=True (one haf_score_objects call per
chunk), on the same frame, the same goal and the same server.

table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad; the support plane
fitted with the library's defaults, the segmentation over it with min_height 0.03, max_gap 0.02, min_pixels 50; the far goal whose grid
leaves most objects out (centre (0.06, 0.45, 0), 56 x 56 cells).  After a warm-up, the host wall clock of whole flows through the Python
binding (segment, measure, requests, picks), the variants alternating within one run so that drift hits them alike:
  unfused_host    fused=False, host frame: the BASELINE (the frame staged and deprojected once per request of a chunk)
  fused_host      fused=True,  host frame
  unfused_device  fused=False, device-resident frame: the baseline of the device pair
  fused_device    fused=True,  device-resident frame
No speed-up is fixed in advance: a gain is claimed only where the difference of the medians exceeds the baseline's own p10-p90 width.
On a GPU box:
  python tools/objects_latency.py --calls 40 --out profiles/score_objects_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o objects -- python tools/objects_latency.py --trace-only fused_host
                    # the kernels' own times; then hand the run's stats to the measuring run:
  python tools/objects_latency.py --kernel-stats DIR/.../objects_kernel_stats.csv --out profiles/score_objects_time.json
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
ap.add_argument("--calls", type=int, default=40, help="flows per variant (each is a dozen requests)")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--max-clouds", type=int, default=8)
ap.add_argument("--out", default="")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", default="", metavar="CSV", help="the *_kernel_stats.csv of such a run")
a = ap.parse_args()

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg, capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)
KERNELS = r"\b((k_roi_mark_objects|k_map_labels_objects|k_object_records|k_roi_mark|k_map_labels|k_label_records|k_frame_points)(<[^>]*>)?)"


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the kernels the two routes differ in, from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(KERNELS, r["Name"])
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
srv = CalcGraspPointsServer(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                            n_rolls=20, roll_step_deg=9, max_points=1 << 22, max_clouds=a.max_clouds)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)
sp = capi.segment_params(plane=capi.fit_plane_ref(frame)["plane"], min_height=0.03, max_gap=0.02, min_pixels=50)
goal = GraspInputMsg(grasp_area_center=(0.06, 0.45, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
flows = {}


def flow(key, fr, fused):
    def call():
        flows[key] = srv.execute_frame_per_object(goal, fr, sp, fused=fused)
    return call


variants = {"unfused_host": flow("unfused_host", frame, False), "fused_host": flow("fused_host", frame, True),
            "unfused_device": flow("unfused_device", d_frame, False), "fused_device": flow("fused_device", d_frame, True)}
if a.trace_only:
    variants = {a.trace_only: variants[a.trace_only]}
for call in variants.values():
    call()
first = next(iter(flows.values()))
assert all(f == first for f in flows.values()), "the routes pick different grasps"
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
    srv.close()
    sys.exit(0)
host = {key: stats(t) for key, t in times.items()}
for key, base in (("fused_host", "unfused_host"), ("fused_device", "unfused_device")):
    diff = host[base]["median_us"] - host[key]["median_us"]
    host[key]["baseline"] = base
    host[key]["median_below_baseline_us"] = diff
    host[key]["below_baseline_by_more_than_its_spread"] = bool(diff > host[base]["spread_p10_p90_us"])
doc = {"tool": "tools/objects_latency.py: host wall clock of whole execute_frame_per_object flows through the Python binding, variants alternating within one run (%d flows each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "table1 from camera A as a 640 x 480 U16 frame; segmented over the fitted plane (min_height 0.03, max_gap 0.02, min_pixels 50); 56 x 56 grids, 20 rolls, goal centre (0.06, 0.45, 0), max_clouds %d" % a.max_clouds,
       "objects": dict(n_labels=len(srv.last_segment_infos), requests=int(srv.last_shapes["found"].sum()), grasps_of_the_flow=len(first)),
       "rule": "a gain is claimed only where the unfused median minus the fused median exceeds the unfused route's own p10-p90 width",
       "host_us": host}
hip.hipFree(d_frame.data)
srv.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
