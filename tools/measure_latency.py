#!/usr/bin/env python3
"""What measuring the objects costs: haf_measure_labels on the device against haf_measure_labels_ref, the same definition on one host
thread, and the per-object flow on top of it against the route a caller had before it.

table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad; the support plane
fitted with the library's defaults, the segmentation over it with min_height 0.03, max_gap 0.02, min_pixels 50; a goal whose grid
leaves most objects out.  After a warm-up, the host wall clock of synchronised calls through the Python binding, the variants
alternating within one run so that drift hits them alike:
  host_ref         haf_measure_labels_ref: the BASELINE, what a caller without the device call runs (one host thread)
  host_host        haf_measure_labels, host frame and host label image (both staged and uploaded by the call)
  device_device    haf_measure_labels, device-resident frame and the label image haf_segment_frame left in the engine
  flow_per_object  CalcGraspPointsServer.execute_frame_per_object: segment, measure, one batched ROI request per chunk of objects, one
                   label call per object
  flow_sequential  the route before it: segment into a host image, the shapes and the requests from haf_measure_labels_ref and
                   haf_object_input on the host, then per object ONE execute_frame under the mask and ONE best_per_object
On a GPU box:
  python tools/measure_latency.py --calls 200 --out profiles/label_shape_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o shape -- python tools/measure_latency.py --trace-only device_device
                    # the kernel's own time; then hand the run's stats to the measuring run:
  python tools/measure_latency.py --kernel-stats DIR/.../shape_kernel_stats.csv --out profiles/label_shape_time.json
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
ap.add_argument("--flow-calls", type=int, default=20, help="calls of the two flows (each is a dozen requests)")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default="")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", default="", metavar="CSV", help="the *_kernel_stats.csv of such a run")
a = ap.parse_args()

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg, capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of k_label_shape from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_label_shape(<[^>]*>)?)", r["Name"])
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
                            n_rolls=20, roll_step_deg=9, max_points=1 << 22, max_clouds=8)
eng = srv.engine
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)
fit = capi.fit_plane_ref(frame)
sp = capi.segment_params(plane=fit["plane"], min_height=0.03, max_gap=0.02, min_pixels=50)
plane = list(sp.plane)
labels, infos, _ = capi.segment_ref(frame, sp)
n = len(infos)
goal = GraspInputMsg(grasp_area_center=(0.06, 0.45, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
seen, flows = {}, {}


def host_ref():
    seen["host_ref"] = capi.measure_labels_ref(frame, labels, n, plane).tobytes()


def host_host():
    seen["host_host"] = eng.measure_labels(frame, labels, n, plane).tobytes()


def device_device():
    seen["device_device"] = eng.measure_labels(d_frame, d_image, n, plane).tobytes()


def flow_per_object():
    flows["flow_per_object"] = [(o[0], o[1], o[2], o[3]) for o in srv.execute_frame_per_object(goal, frame, sp)]


def flow_sequential():
    lab, inf, _ = eng.segment(frame, sp)                  # the image comes to the host
    shapes = capi.measure_labels_ref(frame, lab, len(inf), plane)
    mask, base, out = (lab != 0).astype(np.uint8), goal.to_c(), []
    for l in range(len(inf)):
        if not shapes["found"][l]:
            continue
        inp, _ = capi.object_input(eng.cfg, base, shapes[l], 4)
        g = GraspInputMsg(grasp_area_center=tuple(inp.grasp_area_center), grasp_area_length_x=inp.grasp_area_length_x, grasp_area_length_y=inp.grasp_area_length_y)
        srv.execute_frame(g, frame, roi_mask=mask)
        res = eng.best_per_label(0, frame, lab, n_labels=len(inf))
        if res["picks"]["found"][l]:
            p, c = res["picks"][l], res["poses"][l]
            out.append(((-int(p["vote"]), int(p["roll"]), int(p["v"]) * W + int(p["u"])), l + 1, c, int(p["u"]), int(p["v"])))
    flows["flow_sequential"] = [(l, c["eval"], u, v) for _, l, c, u, v in sorted(out, key=lambda t: t[0])]


d_image = eng.segment(d_frame, sp, device_out=True)[0]      # (the flows segment the same frame again: the engine's image keeps these labels)
variants = {"host_ref": host_ref, "host_host": host_host, "device_device": device_device}
slow = {"flow_per_object": flow_per_object, "flow_sequential": flow_sequential}
if a.trace_only:
    variants, slow = ({a.trace_only: variants[a.trace_only]}, {}) if a.trace_only in variants else ({}, {a.trace_only: slow[a.trace_only]})
for call in list(variants.values()) + list(slow.values()):
    call()
assert len(set(seen.values())) <= 1, "the routes measure different shapes"
if len(flows) == 2:                                       # the two flows pick the same grasps
    assert [(o[0], o[1].eval, o[2], o[3]) for o in flows["flow_per_object"]] == flows["flow_sequential"], flows
for _ in range(a.warmup):
    for call in variants.values():
        call()
times = {key: [] for key in list(variants) + list(slow)}
for _ in range(a.calls):
    for key, call in variants.items():
        t0 = time.perf_counter_ns()
        call()
        times[key].append(time.perf_counter_ns() - t0)
for _ in range(a.flow_calls if slow else 0):
    for key, call in slow.items():
        t0 = time.perf_counter_ns()
        call()
        times[key].append(time.perf_counter_ns() - t0)
if a.trace_only:
    srv.close()
    sys.exit(0)
host = {key: stats(t) for key, t in times.items()}
for key, base in (("host_host", "host_ref"), ("device_device", "host_ref"), ("flow_per_object", "flow_sequential")):
    host[key]["below_%s_by_more_than_its_spread" % base] = bool(host[base]["median_us"] - host[key]["median_us"] > host[base]["spread_p10_p90_us"])
shapes = capi.measure_labels_ref(frame, labels, n, plane)
doc = {"tool": "tools/measure_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds; the flows %d calls each)" % (a.calls, a.warmup, a.flow_calls),
       "request": "table1 from camera A as a 640 x 480 U16 frame; segmented over the fitted plane (min_height 0.03, max_gap 0.02, min_pixels 50); the flows score 56 x 56 grids, 20 rolls, goal centre (0.06, 0.45, 0)",
       "objects": dict(n_labels=n, labelled_pixels=int(shapes["n_pixels"].sum()), grasps_of_the_flow=len(flows.get("flow_per_object", [])),
                       narrow_width_m=[round(float(x), 4) for x in shapes["narrow_width"]], diameter_m=[round(float(x), 4) for x in shapes["diameter"]]),
       "host_us": host}
hip.hipFree(d_frame.data)
srv.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only device_device run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
