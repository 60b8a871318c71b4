#!/usr/bin/env python3
"""What "one grasp per object" costs: L calls of haf_grasp_map_best with the masks labels == l, against ONE haf_grasp_map_labels.

C3 (56 x 56 grid, 20 rolls of 9 degrees, surrogate model), table1 rendered as a 640 x 480 U16 frame from camera A -- 0.9 m above
(0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad -- scored once with haf_score_frames.  Two label layouts, L = 1, 8 and 48 each: "strips"
cuts the frame into L vertical strips of equal width (labels 1..L, no background); "sparse10" keeps those strips in rows 216..263 only
(48 of 480 rows: 10 % object pixels, the rest background -- the case the kernel's background early-out is for).  After a warm-up, the host wall clock of synchronised calls, the
variants alternating within one run so that drift hits them alike:
  best_per_mask    L x haf_grasp_map_best(labels == l): the BASELINE, the only route without the label call
  labels_host      one haf_grasp_map_labels, host frame and host labels
  labels_device    one haf_grasp_map_labels, device-resident frame and labels
On a GPU box:
  python tools/label_latency.py --calls 200 --out profiles/label_best_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o lab -- python tools/label_latency.py --trace-only labels_host --labels 48
                    # the kernels' own time; then hand the run's stats to the measuring run:
  python tools/label_latency.py --kernel-stats DIR/.../lab_kernel_stats.csv --out profiles/label_best_time.json
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
ap.add_argument("--labels", default="1,8,48", help="the label counts L to measure")
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
    """{kernel: calls, avg / min / max us} of the map and label kernels from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_map_labels<[^>]*>|k_label_records|k_grasp_map<[^>]*>|k_map_best|k_cell_record)", r["Name"])
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
inp = capi.default_input(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
eng.score_frames([frame], [inp])
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)

doc = {"tool": "tools/label_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": "C3: 56 x 56 grid, 20 rolls x 9 deg, surrogate model, table1 from camera A as a 640 x 480 U16 frame; labels: L vertical strips over the whole frame (strips) or over rows 216..263 only (sparse10)",
       "labels": {}}
for layout, n_labels in [(lay, int(x)) for lay in ("strips", "sparse10") for x in a.labels.split(",")]:
    dt = np.uint8 if n_labels < 256 else np.uint16
    labels = np.ascontiguousarray(np.broadcast_to((np.arange(W) * n_labels // W + 1).astype(dt), (H, W)))
    if layout == "sparse10":
        labels[:216] = 0
        labels[264:] = 0
    masks = [np.ascontiguousarray((labels == l).astype(np.uint8)) for l in range(1, n_labels + 1)]
    d_labels = (device_array(hip, labels), labels.itemsize, W * labels.itemsize)
    seen = {}

    def best_per_mask():
        seen["best_per_mask"] = [eng.best_in_mask(0, frame, m, 1) for m in masks]

    def labels_host():
        seen["labels_host"] = eng.best_per_label(0, frame, labels, n_labels=n_labels)

    def labels_device():
        seen["labels_device"] = eng.best_per_label(0, d_frame, d_labels, n_labels=n_labels)

    variants = {"best_per_mask": best_per_mask, "labels_host": labels_host, "labels_device": labels_device}
    if a.trace_only:
        variants = {a.trace_only: variants[a.trace_only]}
    for call in variants.values():
        call()
    if not a.trace_only:                                                         # the three routes find the same pixels
        want = [(None if h is None else (h[1], h[2], h[0]["best_vote"])) for h in seen["best_per_mask"]]
        for key in ("labels_host", "labels_device"):
            p = seen[key]["picks"]
            got = [((int(q["u"]), int(q["v"]), int(q["vote"])) if q["found"] else None) for q in p]
            assert got == want, (layout, n_labels, key)
    for _ in range(a.warmup):
        for call in variants.values():
            call()
    times = {key: [] for key in variants}
    for _ in range(a.calls):
        for key, call in variants.items():
            t0 = time.perf_counter_ns()
            call()
            times[key].append(time.perf_counter_ns() - t0)
    hip.hipFree(d_labels[0])
    if a.trace_only:
        continue
    host = {key: stats(t) for key, t in times.items()}
    base = host["best_per_mask"]
    for key in ("labels_host", "labels_device"):
        host[key]["median_minus_baseline_us"] = host[key]["median_us"] - base["median_us"]
    doc["labels"]["%s/%d" % (layout, n_labels)] = {"labelled_pixels": int((labels != 0).sum()), "found": int(seen["labels_host"]["picks"]["found"].sum()), "host_us": host,
                                    "labels_host_below_baseline_by_more_than_its_spread": bool(base["median_us"] - host["labels_host"]["median_us"] > base["spread_p10_p90_us"])}
eng.close()
hip.hipFree(d_frame.data)
if a.trace_only:
    sys.exit(0)
if a.kernel_stats:
    doc["kernel_trace_us"] = dict(kernel_stats(a.kernel_stats), note="rocprofv3 --kernel-trace --stats of a --trace-only labels_host run (the first call and the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
