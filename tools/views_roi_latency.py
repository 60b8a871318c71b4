#!/usr/bin/env python3
"""What "grasp THIS object" costs a two-camera cell end to end: scoring the fused scene in full and filtering afterwards, against
scoring the fused scene only under the cameras' masks (haf_score_views_roi).

Two 640 x 480 U16 depth views of one scene, a rectangular mask over one object in the first and, in the second, the valid pixels whose
base-frame (x, y) lies in the bounding box of the first view's masked points; two engines: C3 (56 x 56 grid, 20 rolls of 9 degrees,
surrogate model, table1 from cameras A and B of the test suite; the rectangle is rows 200..279, columns 280..359) and C5 (512 x 512,
36 rolls of 5 degrees, random 256-SV model, the synthetic cloud from 4 m above its centre and from a tilted second camera; the
rectangle is the central 160 x 120 pixels).  After a warm-up, the host wall clock of synchronised calls, the variants alternating within
one run so that drift hits them alike:
  full_then_best   haf_score_views followed by haf_grasp_map_best(mask) per masked view: the BASELINE, the route without the call
  roi_host         haf_score_views_roi, frames and masks in host memory
  roi_device       haf_score_views_roi, frames and masks resident in device memory
On a GPU box:
  python tools/views_roi_latency.py --calls 300 --out profiles/views_roi_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/c3 -o vroi -- python tools/views_roi_latency.py --trace-only roi_host --configs c3
                    # the kernels' own time, one run per config; then hand the runs' stats to the measuring run:
  python tools/views_roi_latency.py --kernel-stats c3=DIR/c3/.../vroi_kernel_stats.csv --kernel-stats c5=... --out profiles/views_roi_time.json
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
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default="")
ap.add_argument("--configs", default="c3,c5")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone (first call, warm-up, --calls calls) and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="CONFIG=CSV", help="the *_kernel_stats.csv of such a run with --configs CONFIG")
a = ap.parse_args()

import models  # noqa: E402
import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
FEAT, RNG = os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p25_us=q(0.25), p75_us=q(0.75), p90_us=q(0.90), min_us=float(us[0]),
                spread_p10_p90_us=q(0.90) - q(0.10))


def host_frame(depth, s2b):
    f = capi.Frame()
    f.data, f.kind, f.width, f.height, f.on_device, f.row_stride_bytes = depth.ctypes.data, capi.FRAME_DEPTH_U16, W, H, 0, W * 2
    f.fx, f.fy, f.cx, f.cy, f.depth_scale = K["fx"], K["fy"], K["cx"], K["cy"], 0.001
    f.sensor_to_base = (C.c_float * 12)(*s2b)
    return f


def bbox_mask(frame_a, mask_a, frame_b):
    """the valid pixels of view B whose base-frame (x, y) lies in the bounding box of the points of view A's masked pixels"""
    pa, pb = capi.frame_points(frame_a), capi.frame_points(frame_b)
    sel = (mask_a.reshape(-1) != 0) & np.isfinite(pa).all(axis=1)
    lo, hi = pa[sel, :2].min(axis=0), pa[sel, :2].max(axis=0)
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(pb).all(axis=1) & (pb[:, 0] >= lo[0]) & (pb[:, 0] <= hi[0]) & (pb[:, 1] >= lo[1]) & (pb[:, 1] <= hi[1])
    return inside.astype(np.uint8).reshape(H, W)


def setup(name):
    if name == "c3":
        cfg = dict(n_rolls=20, roll_step_deg=9)
        area, centre = 56, (0.13, 0.25, 0.0)
        xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
        poses = [tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9)), tilted_pose((-0.25, 0.20, -0.8), (0.04, 0.34, 0.85))]
        model = os.path.join(ROOT, "tests", "golden", "surrogate.model")
        rect = (200, 280, 280, 360)
        what = "C3: 56 x 56 grid, 20 rolls x 9 deg, surrogate model, table1 from cameras A and B, mask A rows 200..279 x columns 280..359, mask B by A's bounding box"
    else:
        cfg = dict(grid_h=512, grid_w=512, n_rolls=36, roll_step_deg=5)
        area, centre = 512, (0.0, 0.0, 0.0)
        xyz = models.synthetic_cloud(grid=512, k=2, seed=0)
        poses = [np.array([1, 0, 0, 0.0, 0, -1, 0, 0.0, 0, 0, -1, 4.0], np.float32), tilted_pose((0.2, -0.15, 0.5), (0.6, -0.5, 3.9))]
        import tempfile
        model = os.path.join(tempfile.mkdtemp(prefix="haf_vroi_"), "rand256.model")
        models.write_random_model(model, 256, seed=4, balanced=True)
        rect = (180, 300, 240, 400)
        what = "C5: 512 x 512 grid, 36 rolls x 5 deg, random 256-SV model, the synthetic cloud from 4 m above its centre and from a tilted second camera, mask A the central 160 x 120 pixels, mask B by A's bounding box"
    depths = [render_depth(xyz, p, W, H, K["fx"], K["fy"], K["cx"], K["cy"]) for p in poses]
    frames = [host_frame(d, p) for d, p in zip(depths, poses)]
    ma = np.zeros((H, W), np.uint8)
    ma[rect[0]:rect[1], rect[2]:rect[3]] = 1
    return cfg, area, centre, model, depths, frames, [ma, bbox_mask(frames[0], ma, frames[1])], what


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the ROI kernels and of the stages they shorten, from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_roi_mark_view<[^>]*>|k_roi_mark|k_mask_count_roi|k_vote_small<[^>]*>|k_vote_cells<[^>]*>|k_features\w*<[^>]*>|k_svm_screen\w*<[^>]*>|k_small_direct\w*|k_recheck\w*|k_view_points<[^>]*>)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


doc = {"tool": "tools/views_roi_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "views": "two 640 x 480 U16, f = 525", "library": os.path.relpath(capi.LIB_PATH, ROOT), "configs": {}}
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]


def to_device(arr):
    p = C.c_void_p()
    if hip.hipMalloc(C.byref(p), arr.nbytes) != 0 or hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy of a device-resident image failed")
    return p


for name in a.configs.split(","):
    cfg_kw, area, centre, model, depths, frames, masks, what = setup(name)
    L = capi.lib()
    cfg = capi.Config()
    L.haf_config_default(C.byref(cfg))
    cfg.feature_file, cfg.range_file, cfg.model_file = FEAT.encode(), RNG.encode(), model.encode()
    cfg.max_points = 1 << 20
    for k, v in cfg_kw.items():
        setattr(cfg, k, v)
    eng = C.c_void_p()
    if L.haf_create(C.byref(cfg), C.byref(eng)) != 0:
        sys.exit("haf_create: %s" % (L.haf_last_error(None) or b"").decode())
    inp = capi.GraspInput()
    L.haf_grasp_input_default(C.byref(inp))
    inp.grasp_area_center = (C.c_double * 3)(*centre)
    inp.grasp_area_length_x = inp.grasp_area_length_y = area
    out, cand = capi.GraspOutput(), capi.GraspCandidate()
    u, v, found = C.c_int32(), C.c_int32(), C.c_int32()
    n_views, cnt = C.c_int32(2), C.c_int64()
    best = {}
    host_frames = (capi.Frame * 2)(*frames)
    host_rois = (capi.Roi * 2)(*[capi.Roi(m.ctypes.data, W, 0) for m in masks])
    d_ptrs = [to_device(d) for d in depths] + [to_device(m) for m in masks]
    dev_frames = (capi.Frame * 2)(*frames)
    for k in range(2):
        dev_frames[k].data, dev_frames[k].on_device = d_ptrs[k].value, 1
    dev_rois = (capi.Roi * 2)(*[capi.Roi(d_ptrs[2 + k].value, W, 1) for k in range(2)])

    def full_then_best():
        rc = L.haf_score_views(eng, 1, C.byref(n_views), host_frames, C.byref(inp), C.byref(out), C.byref(cnt))
        top = 0
        for k in range(2):
            if rc == 0:
                rc = L.haf_grasp_map_best(eng, 0, C.byref(host_frames[k]), masks[k].ctypes.data, W, 1, C.byref(cand), C.byref(u), C.byref(v), C.byref(found))
                top = max(top, cand.grasp.best_vote if found.value else 0)
        best["full"] = (top, int(out.n_evals))
        return rc

    def roi_call(key, fr, rois):
        def call():
            rc = L.haf_score_views_roi(eng, 1, C.byref(n_views), fr, rois, C.byref(inp), C.byref(out), C.byref(cnt))
            best[key] = (max(0, out.best_vote), int(out.n_evals))
            return rc
        return call
    variants = {"full_then_best": full_then_best, "roi_host": roi_call("roi_host", host_frames, host_rois),
                "roi_device": roi_call("roi_device", dev_frames, dev_rois)}
    if a.trace_only:
        variants = {a.trace_only: variants[a.trace_only]}
    for key, call in variants.items():
        if call() != 0:
            sys.exit("%s: %s" % (key, (L.haf_last_error(eng) or b"").decode()))
    if not a.trace_only:                                                        # the three routes find the same best vote under the masks
        assert best["full"][0] == best["roi_host"][0] == best["roi_device"][0], (name, best)
    for _ in range(a.warmup):
        for call in variants.values():
            call()
    times = {key: [] for key in variants}
    for _ in range(a.calls):
        for key, call in variants.items():
            t0 = time.perf_counter_ns()
            call()
            times[key].append(time.perf_counter_ns() - t0)
    L.haf_destroy(eng)
    for p in d_ptrs:
        hip.hipFree(p)
    if a.trace_only:
        continue
    host = {key: stats(t) for key, t in times.items()}
    base = host["full_then_best"]
    for key in ("roi_host", "roi_device"):
        host[key]["median_minus_baseline_us"] = host[key]["median_us"] - base["median_us"]
    doc["configs"][name] = {"request": what, "masked_pixels": [int((m != 0).sum()) for m in masks], "valid_points": int(cnt.value),
                            "best_vote_under_the_masks": best["full"][0], "n_evals_full": best["full"][1], "n_evals_roi": best["roi_host"][1], "host_us": host,
                            "roi_host_below_baseline_by_more_than_its_spread": bool(base["median_us"] - host["roi_host"]["median_us"] > base["spread_p10_p90_us"])}
if a.trace_only:
    sys.exit(0)
if a.kernel_stats:
    doc["kernel_trace_us"] = {"note": "rocprofv3 --kernel-trace --stats of --trace-only roi_host runs (one config per run; the first call and the warm-up included)"}
    for spec in a.kernel_stats:
        name, _, path = spec.partition("=")
        doc["kernel_trace_us"][name] = kernel_stats(path)
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
