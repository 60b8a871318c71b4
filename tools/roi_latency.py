#!/usr/bin/env python3
"""What "grasp THIS object" costs end to end: scoring the whole search area and filtering afterwards, against scoring only under the mask
(haf_score_frames_roi).

One 640 x 480 U16 depth frame and a rectangular mask over one object, two engines: C3 (56 x 56 grid, 20 rolls of 9 degrees, surrogate
model, table1 rendered from camera A -- 0.9 m above (0.20, 0.13), tilted by (0.21, -0.17, 0.6) rad; the mask is rows 200..279, columns
280..359) and C5 (512 x 512, 36 rolls of 5 degrees, random 256-SV model, the synthetic cloud from 4 m above its centre; the mask is
the central 160 x 120 pixels).  After a warm-up, the host wall clock of synchronised calls, the variants alternating within one run so
that drift hits them alike:
  full_then_best   haf_score_frames followed by haf_grasp_map_best(mask): the BASELINE, what a caller does without the ROI call
  roi_host         haf_score_frames_roi, the mask in host memory
  roi_device       haf_score_frames_roi, the mask resident in device memory
On a GPU box:
  python tools/roi_latency.py --calls 300 --out profiles/roi_time.json
  python tools/roi_latency.py --baseline-lib OTHER/libhafgrasp.so --out parent.json      # the baseline alone on another build of the ABI
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/c3 -o roi -- python tools/roi_latency.py --trace-only roi_host --configs c3
                    # the kernels' own time, one run per config; then hand the runs' stats to the measuring run:
  python tools/roi_latency.py --kernel-stats c3=DIR/c3/.../roi_kernel_stats.csv --kernel-stats c5=... --merge parent.json --out profiles/roi_time.json
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
ap.add_argument("--merge", default="", help="a JSON written with --baseline-lib, stored under 'baseline_on_other_build'")
ap.add_argument("--baseline-lib", default="", help="measure full_then_best alone on this build of libhafgrasp.so (e.g. the parent commit's)")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone (first call, warm-up, --calls calls) and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="CONFIG=CSV", help="the *_kernel_stats.csv of such a run with --configs CONFIG")
a = ap.parse_args()
if a.baseline_lib:
    os.environ["HAF_LIB"] = os.path.abspath(a.baseline_lib)

import models  # noqa: E402
import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
FEAT, RNG = os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def bind_min(path):
    """the entry points the baseline needs, for a build of the ABI that predates the ROI call (capi binds every name of this tree's header)"""
    L = C.CDLL(path)
    E = C.c_void_p
    L.haf_config_default.argtypes = [C.POINTER(capi.Config)]
    L.haf_grasp_input_default.argtypes = [C.POINTER(capi.GraspInput)]
    L.haf_create.argtypes = [C.POINTER(capi.Config), C.POINTER(E)]
    L.haf_destroy.argtypes = [E]
    L.haf_last_error.restype = C.c_char_p
    L.haf_last_error.argtypes = [E]
    L.haf_score_frames.argtypes = [E, C.c_int32, C.POINTER(capi.Frame), C.POINTER(capi.GraspInput), C.POINTER(capi.GraspOutput)]
    L.haf_grasp_map_best.argtypes = [E, C.c_int32, C.POINTER(capi.Frame), C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(capi.GraspCandidate),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p25_us=q(0.25), p75_us=q(0.75), p90_us=q(0.90), min_us=float(us[0]),
                spread_p10_p90_us=q(0.90) - q(0.10))


def setup(name):
    if name == "c3":
        cfg = dict(n_rolls=20, roll_step_deg=9)
        area, centre = 56, (0.13, 0.25, 0.0)
        xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
        pose = tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9))
        model = os.path.join(ROOT, "tests", "golden", "surrogate.model")
        rect = (200, 280, 280, 360)
        what = "C3: 56 x 56 grid, 20 rolls x 9 deg, surrogate model, table1 from camera A, mask rows 200..279 x columns 280..359"
    else:
        cfg = dict(grid_h=512, grid_w=512, n_rolls=36, roll_step_deg=5)
        area, centre = 512, (0.0, 0.0, 0.0)
        xyz = models.synthetic_cloud(grid=512, k=2, seed=0)
        pose = np.array([1, 0, 0, 0.0, 0, -1, 0, 0.0, 0, 0, -1, 4.0], np.float32)
        import tempfile
        model = os.path.join(tempfile.mkdtemp(prefix="haf_roi_"), "rand256.model")
        models.write_random_model(model, 256, seed=4, balanced=True)
        rect = (180, 300, 240, 400)
        what = "C5: 512 x 512 grid, 36 rolls x 5 deg, random 256-SV model, the synthetic cloud from 4 m above its centre, mask the central 160 x 120 pixels"
    depth = render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
    mask = np.zeros((H, W), np.uint8)
    mask[rect[0]:rect[1], rect[2]:rect[3]] = 1
    return cfg, area, centre, model, depth, pose, mask, what


def host_frame(depth, s2b):
    """(capi.depth_frame binds this tree's library; the struct is the same for a --baseline-lib build)"""
    f = capi.Frame()
    f.data, f.kind, f.width, f.height, f.on_device, f.row_stride_bytes = depth.ctypes.data, capi.FRAME_DEPTH_U16, W, H, 0, W * 2
    f.fx, f.fy, f.cx, f.cy, f.depth_scale = K["fx"], K["fy"], K["cx"], K["cy"], 0.001
    f.sensor_to_base = (C.c_float * 12)(*s2b)
    return f


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the ROI kernels and of the stages they shorten, from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_roi_mark|k_mask_count_roi|k_vote_small<[^>]*>|k_vote_cells<[^>]*>|k_features\w*<[^>]*>|k_svm_screen\w*<[^>]*>|k_small_direct\w*|k_recheck\w*|k_frame_points<[^>]*>)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    return rows


doc = {"tool": "tools/roi_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "frame": "640 x 480 U16, f = 525", "library": os.path.relpath(capi.LIB_PATH, ROOT) if not a.baseline_lib else "another build of the ABI (--baseline-lib)",
       "configs": {}}
for name in a.configs.split(","):
    cfg_kw, area, centre, model, depth, pose, mask, what = setup(name)
    frame = host_frame(depth, pose)
    L = bind_min(capi.LIB_PATH) if a.baseline_lib else capi.lib()
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
    best = {}

    def full_then_best():
        rc = L.haf_score_frames(eng, 1, C.byref(frame), C.byref(inp), C.byref(out))
        if rc == 0:
            rc = L.haf_grasp_map_best(eng, 0, C.byref(frame), mask.ctypes.data, W, 1, C.byref(cand), C.byref(u), C.byref(v), C.byref(found))
            best["full"] = (cand.grasp.best_vote if found.value else 0, int(out.n_evals))
        return rc

    variants = {"full_then_best": full_then_best}
    if not a.baseline_lib:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        d_mask = C.c_void_p()
        if hip.hipMalloc(C.byref(d_mask), mask.nbytes) != 0 or hip.hipMemcpy(d_mask, mask.ctypes.data, mask.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
            sys.exit("hipMalloc / hipMemcpy of the device-resident mask failed")
        roi_h, roi_d = capi.Roi(mask.ctypes.data, W, 0), capi.Roi(d_mask.value, W, 1)

        def roi_call(key, roi):
            def call():
                rc = L.haf_score_frames_roi(eng, 1, C.byref(frame), C.byref(roi), C.byref(inp), C.byref(out))
                best[key] = (max(0, out.best_vote), int(out.n_evals))
                return rc
            return call
        variants["roi_host"], variants["roi_device"] = roi_call("roi_host", roi_h), roi_call("roi_device", roi_d)
    if a.trace_only:
        variants = {a.trace_only: variants[a.trace_only]}
    for key, call in variants.items():
        if call() != 0:
            sys.exit("%s: %s" % (key, (L.haf_last_error(eng) or b"").decode()))
    if not a.trace_only and not a.baseline_lib:                                 # the three routes find the same best vote under the mask
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
    if a.trace_only:
        continue
    host = {key: stats(t) for key, t in times.items()}
    c = {"request": what, "masked_pixels": int((mask != 0).sum()), "best_vote_under_the_mask": best["full"][0], "n_evals_full": best["full"][1], "host_us": host}
    if not a.baseline_lib:
        base = host["full_then_best"]
        c["n_evals_roi"] = best["roi_host"][1]
        for key in ("roi_host", "roi_device"):
            host[key]["median_minus_baseline_us"] = host[key]["median_us"] - base["median_us"]
        c["roi_host_below_baseline_by_more_than_its_spread"] = bool(base["median_us"] - host["roi_host"]["median_us"] > base["spread_p10_p90_us"])
    doc["configs"][name] = c
if a.trace_only:
    sys.exit(0)
if a.kernel_stats:
    doc["kernel_trace_us"] = {"note": "rocprofv3 --kernel-trace --stats of --trace-only roi_host runs (one config per run; the first call and the warm-up included)"}
    for spec in a.kernel_stats:
        name, _, path = spec.partition("=")
        doc["kernel_trace_us"][name] = kernel_stats(path)
if a.merge:
    with open(a.merge) as f:
        other = json.load(f)
    doc["baseline_on_other_build"] = {k: v["host_us"]["full_then_best"] for k, v in other["configs"].items()}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
