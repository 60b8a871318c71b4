#!/usr/bin/env python3
"""What a request seen by TWO cameras costs end to end, by the route its views take into the engine (haf_score_views).

C3 configuration (56 x 56 grid, 20 rolls of 9 degrees, 56 x 56 search area at (0.13, 0.25, 0)), surrogate model, two 640 x 480 U16 depth
frames rendered from the table1 cloud: one camera 0.9 m above (0.13, 0.2) looking straight down, one tilted beside it.  After a
warm-up, the host wall clock of synchronised calls, the variants alternating within one run so that drift hits them alike:
  host_fused          haf_frame_points per view on the host, concatenated, haf_score on all 614 400 points: the BASELINE, the only
                      route a build without haf_score_views has (the deprojection is part of the call: it is what the caller pays)
  host_fused_valid    the same with the valid points compacted by the caller before haf_score
  views_host          haf_score_views, both frames in host memory
  views_device        haf_score_views, both frames resident in device memory
  one_view            haf_score_views with the first frame alone        } the same request by the two entry points
  one_frame           haf_score_frames of the first frame               }
On a GPU box:
  python tools/view_latency.py --calls 300 --out profiles/view_input_time.json
  python tools/view_latency.py --baseline-lib OTHER/libhafgrasp.so --out parent.json    # the baseline alone on another build of the ABI
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/V -o V -- python tools/view_latency.py --trace-only V    # the kernels' own
                      time, one run per variant V (views_host, one_view, one_frame); then hand the runs' stats to the measuring run:
  python tools/view_latency.py --kernel-stats views_host=DIR/views_host/.../views_host_kernel_stats.csv --kernel-stats one_view=... --out ...
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
ap.add_argument("--merge", default="", help="a JSON written with --baseline-lib, stored under 'baseline_on_other_build'")
ap.add_argument("--baseline-lib", default="", help="measure host_fused alone on this build of libhafgrasp.so (e.g. the parent commit's)")
ap.add_argument("--trace-only", default="", metavar="VARIANT", help="run this variant alone (first call, warm-up, --calls calls) and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="VARIANT=CSV",
                help="the *_kernel_stats.csv of such a run: the deprojection and binning kernels' times go into the JSON under 'kernel_trace_us'")
a = ap.parse_args()
if a.baseline_lib:
    os.environ["HAF_LIB"] = os.path.abspath(a.baseline_lib)

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
FEAT, RNG, MODEL = os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model")
W, H, FX, FY, CX, CY = 640, 480, 525.0, 525.0, 319.5, 239.5
DOWN = np.array([1, 0, 0, 0.13, 0, -1, 0, 0.2, 0, 0, -1, 0.9], np.float32)


def bind_min(path):
    """the entry points the baseline needs, for a build of the ABI that predates views (capi binds every name of this tree's header)"""
    L = C.CDLL(path)
    E = C.c_void_p
    L.haf_config_default.argtypes = [C.POINTER(capi.Config)]
    L.haf_grasp_input_default.argtypes = [C.POINTER(capi.GraspInput)]
    L.haf_create.argtypes = [C.POINTER(capi.Config), C.POINTER(E)]
    L.haf_destroy.argtypes = [E]
    L.haf_last_error.restype = C.c_char_p
    L.haf_last_error.argtypes = [E]
    L.haf_score.argtypes = [E, C.POINTER(capi.Cloud), C.POINTER(capi.GraspInput), C.POINTER(capi.GraspOutput)]
    L.haf_frame_points.argtypes = [C.POINTER(capi.Frame), C.c_void_p]
    return L


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p25_us=q(0.25), p75_us=q(0.75), p90_us=q(0.90), min_us=float(us[0]),
                spread_p10_p90_us=q(0.90) - q(0.10))


def host_frame(depth, s2b):
    """(capi.depth_frame binds this tree's library; the struct is the same for a --baseline-lib build)"""
    f = capi.Frame()
    f.data, f.kind, f.width, f.height, f.on_device, f.row_stride_bytes = depth.ctypes.data, capi.FRAME_DEPTH_U16, W, H, 0, W * 2
    f.fx, f.fy, f.cx, f.cy, f.depth_scale = FX, FY, CX, CY, 0.001
    f.sensor_to_base = (C.c_float * 12)(*s2b)
    return f


xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
poses = [DOWN, tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9))]
depths = [render_depth(xyz, p, W, H, FX, FY, CX, CY) for p in poses]
frames = [host_frame(d, p) for d, p in zip(depths, poses)]

L = bind_min(capi.LIB_PATH) if a.baseline_lib else capi.lib()
cfg = capi.Config()
L.haf_config_default(C.byref(cfg))
cfg.feature_file, cfg.range_file, cfg.model_file = FEAT.encode(), RNG.encode(), MODEL.encode()
cfg.n_rolls, cfg.roll_step_deg, cfg.max_points = 20, 9, 1 << 20
eng = C.c_void_p()
if L.haf_create(C.byref(cfg), C.byref(eng)) != 0:
    sys.exit("haf_create: %s" % (L.haf_last_error(None) or b"").decode())
inp = capi.GraspInput()
L.haf_grasp_input_default(C.byref(inp))
inp.grasp_area_center = (C.c_double * 3)(0.13, 0.25, 0.0)
inp.grasp_area_length_x = inp.grasp_area_length_y = 56
out = capi.GraspOutput()
fused = np.empty((2 * W * H, 3), np.float32)            # the caller's buffer for the host route, reused by every call
n_valid = [0]


def host_fused(compact):
    def call():
        for k, f in enumerate(frames):
            rc = L.haf_frame_points(C.byref(f), fused[k * W * H:].ctypes.data)
            if rc != 0:
                return rc
        pts = fused
        if compact:
            pts = fused[np.isfinite(fused).all(axis=1)]
            n_valid[0] = len(pts)
        cl = capi.Cloud(pts.ctypes.data_as(C.c_void_p), pts.shape[0], 3, 0)
        return L.haf_score(eng, C.byref(cl), C.byref(inp), C.byref(out))
    return call


variants = {"host_fused": host_fused(False)}
keep = []
if not a.baseline_lib:
    variants["host_fused_valid"] = host_fused(True)
    counts = (C.c_int64 * 1)()

    def views_variant(name, fr):
        arr, per = (capi.Frame * len(fr))(*fr), (C.c_int32 * 1)(len(fr))
        variants[name] = lambda: L.haf_score_views(eng, 1, per, arr, C.byref(inp), C.byref(out), counts)

    views_variant("views_host", frames)
    # the device-resident frames: plain hipMalloc'ed copies through the HIP runtime the library itself is linked against
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    dev = []
    for d, f in zip(depths, frames):
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), d.nbytes) != 0 or hip.hipMemcpy(p, d.ctypes.data, d.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
            sys.exit("hipMalloc / hipMemcpy of a device-resident frame failed")
        keep.append(p)
        g = capi.Frame.from_buffer_copy(f)
        g.data, g.on_device = p.value, 1
        dev.append(g)
    views_variant("views_device", dev)
    views_variant("one_view", frames[:1])
    one = frames[0]
    variants["one_frame"] = lambda: L.haf_score_frames(eng, 1, C.byref(one), C.byref(inp), C.byref(out))

if a.trace_only:
    variants = {a.trace_only: variants[a.trace_only]}
FIELDS = ("eval", "best_row", "best_col", "best_roll", "best_vote", "n_evals", "grasp_point1", "grasp_point2")
first = {}
for name, call in variants.items():
    rc = call()
    if rc != 0:
        sys.exit("%s: %s" % (name, (L.haf_last_error(eng) or b"").decode()))
    first[name] = capi.output_to_dict(out)
ref = first.get("host_fused", first[next(iter(first))])
for name, o in ({} if a.trace_only else first).items():                             # every two-view variant computes the same request; so do the two one-view ones
    want = first["one_frame"] if name.startswith("one_") else ref
    assert all(o[k] == want[k] for k in FIELDS), (name, o, want)
for _ in range(a.warmup):
    for call in variants.values():
        call()
times = {name: [] for name in variants}
for _ in range(a.calls):
    for name, call in variants.items():
        t0 = time.perf_counter_ns()
        call()
        times[name].append(time.perf_counter_ns() - t0)
L.haf_destroy(eng)
if a.trace_only:
    sys.exit(0)


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the kernels that turn views into height grids, from a rocprofv3 *_kernel_stats.csv"""
    import csv
    import re
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"\b(k_view_points<[^>]*>|k_frame_points<[^>]*>|k_bin\w*|k_bkt_\w+|k_small_pre<[^>]*>)", r["Name"])
            if m:
                rows[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3,
                                        stddev_us=float(r["StdDev"]) / 1e3)
    return rows


doc = {"tool": "tools/view_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": {"config": "C3: 56 x 56 grid, 20 rolls x 9 deg, 56 x 56 cm at (0.13, 0.25, 0), surrogate model",
                   "views": "two 640 x 480 U16 frames rendered from table1: 0.9 m above (0.13, 0.2) looking down; 0.9 m above (0.20, 0.13) tilted by (0.21, -0.17, 0.6) rad",
                   "pixels": 2 * W * H, "valid_points": int(n_valid[0]) if not a.baseline_lib else None, "n_evals": ref["n_evals"], "eval": ref["eval"],
                   "best": [ref["best_row"], ref["best_col"], ref["best_roll"]]},
       "library": os.path.relpath(capi.LIB_PATH, ROOT) if not a.baseline_lib else "another build of the ABI (--baseline-lib)",
       "host_us": {name: stats(t) for name, t in times.items()}}
if not a.baseline_lib:
    base = doc["host_us"]["host_fused"]
    for name in ("host_fused_valid", "views_host", "views_device"):
        doc["host_us"][name]["median_minus_baseline_us"] = doc["host_us"][name]["median_us"] - base["median_us"]
    doc["views_host_below_baseline"] = bool(doc["host_us"]["views_host"]["median_us"] < base["median_us"])
    one = doc["host_us"]["one_view"]["median_us"] - doc["host_us"]["one_frame"]["median_us"]
    doc["host_us"]["one_view"]["median_minus_one_frame_us"] = one
    doc["one_view_slower_than_one_frame_by_more_than_the_baseline_spread"] = bool(one > base["spread_p10_p90_us"])
if a.kernel_stats:
    doc["kernel_trace_us"] = {"note": "rocprofv3 --kernel-trace --stats of --trace-only VARIANT runs (one variant per run; the first call and the warm-up included)"}
    for spec in a.kernel_stats:
        name, _, path = spec.partition("=")
        doc["kernel_trace_us"][name] = kernel_stats(path)
if a.merge:
    with open(a.merge) as f:
        doc["baseline_on_other_build"] = json.load(f)["host_us"]["host_fused"]
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
