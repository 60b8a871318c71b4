#!/usr/bin/env python3
"""What a request costs end to end when the engine takes the sensor's frame instead of a base-frame cloud (haf_score_frames).

C3 configuration (56 x 56 grid, 20 rolls of 9 degrees, 56 x 56 search area at (0.13, 0.25, 0)), surrogate model, the 640 x 480 depth
frame rendered from the table1 cloud by a camera 0.9 m above (0.13, 0.2) looking straight down.  After a warm-up, the host wall
clock of synchronised calls, the variants alternating within one run so that drift hits them alike:
  cloud_organised   haf_score on the organised 307 200-point host xyz cloud of that frame (haf_frame_points): the BASELINE
  cloud_valid       haf_score on the valid points only (what a caller gets who also compacts on the host; for information)
  frame_u16         haf_score_frames, host U16 frame
  frame_f32         haf_score_frames, host F32 frame (the same depths in metres)
  frame_u16_device  haf_score_frames, U16 frame resident in device memory
On a GPU box:
  python tools/frame_latency.py --calls 200 --out profiles/frame_input_time.json
  python tools/frame_latency.py --baseline-lib OTHER/libhafgrasp.so --out parent.json    # the baseline alone on another build of the ABI
  rocprofv3 --kernel-trace --stats -d DIR -o frame -- python tools/frame_latency.py --trace-only   # the kernel's own time
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
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default="")
ap.add_argument("--merge", default="", help="a JSON written with --baseline-lib, stored under 'baseline_on_other_build'")
ap.add_argument("--baseline-lib", default="", help="measure cloud_organised alone on this build of libhafgrasp.so (e.g. the parent commit's)")
ap.add_argument("--trace-only", action="store_true", help="warm up, then 20 calls of every frame variant: for rocprofv3 --kernel-trace")
a = ap.parse_args()
if a.baseline_lib:
    os.environ["HAF_LIB"] = os.path.abspath(a.baseline_lib)

import pcdio  # noqa: E402
from render import render_depth  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
FEAT, RNG, MODEL = os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model")
W, H, FX, FY, CX, CY = 640, 480, 525.0, 525.0, 319.5, 239.5
S2B = np.array([1, 0, 0, 0.13, 0, -1, 0, 0.2, 0, 0, -1, 0.9], np.float32)


def host_points(depth):
    """haf_frame_points' arithmetic for this frame in numpy fp32 (the --baseline-lib build may not have the function)"""
    f = np.float32
    z = depth.astype(f) * f(0.001)
    u, v = np.arange(W, dtype=f)[None, :], np.arange(H, dtype=f)[:, None]
    xc = ((u - f(CX)) * (f(1) / f(FX))) * z
    yc = ((v - f(CY)) * (f(1) / f(FY))) * z
    t = S2B.reshape(3, 4)
    p = np.stack([((t[r, 0] * xc + t[r, 1] * yc) + t[r, 2] * z) + t[r, 3] for r in range(3)], axis=-1)
    p[depth == 0] = np.nan
    return np.ascontiguousarray(p.reshape(-1, 3), dtype=f)


def bind_min(path):
    """the entry points the baseline needs, for a build of the ABI that predates frames (capi binds every name of this tree's header)"""
    L = C.CDLL(path)
    E = C.c_void_p
    L.haf_config_default.argtypes = [C.POINTER(capi.Config)]
    L.haf_grasp_input_default.argtypes = [C.POINTER(capi.GraspInput)]
    L.haf_create.argtypes = [C.POINTER(capi.Config), C.POINTER(E)]
    L.haf_destroy.argtypes = [E]
    L.haf_last_error.restype = C.c_char_p
    L.haf_last_error.argtypes = [E]
    L.haf_score.argtypes = [E, C.POINTER(capi.Cloud), C.POINTER(capi.GraspInput), C.POINTER(capi.GraspOutput)]
    return L


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p25_us=q(0.25), p75_us=q(0.75), p90_us=q(0.90), min_us=float(us[0]),
                spread_p10_p90_us=q(0.90) - q(0.10))


xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
depth = render_depth(xyz, S2B, W, H, FX, FY, CX, CY)
organised = host_points(depth)
valid = np.ascontiguousarray(organised[np.isfinite(organised).all(axis=1)])
metres = depth.astype(np.float32) * np.float32(0.001)

L = bind_min(capi.LIB_PATH) if a.baseline_lib else capi.lib()
cfg = capi.Config()
L.haf_config_default(C.byref(cfg))
cfg.feature_file, cfg.range_file, cfg.model_file = FEAT.encode(), RNG.encode(), MODEL.encode()
cfg.n_rolls, cfg.roll_step_deg, cfg.max_points = 20, 9, 1 << 19
eng = C.c_void_p()
if L.haf_create(C.byref(cfg), C.byref(eng)) != 0:
    sys.exit("haf_create: %s" % (L.haf_last_error(None) or b"").decode())
inp = capi.GraspInput()
L.haf_grasp_input_default(C.byref(inp))
inp.grasp_area_center = (C.c_double * 3)(0.13, 0.25, 0.0)
inp.grasp_area_length_x = inp.grasp_area_length_y = 56
out = capi.GraspOutput()

variants = {}


def cloud_variant(name, pts):
    cl = capi.Cloud(pts.ctypes.data_as(C.c_void_p), pts.shape[0], 3, 0)
    variants[name] = lambda: L.haf_score(eng, C.byref(cl), C.byref(inp), C.byref(out))


def frame_variant(name, frame):
    variants[name] = lambda: L.haf_score_frames(eng, 1, C.byref(frame), C.byref(inp), C.byref(out))


cloud_variant("cloud_organised", organised)
keep = []
if not a.baseline_lib:
    assert (capi.frame_points(capi.depth_frame(depth, FX, FY, CX, CY, sensor_to_base=S2B)).view(np.uint32) == organised.view(np.uint32)).all()
    cloud_variant("cloud_valid", valid)
    frame_variant("frame_u16", capi.depth_frame(depth, FX, FY, CX, CY, sensor_to_base=S2B))
    frame_variant("frame_f32", capi.depth_frame(metres, FX, FY, CX, CY, sensor_to_base=S2B))
    # the device-resident frame: a plain hipMalloc'ed copy through the HIP runtime the library itself is linked against
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d_depth = C.c_void_p()
    if hip.hipMalloc(C.byref(d_depth), depth.nbytes) != 0 or hip.hipMemcpy(d_depth, depth.ctypes.data, depth.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0:
        sys.exit("hipMalloc / hipMemcpy of the device-resident frame failed")
    keep.append(d_depth)
    frame_variant("frame_u16_device", capi.depth_frame(d_depth.value, FX, FY, CX, CY, sensor_to_base=S2B, width=W, height=H, dtype=np.uint16))

results, first = {}, {}
for name, call in variants.items():                       # every variant computes the same request
    rc = call()
    if rc != 0:
        sys.exit("%s: %s" % (name, (L.haf_last_error(eng) or b"").decode()))
    first[name] = capi.output_to_dict(out)
ref = first["cloud_organised"]
for name, o in first.items():
    same = all(o[k] == ref[k] for k in ("eval", "best_row", "best_col", "best_roll", "best_vote", "n_evals", "grasp_point1", "grasp_point2"))
    assert same, (name, o, ref)
for _ in range(a.warmup):
    for call in variants.values():
        call()
if a.trace_only:
    for _ in range(20):
        for name, call in variants.items():
            if name.startswith("frame"):
                call()
    L.haf_destroy(eng)
    sys.exit(0)
times = {name: [] for name in variants}
for _ in range(a.calls):
    for name, call in variants.items():
        t0 = time.perf_counter_ns()
        call()
        times[name].append(time.perf_counter_ns() - t0)
L.haf_destroy(eng)
doc = {"tool": "tools/frame_latency.py: host wall clock of synchronised calls, variants alternating within one run (%d calls each after %d warm-up rounds)" % (a.calls, a.warmup),
       "request": {"config": "C3: 56 x 56 grid, 20 rolls x 9 deg, 56 x 56 cm at (0.13, 0.25, 0), surrogate model", "frame": "640 x 480 U16 rendered from table1, camera 0.9 m above (0.13, 0.2) looking down",
                   "pixels": W * H, "valid_pixels": int(valid.shape[0]), "n_evals": ref["n_evals"], "eval": ref["eval"], "best": [ref["best_row"], ref["best_col"], ref["best_roll"]]},
       "bytes_per_request": {"cloud_organised": int(organised.nbytes), "cloud_valid": int(valid.nbytes), "frame_u16": int(depth.nbytes), "frame_f32": int(metres.nbytes)},
       "library": os.path.relpath(capi.LIB_PATH, ROOT) if not a.baseline_lib else "another build of the ABI (--baseline-lib)",
       "host_us": {name: stats(t) for name, t in times.items()}}
if not a.baseline_lib:
    base = doc["host_us"]["cloud_organised"]
    for name in ("frame_u16", "frame_f32", "frame_u16_device", "cloud_valid"):
        doc["host_us"][name]["median_minus_baseline_us"] = doc["host_us"][name]["median_us"] - base["median_us"]
    doc["frame_u16_below_baseline_by_more_than_its_spread"] = bool(base["median_us"] - doc["host_us"]["frame_u16"]["median_us"] > base["spread_p10_p90_us"])
if a.merge:
    with open(a.merge) as f:
        doc["baseline_on_other_build"] = json.load(f)["host_us"]["cloud_organised"]
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
