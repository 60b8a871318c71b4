#!/usr/bin/env python3
"""What asking "has a camera seen this space empty" costs: haf_check_space on the device against haf_check_space_ref, the same
definition on one host thread; haf_check_grasps on the same frame stands beside them for context only (it answers another question).

The set-up is tools/openings_latency.py's: table1 rendered as a 640 x 480 U16 frame from camera A, and once more from a second pose for
the two-view variants; the C3 request on the first (56 x 56 grid, 20 rolls); the candidates of haf_top_grasps with k = 32 and -- its
suppression leaves this scene only a few dozen -- with k = 1024, min_vote 1 and the suppression off, handed over as
haf_grasp_candidate arrays built once; the library's default (nominal) gripper and space parameters: 4800 samples per grasp.  After a
warm-up, the host wall clock of synchronised calls through the Python binding, the variants alternating within one run so that drift
hits them alike -- per candidate set:
  space_device_1view / _2views   haf_check_space, device-resident views
  space_host_1view / _2views     haf_check_space, host views (staged and uploaded again by the call: that cost is shown, not hidden)
  check_grasps_device            CONTEXT: haf_check_grasps on the device-resident first frame
  host_ref_1view / _2views       BASELINE: haf_check_space_ref on one host thread (--ref-calls calls up front, NOT alternating with the
                                 device variants: a call takes 1 to 110 ms, 40 to 500 times theirs)
On a GPU box:
  python tools/space_latency.py --calls 200 --out profiles/grasp_space_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o space -- python tools/space_latency.py --trace-only --set k32
                    # the kernel's own time, one trace per candidate set; then hand the stats to the measuring run:
  python tools/space_latency.py --kernel-stats k32=DIR/.../space_kernel_stats.csv --out profiles/grasp_space_time.json
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
ap.add_argument("--ref-calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default="")
ap.add_argument("--trace-only", action="store_true", help="run haf_check_space on the device-resident views alone and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--set", default="", metavar="k32|k1024_unsuppressed", help="this candidate set alone (with --trace-only: one trace per set)")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="SET=CSV", help="the *_kernel_stats.csv of such a run of that set; may be given once per set")
a = ap.parse_args()

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)
POSE_FIELDS = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector")
KERNELS = r"\b(k_space_samples)"


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} from a rocprofv3 *_kernel_stats.csv"""
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


def candidate_array(cands):
    arr = (capi.GraspCandidate * len(cands))()
    for c, d in zip(arr, cands):
        for f in POSE_FIELDS:
            setattr(c.grasp, f, (C.c_double * 3)(*d[f]))
    return arr


xyz = pcdio.load_pcd(os.path.join(D, "table1_mult_obj_rcs_1428580506606673.pcd"))
poses = [tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9)), tilted_pose((-0.19, 0.15, 0.6), (0.02, 0.42, 0.9))]
depths = [render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"]) for pose in poses]
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 20)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
inp = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
frames = [capi.depth_frame(depth, sensor_to_base=pose, **K) for depth, pose in zip(depths, poses)]
d_frames = [capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K) for depth, pose in zip(depths, poses)]
gripper, P = capi.gripper(), capi.space_params()
eng.score_frames([frames[0]], [inp])
sets = {"k32": candidate_array(eng.top_grasps(k=32)[0]),
        "k1024_unsuppressed": candidate_array(eng.top_grasps(k=1024, min_vote=1, cell_radius=0, roll_window=0, min_dist_m=0.0)[0])}
if a.set:
    sets = {a.set: sets[a.set]}

if a.trace_only:
    for _ in range(a.warmup + a.calls):
        for cands in sets.values():
            eng.check_space(d_frames[:1], cands, gripper, P)
            eng.check_space(d_frames, cands, gripper, P)
    eng.close()
    sys.exit(0)

routes = {"space_device_1view": lambda c: eng.check_space(d_frames[:1], c, gripper, P), "space_device_2views": lambda c: eng.check_space(d_frames, c, gripper, P),
          "space_host_1view": lambda c: eng.check_space(frames[:1], c, gripper, P), "space_host_2views": lambda c: eng.check_space(frames, c, gripper, P),
          "check_grasps_device": lambda c: eng.check_grasps(d_frames[0], c, gripper)}
variants = {(route, name): (lambda call=call, cands=cands: call(cands)) for name, cands in sets.items() for route, call in routes.items()}
doc_sets = {}
for name, cands in sets.items():
    block, wants = {}, {}
    for tag, views in (("1view", frames[:1]), ("2views", frames)):
        ns = []
        for _ in range(a.ref_calls):
            t0 = time.perf_counter_ns()
            wants[tag] = capi.check_space_ref(views, cands, gripper, P)
            ns.append(time.perf_counter_ns() - t0)
        block["host_ref_" + tag] = stats(ns)
        for where in ("device", "host"):
            got = variants["space_%s_%s" % (where, tag), name]()
            assert got[0].tobytes() == wants[tag][0].tobytes() and got[1].tolist() == wants[tag][1].tolist() and got[2] == wants[tag][2], (where, tag, name)
    doc_sets[name] = dict(n_grasps=len(cands), info=wants["1view"][2], n_clear_1view=int(wants["1view"][1].size), n_clear_2views=int(wants["2views"][1].size),
                          states_1view=wants["1view"][0]["n"].sum(axis=0).tolist(), states_2views=wants["2views"][0]["n"].sum(axis=0).tolist(), host_us=block)
for _ in range(a.warmup):
    for call in variants.values():
        call()
times = {key: [] for key in variants}
for _ in range(a.calls):
    for key, call in variants.items():
        t0 = time.perf_counter_ns()
        call()
        times[key].append(time.perf_counter_ns() - t0)
for name in sets:
    block = doc_sets[name]["host_us"]
    block.update({route: stats(times[route, name]) for route in routes})
    for route in routes:
        if route.startswith("space_"):
            base = "host_ref_" + route.rsplit("_", 1)[1]
            block[route]["below_%s_by_more_than_its_spread" % base] = bool(block[base]["median_us"] - block[route]["median_us"] > block[base]["spread_p10_p90_us"])
doc = {"tool": "tools/space_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds; host_ref_*: %d calls, not alternating)" % (a.calls, a.warmup, a.ref_calls),
       "request": "table1 from camera A, and from a second pose for the two-view variants, as 640 x 480 U16 frames; candidates of haf_top_grasps(k = 32, and k = 1024 with min_vote 1 and no suppression) of the C3 request (56 x 56 grid, 20 rolls) on the first as haf_grasp_candidate arrays built once; the default nominal gripper and space parameters (4800 samples per grasp)",
       "baselines": "host_ref_1view / host_ref_2views: haf_check_space_ref on one host thread; check_grasps_device: haf_check_grasps on the device-resident first frame, for context only -- it counts points, it does not ask what was seen",
       "not_measured": "F32 views, other sizes and more than two views, other lattice steps, the states copied back, the cost of building the candidate array from Python dicts, more than one host thread for the baseline",
       "sets": doc_sets}
for f in d_frames:
    hip.hipFree(f.data)
eng.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict({spec.split("=", 1)[0]: kernel_stats(spec.split("=", 1)[1]) for spec in a.kernel_stats},
                                  note="rocprofv3 --kernel-trace --stats of a --trace-only --set run per candidate set: per round one haf_check_space with one and one with two device-resident views (the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
