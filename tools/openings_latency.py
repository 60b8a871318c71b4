#!/usr/bin/env python3
"""What the smallest free opening costs: haf_fit_openings on the device against the route a caller had before it -- a loop of
haf_check_grasps over the candidate openings -- and against haf_fit_openings_ref, the same definition on one host thread.

The set-up is tools/clearance_latency.py's: table1 rendered as a 640 x 480 U16 frame from camera A; the C3 request on it (56 x 56 grid,
20 rolls); the candidates of haf_top_grasps with k = 32 and -- its suppression leaves this scene only a few dozen -- with k = 1024,
min_vote 1 and the suppression off, handed over as haf_grasp_candidate arrays built once; the library's default (nominal) gripper and
opening parameters.  After a warm-up, the host wall clock of synchronised calls through the Python binding, the variants alternating
within one run so that drift hits them alike -- per candidate set:
  fit_device_shift0 / _shift1cm   haf_fit_openings, device-resident frame, max_shift 0 / 1 cm
  fit_host_shift0 / _shift1cm     haf_fit_openings, host frame (staged and uploaded again by the call: that cost is shown, not hidden)
  loop_check_grasps               BASELINE A: haf_check_grasps (device-resident frame) once per opening 2 j B, j = j_min .. j_max of the
                                  max_shift 0 call, the whole candidate array each time, until every candidate has had a free opening
                                  or the openings run out.  It cannot shift the gripper, so it answers the max_shift 0 question only
  host_ref_shift0                 BASELINE B: haf_fit_openings_ref on one host thread (--ref-calls calls: it takes far longer)
On a GPU box:
  python tools/openings_latency.py --calls 200 --out profiles/grasp_opening_time.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o open -- python tools/openings_latency.py --trace-only --set k32
                    # the kernels' own times -- one haf_fit_openings and one haf_check_grasps per round on the device-resident frame --,
                    # one trace per candidate set; then hand the stats to the measuring run:
  python tools/openings_latency.py --kernel-stats k32=DIR/.../open_kernel_stats.csv --out profiles/grasp_opening_time.json
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
ap.add_argument("--trace-only", action="store_true", help="run haf_fit_openings and haf_check_grasps on the device-resident frame alone and write nothing: the body of a rocprofv3 --kernel-trace --stats run")
ap.add_argument("--set", default="", metavar="k32|k1024_unsuppressed", help="this candidate set alone (with --trace-only: one trace per set)")
ap.add_argument("--kernel-stats", action="append", default=[], metavar="SET=CSV", help="the *_kernel_stats.csv of such a run of that set; may be given once per set")
a = ap.parse_args()

import pcdio  # noqa: E402
from render import render_depth, tilted_pose  # noqa: E402  (tools/render.py)
from haf_grasping_amd import capi  # noqa: E402

D = os.path.join(ROOT, "tests", "golden", "data")
W, H, K = 640, 480, dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)
POSE_FIELDS = ("grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector")
KERNELS = r"\b(k_clear_points(<[^>]*>)?|k_grasp_clear|k_grasp_slab|k_open_search)"


def stats(ns):
    us = np.sort(np.asarray(ns, np.float64)) / 1e3
    q = lambda p: float(us[min(len(us) - 1, int(p * len(us)))])
    return dict(calls=len(us), median_us=float(np.median(us)), p10_us=q(0.10), p90_us=q(0.90), min_us=float(us[0]), spread_p10_p90_us=q(0.90) - q(0.10))


def kernel_stats(path):
    """{kernel: calls, avg / min / max us} of the four kernels from a rocprofv3 *_kernel_stats.csv"""
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
pose = tilted_pose((0.21, -0.17, 0.6), (0.20, 0.13, 0.9))
depth = render_depth(xyz, pose, W, H, K["fx"], K["fy"], K["cx"], K["cy"])
eng = capi.Engine(os.path.join(D, "Features.txt"), os.path.join(D, "range21062012_allfeatures"), os.path.join(ROOT, "tests", "golden", "surrogate.model"),
                  n_rolls=20, roll_step_deg=9, max_points=1 << 20)
hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
inp = capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0))
frame = capi.depth_frame(depth, sensor_to_base=pose, **K)
d_frame = capi.depth_frame(device_array(hip, depth), width=W, height=H, dtype=np.uint16, sensor_to_base=pose, **K)
gripper = capi.gripper()
P0, P1 = capi.opening_params(), capi.opening_params(max_shift=0.01)
eng.score_frames([frame], [inp])
sets = {"k32": candidate_array(eng.top_grasps(k=32)[0]),
        "k1024_unsuppressed": candidate_array(eng.top_grasps(k=1024, min_vote=1, cell_radius=0, roll_window=0, min_dist_m=0.0)[0])}
if a.set:
    sets = {a.set: sets[a.set]}
INFO = capi.fit_openings_ref(frame, list(sets.values())[0], gripper, P0)[2]
OPENINGS = [2 * j * INFO["bin_m"] for j in range(INFO["j_min"], INFO["j_max"] + 1)]
GRIPPERS = [capi.gripper(opening=o, max_hits=P0.max_hits, min_between=P0.min_between) for o in OPENINGS]      # (every opening is exact in float32)


def loop_check_grasps(cands):
    """baseline A -> (the first free opening of every candidate, 0 without one; the calls it took)"""
    first = np.zeros(len(cands))
    for calls, g in enumerate(GRIPPERS, 1):
        rows, _ = eng.check_grasps(d_frame, cands, g)
        new = (rows["free"] == 1) & (first == 0)
        first[new] = g.opening
        if (first > 0).all():
            break
    return first, calls


if a.trace_only:
    mid = GRIPPERS[len(GRIPPERS) // 2]
    for _ in range(a.warmup + a.calls):
        for cands in sets.values():
            eng.fit_openings(d_frame, cands, gripper, P0)
            eng.check_grasps(d_frame, cands, mid)
    eng.close()
    sys.exit(0)

routes = {"fit_device_shift0": lambda c: eng.fit_openings(d_frame, c, gripper, P0), "fit_device_shift1cm": lambda c: eng.fit_openings(d_frame, c, gripper, P1),
          "fit_host_shift0": lambda c: eng.fit_openings(frame, c, gripper, P0), "fit_host_shift1cm": lambda c: eng.fit_openings(frame, c, gripper, P1),
          "loop_check_grasps": loop_check_grasps}
variants = {(route, name): (lambda call=call, cands=cands: call(cands)) for name, cands in sets.items() for route, call in routes.items()}
doc_sets = {}
for name, cands in sets.items():
    t0 = time.perf_counter_ns()
    want = capi.fit_openings_ref(frame, cands, gripper, P0)
    ref_ns = [time.perf_counter_ns() - t0]
    want1 = capi.fit_openings_ref(frame, cands, gripper, P1)
    for route, p, w in (("fit_device_shift0", P0, want), ("fit_host_shift0", P0, want), ("fit_device_shift1cm", P1, want1), ("fit_host_shift1cm", P1, want1)):
        got = variants[route, name]()
        assert got[0].tobytes() == w[0].tobytes() and got[1].tolist() == w[1].tolist() and got[2] == w[2], (route, name)
    first, loop_calls = loop_check_grasps(cands)
    sym = want[0]["sym_opening_m"]                          # (its fingers and palm are the nominal ones, ours a bin wider: it may be free sooner)
    assert (first[sym > 0] > 0).all() and (first[sym > 0] <= sym[sym > 0]).all(), "found at c = 0 implies free at that opening"
    for _ in range(a.ref_calls - 1):
        t0 = time.perf_counter_ns()
        capi.fit_openings_ref(frame, cands, gripper, P0)
        ref_ns.append(time.perf_counter_ns() - t0)
    doc_sets[name] = dict(n_grasps=len(cands), n_found_shift0=int(want[1].size), n_found_shift1cm=int(want1[1].size), info_shift0=want[2], info_shift1cm=want1[2],
                          loop_check_grasps_calls=loop_calls, candidate_openings=len(OPENINGS), host_us=dict(host_ref_shift0=stats(ref_ns)))
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
        if route.startswith("fit_"):
            for base in ("loop_check_grasps", "host_ref_shift0"):
                block[route]["below_%s_by_more_than_its_spread" % base] = bool(block[base]["median_us"] - block[route]["median_us"] > block[base]["spread_p10_p90_us"])
doc = {"tool": "tools/openings_latency.py: host wall clock of synchronised calls through the Python binding, variants alternating within one run (%d calls each after %d warm-up rounds; host_ref_shift0: %d calls, not alternating)" % (a.calls, a.warmup, a.ref_calls),
       "request": "table1 from camera A as a 640 x 480 U16 frame; candidates of haf_top_grasps(k = 32, and k = 1024 with min_vote 1 and no suppression) of the C3 request (56 x 56 grid, 20 rolls) as haf_grasp_candidate arrays built once; the default nominal gripper, the default opening parameters (max_shift 0) and the same with max_shift 1 cm",
       "baselines": "loop_check_grasps: haf_check_grasps on the device-resident frame once per opening 2 j B, j = j_min .. j_max, the whole array each time, until every candidate has had a free opening or the openings run out (answers max_shift 0 only); host_ref_shift0: haf_fit_openings_ref on one host thread",
       "not_measured": "other frame kinds and sizes, a mask, the histograms copied back, the cost of building the candidate array from Python dicts, more than one host thread for baseline B, a baseline loop that drops the candidates already free",
       "sets": doc_sets}
hip.hipFree(d_frame.data)
eng.close()
if a.kernel_stats:
    doc["kernel_trace_us"] = dict({spec.split("=", 1)[0]: kernel_stats(spec.split("=", 1)[1]) for spec in a.kernel_stats},
                                  note="rocprofv3 --kernel-trace --stats of a --trace-only --set run per candidate set: per round one haf_fit_openings (max_shift 0) and one haf_check_grasps at the middle opening, device-resident frame (the warm-up included)")
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
