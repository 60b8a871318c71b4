#!/usr/bin/env python3
"""Benchmark of the grasp-scoring hot path on MI355X.

Metric (BASELINE.json): grid-cell x rotation SVM evals/sec (whole job), plus end-to-end grasp latency per cloud.
Workload at every N: BASELINE config C5 -- synthetic 512x512 height map (524 288 points), 36 rolls of 5 degrees,
512x512 search area, seeded random libsvm RBF model with the full SV set (default nSV = 4096, D = 323) -- one cloud
per GPU per step (weak scaling: rolls x cells of independent clouds shard across ranks with no data-path collective;
the only exchange is one 8-byte RCCL all-reduce(max) per step that elects the best grasp of the batch).

A step = one pass of the whole hot path (bin -> integral -> mask -> features+text round trips+scale -> RBF decision
(fp16 screening pass -> three-pass kernel on its guard band) -> fp64 recheck tiers -> vote/argmax -> pose) over one cloud per rank, inputs already resident in HBM.

A plain run times the headline alone: model seed 42 (the median of the five seeds of a --full run on every box measured), `--warmup`
untimed and `--steps` timed steps.  --full adds everything else: the workload timed once per seed of --seeds with the median seed as
headline, label shares, the MFMA rate probe, the other contraction modes, two requests in flight, the hard and the trained model, the CPU
baselines, the grasp latencies (C2/C3/C4) and the C++-host multi-GPU path (each --no-* option drops one of them).
--dump-outputs DIR writes what the last timed step returned (roll records and grasp) to DIR/*.npy as float64.

  python bench.py --gpus 1 --steps 5 --warmup 1 [--dump-outputs DIR]
  python bench.py --gpus 1 --steps 20 --warmup 5 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_F16_MFMA_TFLOPS = 2500.0      # MI355X_MICROARCH.md: BF16/FP16 MFMA, dense
D_ATTR = 323                       # algorithmic work 2*D*nSV flop per eval, D unpadded
FULL_SEEDS = "1234,7,11,23,42"
PLAIN_SEEDS = "42"                 # the median seed of FULL_SEEDS in every --full run recorded (profiles/r0[45]_bench_*_default*.json)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement (per-seed median, label shares, MFMA probe, other contraction modes, two "
                         "requests in flight, hard and trained models, CPU baselines, grasp latencies, C++-host multi-GPU path); "
                         "off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step (the last seed's) returned -- roll records, grasp -- to DIR/<name>.npy as float64")
    ap.add_argument("--nsv", type=int, default=4096, help="support vectors of the seeded random model")
    ap.add_argument("--seeds", default=None,
                    help="seeds of the random model generator (tests/models.py): the workload is timed once per seed (same K steps, "
                         "same fences each) and `value` is the MEDIAN seed's rate; the per-seed lines are in `seeds`.  Default: "
                         "%s with --full, %s without" % (FULL_SEEDS, PLAIN_SEEDS))
    ap.add_argument("--no-label-stats", action="store_true", help="skip the per-seed positive-label share (one untimed debug run per seed)")
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--rolls", type=int, default=36)
    ap.add_argument("--roll-step", type=int, default=5)
    ap.add_argument("--precision", choices=["f32", "f16x3", "f16s"], default="f16s",
                    help="RBF contraction: f16s (default) = one fp16 MFMA screening pass over every evaluation, the three-pass "
                         "kernel only on what falls inside its rigorous guard band; f16x3 = three fp16 MFMA passes on the "
                         "hi/lo halves of the fp32 operands for every evaluation; f32 = one fp32 MFMA pass.  Identical labels.")
    ap.add_argument("--shard", choices=["clouds", "rolls"], default="clouds",
                    help="clouds (default, weak scaling): one cloud per GPU per step; rolls (strong scaling): ONE cloud per "
                         "step, its rolls split over the GPUs, roll records all-gathered (16 B each) and finalised on every rank")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-crop", type=int, default=70, help="grid size of the single-core CPU-baseline sample (one roll)")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-f32-side", action="store_true", help="skip the side measurements of the other contraction modes")
    ap.add_argument("--no-hard-side", action="store_true",
                    help="skip the side measurement on the ill-conditioned model (the committed libsvm-trained surrogate, C = 512, "
                         "replicated to bench size)")
    ap.add_argument("--no-trained-side", action="store_true",
                    help="skip the side measurement on the repo's large genuine libsvm model (tests/golden/trained.model.npz: 8964 SVs, "
                         "trained by the reference svm-train with an easy.py-style grid on 24000 harvested rows)")
    ap.add_argument("--no-cabi-side", action="store_true",
                    help="skip the side measurement of the C++-host multi-GPU path (haf_create_multi / haf_score_sharded: one "
                         "process, N GPUs, RCCL all-gather behind the C-ABI)")
    ap.add_argument("--cabi-child", action="store_true", help=argparse.SUPPRESS)   # internal: run that side measurement, print JSON
    ap.add_argument("--cabi-seed", type=int, default=1234, help=argparse.SUPPRESS)  # internal: the model seed of that side measurement
    return ap.parse_args()


def spawn_ranks(args, script=None, argv=None):
    """`python bench.py --gpus N` without a launcher: start one rank process per GPU ourselves (what torch.distributed.run
    would do), BEFORE anything in this process touches a GPU -- this parent never imports torch -- and wait for them.
    Rank 0's JSON line goes straight to our stdout.  Any rank failing fails the run.  (script / argv: the rank program and its
    arguments -- this file and our own by default; tests/test_distributed_cpu.py drives the same plumbing with a gloo stub.)"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + (sys.argv[1:] if argv is None else list(argv)), env=env))
    # poll ALL ranks: when one dies the others would sit in a collective until its timeout -- stop them at once
    rc, alive = 0, set(range(len(procs)))
    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                sys.stderr.write("bench.py: rank %d exited with %d; stopping the other ranks\n" % (r, code))
                for q in alive:
                    procs[q].terminate()
        if alive:
            time.sleep(0.2)
    return rc


def cabi_child(args):
    """The C++-host multi-GPU path, measured from ONE process: haf_create_multi over devices 0..N-1, the rolls of one C5
    request sharded 5,5,5,5,4,4,4,4-style, the cloud resident on device 0 and broadcast by RCCL, one ncclAllGather of
    the roll records per request, haf_finalize.  Strong scaling of a single request.  Prints one JSON object."""
    import torch
    import models
    from haf_grasping_amd import capi
    n = args.gpus
    data = os.path.join(ROOT, "tests", "golden", "data")
    feat, rng_file = os.path.join(data, "Features.txt"), os.path.join(data, "range21062012_allfeatures")
    tmp = tempfile.mkdtemp(prefix="hafbench_cabi_")
    model_path = os.path.join(tmp, "rand%d.model" % args.nsv)
    models.write_random_model(model_path, args.nsv, D=D_ATTR, seed=args.cabi_seed, balanced=True)
    G = args.grid
    xyz = models.synthetic_cloud(grid=G, k=2, seed=0)
    torch.cuda.set_device(0)
    d_xyz = torch.from_numpy(xyz).cuda()
    cloud = (d_xyz.data_ptr(), xyz.shape[0], 3)
    inp = capi.default_input(grasp_area_length_x=G, grasp_area_length_y=G)
    me = capi.MultiEngine(feat, rng_file, model_path, list(range(n)), capi.SHARD_ROLLS, grid_h=G, grid_w=G, n_rolls=args.rolls,
                          roll_step_deg=args.roll_step, max_clouds=1, max_points=G * G * 2, flags=capi.FLAG_PROFILE)
    info = me.info()
    for _ in range(max(1, args.warmup)):
        out = me.score_sharded(cloud, inp)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tim = []
    for _ in range(args.steps):
        out = me.score_sharded(cloud, inp)
        tim.append(me.last_timing())
    dt = time.perf_counter() - t0
    stage = [me.shard_stage_ms(s) for s in range(n)]
    me.close()
    print(json.dumps({"value": out["n_evals"] * args.steps / dt, "unit": "evals/s", "ms_per_request": 1e3 * dt / args.steps,
                      "n_devices": n, "rccl_ranks": info["n_ranks"], "rccl_version": info["rccl_version"], "scaling": "strong",
                      "evals_per_request": out["n_evals"], "shard_svm_ms": [st["svm"] if st else None for st in stage],
                      "bcast_us": float(np.median([t["bcast_us"] for t in tim])), "gather_us": float(np.median([t["collective_us"] for t in tim])),
                      "shard_ms": [float(np.median([t["shard_ms"][s] for t in tim])) for s in range(n)],
                      "timing_note": "host wall-clock inside haf_score_sharded (haf_multi_last_timing), medians over the steps: ncclBroadcast of the "
                                     "device-resident cloud, every shard's own haf_score_rolls, the ncclAllGather + the copy of the gathered records to the host",
                      "best": {"eval": out["eval"], "row": out["best_row"], "col": out["best_col"], "roll": out["best_roll"]},
                      "workload": "ONE C5 request (cloud on device 0 -> ncclBroadcast), rolls sharded over %d GPUs in one process, "
                                  "one ncclAllGather of the 16-byte roll records, haf_finalize" % n}), flush=True)


def run_cabi_side(args, world, seed):
    """Rank 0, after the ranks have let go of the GPUs: the measurement above in a fresh child process (a crash there cannot
    take the bench line with it)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cabi-child", "--gpus", str(world), "--steps", str(max(3, min(args.steps, 10))),
           "--warmup", "1", "--nsv", str(args.nsv), "--grid", str(args.grid), "--rolls", str(args.rolls), "--roll-step", str(args.roll_step),
           "--cabi-seed", str(seed)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                           "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "TORCHELASTIC_RUN_ID")}
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180, text=True)
        if p.returncode != 0:
            return {"error": "child exited with %d: %s" % (p.returncode, p.stderr.strip()[-400:])}
        return json.loads(p.stdout.strip().splitlines()[-1])
    except Exception as ex:          # noqa: BLE001 -- a side measurement must never cost the main line
        return {"error": repr(ex)}


SCREEN_FORMS = ("plain", "sumsq", "centred-remainder/exp", "centred-remainder/poly")


def profile_entry(args, model_key, precision, n_sv, kernel):
    """The committed rocprofv3 evidence for ONE kernel instance of ONE profiled run, or None.  profiles/index.json (written by
    tools/collect_profiles.sh from the passes of tools/profile_round.sh) lists, per profiled run -- keyed "<model>/<precision>", e.g.
    "seed42/f16s", "trained/f16s", "seed42/f16x3" -- the workload, the build commit and per kernel instance the full-size average under
    --kernel-trace (avg_ms), the MFMA-busy share of the SQ pass (mfma_busy) and the HBM bytes of the FETCH_SIZE / WRITE_SIZE passes
    (hbm_bytes).  A figure is only handed out when grid, rolls, SV count, model, contraction mode AND kernel instance (template
    arguments included: the screening form) are those of the run being reported; PMC counters cannot be read from inside this process."""
    try:
        with open(os.path.join(ROOT, "profiles", "index.json")) as f:
            idx = json.load(f)
        run = idx["runs"].get("%s/%s" % (model_key, precision))
        if not run:
            return None
        w = run["workload"]
        if (w["grid"], w["rolls"], w["n_sv"]) != (args.grid, args.rolls, n_sv):
            return None
        k = run["kernels"].get(kernel)
        if not k:
            return None
        return dict(k, source="profiles/index.json run %s/%s (%s, build %s)" % (model_key, precision, idx.get("round", "?"), idx.get("commit", "?")))
    except (OSError, KeyError, ValueError, TypeError):
        return None


def cpu_baseline(feat, rng_file, model_path, xyz, args):
    """The oracle (scalar C port of the reference's arithmetic incl. both text round trips, in-process) on a bounded
    sample of the same workload: the central crop x crop cells of the same cloud, one roll, same model.  Timed on one
    core and on all host cores (OpenMP over feature lines / rows); `value` is the all-cores figure."""
    from oracle import oracle as O
    o = O.Oracle(feat, rng_file, model_path)

    def run(c, threads):
        half = c * 0.01 / 2
        sel = (np.abs(xyz[:, 0]) < half) & (np.abs(xyz[:, 1]) < half)
        pts = np.ascontiguousarray(xyz[sel])
        os.environ["HAFO_THREADS"] = str(threads)
        t0 = time.perf_counter()
        r = o.run(pts, O.make_cfg(H=c, W=c, n_rolls=1, roll_step_deg=args.roll_step), O.make_input(length_x=c, length_y=c),
                  debug=False)
        return r["n_evals"], time.perf_counter() - t0

    cores = len(os.sched_getaffinity(0))
    n1, t1 = run(args.cpu_crop, 1)
    per_core = n1 / t1
    # all cores: size the crop for roughly 10 s of work
    c_all = int(min(args.grid, 14 + (per_core * cores * 10.0) ** 0.5))
    na, ta = run(c_all, cores)
    os.environ["HAFO_THREADS"] = "1"
    ref = reference_tools_baseline(o, O, rng_file, model_path, xyz, args)
    return dict(value=na / ta, unit="evals/s", cores=cores, kind="port", single_core_value=per_core, reference_tools=ref,
                sample="oracle/haf_oracle.c end to end (features, %%.4g/%%g text round trips, svm-scale, libsvm-order fp64 "
                       "RBF over nSV=%d, vote), same cloud and model, 1 roll: central %dx%d crop on 1 core (%d evals in "
                       "%.1f s), central %dx%d crop on %d cores (%d evals in %.1f s)"
                       % (args.nsv, args.cpu_crop, args.cpu_crop, n1, t1, c_all, c_all, cores, na, ta))


def reference_tools_baseline(o, O, rng_file, model_path, xyz, args):
    """The reference's own SVM stage as the server runs it (server.cpp:775-788): the REAL svm-scale and svm-predict
    binaries (built from /root/reference/libsvm-3.12 into oracle/_ref) on the feature text file of one roll of a
    40x40 crop, through temp files, 1 core.  None when oracle/_ref is not present."""
    import subprocess
    ref = O.ref_dir()
    if not (os.path.exists(os.path.join(ref, "svm-scale")) and os.path.exists(os.path.join(ref, "svm-predict"))):
        return dict(kind="reference", value=None, unit="evals/s", cores=1,
                    sample="NOT MEASURED: oracle/_ref/svm-scale and svm-predict are absent.  They are built from "
                           "/root/reference/libsvm-3.12 by `make -C oracle ref` in the build container only (git-ignored, they "
                           "travel to the GPU box with the snapshot); a clean checkout has the oracle port figure alone")
    c = 40
    half = c * 0.01 / 2
    sel = (np.abs(xyz[:, 0]) < half) & (np.abs(xyz[:, 1]) < half)
    pts = np.ascontiguousarray(xyz[sel])
    tmp = tempfile.mkdtemp(prefix="hafref_")
    f = os.path.join(tmp, "features.txt")
    t0 = time.perf_counter()
    n = o.dump_feature_file(pts, O.make_cfg(H=c, W=c, n_rolls=1, roll_step_deg=args.roll_step), O.make_input(length_x=c, length_y=c), 0, f)
    t_feat = time.perf_counter() - t0
    t0 = time.perf_counter()
    with open(f + ".scale", "w") as out:
        subprocess.run([os.path.join(ref, "svm-scale"), "-r", rng_file, f], stdout=out, check=True)
    t_scale = time.perf_counter() - t0
    t0 = time.perf_counter()
    subprocess.run([os.path.join(ref, "svm-predict"), f + ".scale", model_path, f + ".out"], stdout=subprocess.DEVNULL, check=True)
    t_pred = time.perf_counter() - t0
    return dict(kind="reference", value=n / (t_feat + t_scale + t_pred), unit="evals/s", cores=1,
                sample="real svm-scale + svm-predict (oracle/_ref) on the oracle's feature file of a %dx%d crop, 1 roll, nSV=%d: "
                       "%d evals; features+text %.2f s, svm-scale %.2f s, svm-predict %.2f s" % (c, c, args.nsv, n, t_feat, t_scale, t_pred))


def latency_small(feat, rng_file, device, flags, trained_model=None, headline_model=None):
    """BASELINE configs C2 (pcd2.pcd, 32x32 cm area, 12 rolls) and C3 (table1_mult_obj, 56x56 cm, 20 rolls of 9 degrees), surrogate
    model, host-resident cloud: wall time of one haf_score call including the PCIe copies -- the second half of the metric."""
    from haf_grasping_amd import capi
    model = os.path.join(ROOT, "tests", "golden", "surrogate.model")
    data = os.path.join(ROOT, "tests", "golden", "data")

    def one(name, pcd, inp, model=model, **cfg):
        xyz = capi.load_pcd(os.path.join(data, pcd))
        eng = capi.Engine(feat, rng_file, model, device=device, flags=flags, max_points=1 << 18, **cfg)
        res = {}
        for registered in (False, True):
            if registered:
                eng.register_host(xyz)         # haf_register_host_cloud: the caller's buffer page-locked once, on_device = 2
            for _ in range(3):
                out = eng.score(xyz, inp)
            ts = []
            for _ in range(30):
                t0 = time.perf_counter()
                out = eng.score(xyz, inp)
                ts.append(time.perf_counter() - t0)
            res[registered] = (1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)))
        form = eng.screen_form()
        eng.close()
        return dict(workload=name % xyz.shape[0], ms_median=res[False][0], ms_min=res[False][1],
                    ms_median_registered_host=res[True][0], ms_min_registered_host=res[True][1],
                    evals=out["n_evals"], eval=out["eval"], screening_form=form,
                    note="ms_median: the cloud in ordinary (pageable) host memory, staged through the engine's pinned block; "
                         "ms_median_registered_host: the same numpy buffer page-locked once with haf_register_host_cloud (on_device = 2)")

    c2 = one("C2: pcd2.pcd %d pts, 32x32 cm, 12 rolls, surrogate model nSV=172, host cloud (PCIe included)", "pcd2.pcd",
             capi.default_input(grasp_area_length_x=32, grasp_area_length_y=32))
    c3 = one("C3: table1_mult_obj %d pts, 56x56 cm, centre (0.13, 0.25, 0), 20 rolls x 9 deg, surrogate model nSV=172, host cloud (PCIe included)",
             "table1_mult_obj_rcs_1428580506606673.pcd",
             capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0)), n_rolls=20, roll_step_deg=9)
    c2["c3"] = c3
    if trained_model is not None:
        # the same C3 request against the trained model (8964 SVs: past the small-request shortcut, every decision tier in play)
        c2["c3_trained"] = one("C3 request (table1_mult_obj %d pts, 56x56 cm, 20 rolls x 9 deg) against the TRAINED model nSV=8964 "
                               "(tests/golden/trained.model.npz), host cloud (PCIe included)", "table1_mult_obj_rcs_1428580506606673.pcd",
                               capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0)),
                               model=trained_model, n_rolls=20, roll_step_deg=9)
    if headline_model is not None:
        # ... and against the headline's random model (median seed, nSV = 4096): a reference-sized request with a model of thousands of
        # SVs does not fill the chip -- the screening pass and the three-pass tier are cut into SV ranges by the live counts (round 4)
        c2["c3_headline_model"] = one("C3 request (table1_mult_obj %d pts, 56x56 cm, 20 rolls x 9 deg) against the headline's random model "
                                      "(median seed, nSV=4096), host cloud (PCIe included)", "table1_mult_obj_rcs_1428580506606673.pcd",
                                      capi.default_input(grasp_area_length_x=56, grasp_area_length_y=56, grasp_area_center=(0.13, 0.25, 0.0)),
                                      model=headline_model, n_rolls=20, roll_step_deg=9)
    # C4: the eight pcd files as ONE batched call (haf_score_batch), 20 rolls of 9 degrees each: what a server that collects goals pays per cloud
    clouds = [capi.load_pcd(os.path.join(data, "pcd%d.pcd" % i)) for i in range(1, 9)]
    inputs = [capi.default_input() for _ in clouds]
    eng = capi.Engine(feat, rng_file, model, device=device, flags=flags, max_clouds=len(clouds), max_points=1 << 18, n_rolls=20, roll_step_deg=9)
    for _ in range(3):
        outs = eng.score_batch(clouds, inputs)
    ts = []
    for _ in range(30):
        t0 = time.perf_counter()
        outs = eng.score_batch(clouds, inputs)
        ts.append(time.perf_counter() - t0)
    eng.close()
    c2["c4"] = dict(workload="C4: pcd1..pcd8 (%d pts) in one batched call, 32x44 cm, 20 rolls x 9 deg, surrogate model nSV=172, host clouds (PCIe included)"
                    % sum(c.shape[0] for c in clouds), ms_median=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)),
                    ms_per_cloud=1e3 * float(np.median(ts)) / len(clouds), evals=int(sum(o["n_evals"] for o in outs)), evals_best=[int(o["eval"]) for o in outs])
    return c2


def reduce_over_ranks(dist, torch, device, world, elapsed_s, evals, step_ms, coll_us, kernel_ms):
    """The contract's reductions for one timed run -- MAX of the elapsed time over the ranks, SUM of the evaluations -- and an
    all-gather of every rank's own (ms per step, collective us, kernel ms), so that a multi-GPU run explains itself.
    -> (elapsed_max_s, total_evals, per_rank [[step_ms, coll_us, kernel_ms] per rank])"""
    t = torch.tensor([elapsed_s], dtype=torch.float64, device=device)
    ev = torch.tensor([evals], dtype=torch.int64, device=device)
    mine = torch.tensor([step_ms, coll_us or 0.0, kernel_ms], dtype=torch.float64, device=device)
    allr = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(allr, mine)
    per_rank = [[float(v) for v in q.tolist()] for q in allr]
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(ev, op=dist.ReduceOp.SUM)
    return float(t.item()), int(ev.item()), per_rank


def ranks_block(world, per_rank, shard, use_dist, dist=None, rccl_version=None, fallback=None):
    """The `ranks` object of the JSON line: how the ranks were launched, what the communicator saw, every rank's own timings."""
    return {"world_size": world, "launched_by": "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else
            ("bench.py (self-spawned ranks)" if world > 1 else "single process"),
            "per_rank_ms_per_step": [q[0] for q in per_rank] if per_rank else [fallback[0]],
            "per_rank_collective_us": [q[1] for q in per_rank] if per_rank else None,
            "per_rank_kernel_ms": [q[2] for q in per_rank] if per_rank else [fallback[1]],
            "collective": ("one all-gather of the 16-byte roll records per step" if shard == "rolls" else
                           "one 8-byte all-reduce(max) per step") + " (host wall-clock incl. its synchronisation, median over the steps of the median seed)",
            "rccl_world_size": dist.get_world_size() if use_dist else 1,
            "rccl_version": rccl_version}


GRASP_FIELDS = ("eval", "grasp_point1", "grasp_point2", "averaged_grasp_point", "approach_vector", "roll", "best_row", "best_col",
                "best_roll", "best_vote", "rolls_done", "n_evals")


def dump_outputs(dirname, records, out):
    """--dump-outputs: what the caller of the timed path receives from its last step -- the roll records of haf_score_rolls (all rolls
    of the request) and the grasp of haf_finalize -- one float64 .npy per field (a few hundred bytes in all).  The grasp's n_rechecked
    is left out: it counts the work of the recheck tiers, not a result."""
    from haf_grasping_amd import capi
    os.makedirs(dirname, exist_ok=True)
    arrays = {"roll_" + f: records[f] for f in capi.ROLL_RECORD_DTYPE.names}
    arrays.update({"grasp_" + k.replace("grasp_", ""): out[k] for k in GRASP_FIELDS})     # grasp_eval, grasp_point1, ...
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.asarray(a, dtype=np.float64))


def main():
    args = parse()
    if args.cabi_child:
        return cabi_child(args)
    if "RANK" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args))          # one rank per GPU, started here; this process stays off the GPUs
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE %d != --gpus %d" % (world, args.gpus))

    import torch
    import torch.distributed as dist
    torch.cuda.set_device(local_rank)
    use_dist = "RANK" in os.environ and "MASTER_ADDR" in os.environ
    if use_dist:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))   # RCCL

    import models
    from haf_grasping_amd import capi
    from haf_grasping_amd import distributed as hd

    data = os.path.join(ROOT, "tests", "golden", "data")
    feat, rng_file = os.path.join(data, "Features.txt"), os.path.join(data, "range21062012_allfeatures")
    tmp = tempfile.mkdtemp(prefix="hafbench_%d_" % rank)
    if args.seeds is None:
        args.seeds = FULL_SEEDS if args.full else PLAIN_SEEDS
    seeds = [int(t) for t in args.seeds.split(",") if t.strip()]
    if not seeds:
        raise SystemExit("--seeds needs at least one seed")

    G = args.grid
    xyz = models.synthetic_cloud(grid=G, k=2, seed=rank if args.shard == "clouds" else 0)
    d_xyz = torch.from_numpy(xyz).cuda()                    # resident in HBM before the timed region
    cloud = (d_xyz.data_ptr(), xyz.shape[0], 3)
    inp = capi.default_input(grasp_area_length_x=G, grasp_area_length_y=G)

    def make_engine(precision, model_file=None):
        return capi.Engine(feat, rng_file, model_file or model_path, device=local_rank, grid_h=G, grid_w=G, n_rolls=args.rolls,
                           roll_step_deg=args.roll_step, max_clouds=1, max_points=G * G * 2,
                           flags=capi.FLAG_PROFILE | {"f32": capi.FLAG_FP32_MFMA, "f16x3": capi.FLAG_SPLIT_F16, "f16s": 0}[precision])

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def run(eng, steps, warmup, collective):
        coll_us = []                                        # host wall-clock of the step's one collective (incl. its sync)

        def step():
            """-> (this rank's roll records, the grasp, the records of all rolls the grasp was finalised from)"""
            if args.shard == "rolls" and collective:
                first, count = hd.roll_shard(args.rolls, world, rank)
                local = eng.score_rolls([cloud], [inp], first, count)
                tc = time.perf_counter()
                full = hd.gather_roll_records(local, args.rolls, device="cuda")[0]   # one all-gather of 16 B per roll
                coll_us.append(1e6 * (time.perf_counter() - tc))
                return local[0], eng.finalize(inp, full), full
            rec = eng.score_rolls([cloud], [inp], 0, args.rolls)[0]
            out = eng.finalize(inp, rec)
            if collective:
                tc = time.perf_counter()
                hd.best_of_batch(out["best_vote"], tag=rank, device="cuda")   # one 8-byte all-reduce(max) over xGMI (RCCL)
                coll_us.append(1e6 * (time.perf_counter() - tc))
            return rec, out, rec
        for _ in range(warmup):
            step()
        svm_ms, stage_acc, evals, rechecked, strict, refined, n_i8, n_fp64 = [], {}, 0, 0, 0, 0, 0, 0
        del coll_us[:]
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            rec, out, records = step()
            evals += int(rec["n_evals"].sum())
            c = eng.last_counts()
            rechecked += c["n_rechecked"]
            strict += c["n_strict"]
            refined += c["n_refined"]
            ex = eng.last_exact_tiers()
            n_i8 += ex["n_integer"]
            n_fp64 += ex["n_fp64"]
            st = eng.stage_ms()
            svm_ms.append(st["svm"])
            for k, v in st.items():
                stage_acc[k] = stage_acc.get(k, 0.0) + v
        fence()
        return dict(low_rank=eng.screen_low_rank(), form=eng.screen_form(),
                    elapsed=time.perf_counter() - t0, coll_us=float(np.median(coll_us)) if coll_us else None, evals=evals, steps=steps, svm_s=float(np.mean(svm_ms)) * 1e-3,
                    stage_ms={k: v / steps for k, v in stage_acc.items()}, rechecked=rechecked / steps,
                    strict=strict / steps, refined=refined / steps, exact_integer=n_i8 / steps, fp64=n_fp64 / steps, out=out, records=records)

    def positive_share(model_file):
        """share of the evaluations libsvm labels with label[0] (untimed; a debug engine that keeps the label grids)"""
        e = capi.Engine(feat, rng_file, model_file, device=local_rank, grid_h=G, grid_w=G, n_rolls=args.rolls, roll_step_deg=args.roll_step,
                        max_clouds=1, max_points=G * G * 2, flags=capi.FLAG_KEEP_DEBUG)
        e.score_rolls([cloud], [inp], 0, args.rolls)
        pos = n = 0
        for roll in range(args.rolls):
            lab = e.debug(capi.DBG_LABELS, 0, roll)
            m = e.debug(capi.DBG_MASK, 0, roll) == 1
            pos += int((lab[m] == 1).sum())
            n += int(m.sum())
        e.close()
        return pos / max(1, n)

    # the same workload once per model seed: K timed steps between the same fences each; the headline is the MEDIAN seed
    runs = []
    for sd in seeds:
        mp = os.path.join(tmp, "rand%d_s%d.model" % (args.nsv, sd))
        models.write_random_model(mp, args.nsv, D=D_ATTR, seed=sd, balanced=True)
        eng = make_engine(args.precision, mp)
        r = run(eng, args.steps, args.warmup, use_dist)
        eng.close()
        per_rank, el, tot = None, r["elapsed"], r["evals"]
        if use_dist:
            el, tot, per_rank = reduce_over_ranks(dist, torch, "cuda", world, r["elapsed"], r["evals"], 1e3 * r["elapsed"] / args.steps,
                                                  r["coll_us"], r["svm_s"] * 1e3)
        runs.append(dict(seed=sd, model=mp, res=r, elapsed=el, total_evals=tot, per_rank=per_rank))
    ranked = sorted(runs, key=lambda q: q["total_evals"] / q["elapsed"])
    med = ranked[(len(ranked) - 1) // 2]                    # lower median: never better than half of the seeds
    res, elapsed, total_evals, model_path = med["res"], med["elapsed"], med["total_evals"], med["model"]
    if args.dump_outputs and rank == 0:
        # the last timed step of the run: the last seed's (fixed by the arguments, unlike the median seed)
        dump_outputs(args.dump_outputs, runs[-1]["res"]["records"], runs[-1]["res"]["out"])

    def roofline(r, precision, nsv=None, model_key=None):
        """model_key: which profiled run of profiles/index.json this result may be compared with ("seed42", "trained", "hard"; None: none)"""
        nsv = nsv or args.nsv
        evals_per_launch = r["evals"] / r["steps"]
        flop = evals_per_launch * 2.0 * D_ATTR * nsv                # algorithmic: 646*nSV per eval, ONE pass
        achieved = flop / r["svm_s"] / 1e12
        peak = PEAK_F32_MFMA_TFLOPS if precision == "f32" else PEAK_F16_MFMA_TFLOPS
        lr = precision == "f16s" and bool(r.get("low_rank", {}).get("last_used"))
        form = r.get("form")
        var = SCREEN_FORMS.index(form) if form in SCREEN_FORMS else 0
        # the kernel INSTANCE (template arguments included): the profile of another screening form is another kernel
        if precision == "f16s":
            kernel, instance = ("k_svm_screen_lr", "k_svm_screen_lr<%d, true, false>" % var) if lr else ("k_svm_screen", "k_svm_screen<%d, false>" % var)
        elif precision == "f16x3":
            kernel, instance = "k_svm_rbf_h", "k_svm_rbf_h<false, false>"
        else:
            kernel, instance = "k_svm_rbf", "k_svm_rbf"
        prof = profile_entry(args, model_key, precision, nsv, instance) if model_key else None
        o = {"kernel": kernel, "kernel_instance": instance, "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
             "frac": achieved / peak, "traffic": prof.get("hbm_bytes") if prof else None, "kernel_ms": r["svm_s"] * 1e3,
             "flop_per_launch": flop,
             "frac_note": "frac = ALGORITHMIC flop (646 x nSV per evaluation, SURVEY 8d) / kernel time / dense peak -- for the low-rank form that includes "
                          "an algorithmic saving, it is not matrix-pipe utilisation: see frac_executed and mfma_busy"}
        if prof and prof.get("avg_ms"):
            # both readings of the same kernel instance: HIP events in this run (`frac`) and the committed rocprofv3 summary (the profiler's runs are ~3 % slower)
            fr = flop / (prof["avg_ms"] * 1e-3) / 1e12 / peak
            if fr <= 1.0:                                    # a figure above the peak can only be a mismatched profile: never published
                o.update({"kernel_ms_rocprof": prof["avg_ms"], "frac_rocprof": fr, "rocprof_source": prof["source"]})
            if prof.get("mfma_busy") is not None:
                o["mfma_busy"] = prof["mfma_busy"]           # SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs / (GRBM_GUI_ACTIVE / 8), tracked PMC pass
        if precision == "f16x3":
            # three fp16 passes over K padded to 336 execute 3*336/323 = 3.12 times the algorithmic flop: the ceiling
            # of `frac` for this split-precision contraction is 0.32, not 1
            executed = flop * 3.0 * 336.0 / D_ATTR
            o.update({"passes": 3, "executed_tflops": executed / r["svm_s"] / 1e12,
                      "frac_executed": executed / r["svm_s"] / 1e12 / peak,
                      "note": "fp32 operands split into fp16 hi+lo; x.s = xh.sh + xl.sh + xh.sl (3 MFMA passes, fp32 "
                              "accumulate); algorithmic flop counted once, per SURVEY.md 8(d)"})
        if precision == "f16s" and lr:
            # The HAF attributes are linear functionals of the window spanning `rank` dimensions: the sweep runs on rank + 21 SHAF slots
            # padded to 192 (6 k-steps instead of 10), behind a projection of the 320-slot operand (320 x 192 per evaluation).  `frac`
            # stays what SURVEY.md 8(d) defines -- ALGORITHMIC flop (646 nSV per evaluation) over the time of the kernel, projection
            # prologue included (stage 'svm' = k_svm_screen_lr + the two compaction launches) -- the executed flop are fewer
            executed = evals_per_launch * 2.0 * (192.0 * nsv + 320.0 * 192.0)
            o.update({"passes": 1, "low_rank": {"rank": r["low_rank"]["rank"], "slots": 192, "executed_over_algorithmic": executed / flop},
                      "executed_tflops": executed / r["svm_s"] / 1e12, "frac_executed": executed / r["svm_s"] / 1e12 / peak,
                      "note": "single fp16 MFMA pass over every evaluation in the LOW-RANK form (centred operands; screening_form says which epilogue): the 299 HAF slots are linear "
                              "functionals of the 15x15 window (fv.cpp:141-199) spanning %d dimensions, so the kernel's prologue forms y = fp16(B'p) (B: an "
                              "orthonormal basis of that span + the 21 SHAF slots, 192 columns; 480 MFMAs per 64 evaluations) and its sweep runs over the "
                              "support vectors with K = 192; the guard band carries what the projection drops (the '%%.4g' rounding and the fp32 roundings of "
                              "the reference's feature arithmetic, bounded per evaluation) and the rounding of y; "
                              "evaluations inside the band are re-done by the tiers behind, so the labels are libsvm's" % r["low_rank"]["rank"],
                      "refined_per_launch": r["refined"], "refined_share": r["refined"] / max(1.0, evals_per_launch),
                      "refine_ms": r["stage_ms"].get("refine")})
        elif precision == "f16s":
            executed = flop * 320.0 / D_ATTR
            o.update({"passes": 1, "executed_tflops": executed / r["svm_s"] / 1e12, "frac_executed": executed / r["svm_s"] / 1e12 / peak,
                      "note": "single fp16 MFMA pass over every evaluation; K = 320 slots for the 323 attributes (three pairs of "
                              "Features.txt rows are the same feature with the same range and share a slot; the norm terms are the "
                              "accumulator's initial value and a common factor, not K slots); evaluations inside its rigorous guard "
                              "band are re-done by the three-pass kernel (stage 'refine') and the fp64 tiers, so the labels are libsvm's",
                      "refined_per_launch": r["refined"], "refined_share": r["refined"] / max(1.0, evals_per_launch),
                      "refine_ms": r["stage_ms"].get("refine")})
        return o

    if rank == 0:
        line = {
            "metric": "grid-cell x rotation SVM evals/sec",
            "value": total_evals / elapsed,
            "unit": "evals/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak" if args.shard == "clouds" else "strong", "vs_baseline": None,
            "dtype": {"f32": "f32", "f16x3": "f16x3", "f16s": "f16"}[args.precision],
            "data": "synthetic",
            # (the driver keeps the first ~100 characters of `workload`: what identifies the model comes first)
            "config": {"workload": "C5 nSV=%d D=323 gamma=1/323 random RBF model (%s); synthetic %dx%d heightmap, %d pts, "
                                   "%d rolls x %d deg, %dx%d cm area, one cloud per GPU per step, resident in HBM"
                                   % (args.nsv, ("median of seeds %s: %d" % (",".join(str(q) for q in seeds), med["seed"])) if len(seeds) > 1
                                      else "seed %d" % med["seed"], G, G, xyz.shape[0], args.rolls, args.roll_step, G, G),
                       "evals_per_cloud": int(res["evals"] / args.steps), "n_sv": args.nsv, "grid": G, "rolls": args.rolls,
                       "contraction": args.precision,
                       "sharding": ("clouds (1 per GPU); all-reduce(max) of an 8-byte best-grasp key per step" if args.shard == "clouds"
                                    else "rolls of one cloud split over the GPUs; all-gather of the 16-byte roll records per step")},
            "roofline": roofline(res, args.precision, model_key="seed%d" % med["seed"]),
            # the whole step against the same roof: algorithmic flop of the dominant contraction / ms_per_step / dense peak of its dtype
            "end_to_end_frac": (res["evals"] / res["steps"]) * 2.0 * D_ATTR * args.nsv / (elapsed / args.steps) / 1e12 /
                               (PEAK_F32_MFMA_TFLOPS if args.precision == "f32" else PEAK_F16_MFMA_TFLOPS),   # rank 0's GPU against one GPU's peak
            "seeds": {"generator": "tests/models.py write_random_model(nsv, seed, balanced=True): SV values U(-1,1), coef U(0,2) x class sign, "
                                   "sum(coef) = 0, gamma = 1/323, rho 0.01",
                      "headline": "%s seed %d (value, ms_per_step, roofline, stage_ms_per_step are that seed's run)"
                                  % ("median" if len(seeds) > 1 else "the one", med["seed"]),
                      "min_value": ranked[0]["total_evals"] / ranked[0]["elapsed"], "min_seed": ranked[0]["seed"],
                      "max_value": ranked[-1]["total_evals"] / ranked[-1]["elapsed"], "max_seed": ranked[-1]["seed"],
                      "worst_over_median_ms": (ranked[0]["elapsed"] / ranked[0]["res"]["steps"]) / (elapsed / args.steps),
                      "per_seed": [{"seed": q["seed"], "value": q["total_evals"] / q["elapsed"],
                                    "ms_per_step": 1e3 * q["elapsed"] / args.steps,
                                    "refined_share": q["res"]["refined"] / max(1.0, q["res"]["evals"] / q["res"]["steps"]),
                                    "three_pass_tier": q["res"]["refined"], "exact_integer_tier": q["res"]["exact_integer"],
                                    "fp64_mfma_tier": q["res"]["fp64"], "strict_order_tier": q["res"]["strict"],
                                    "screening_form": q["res"]["form"],
                                    "kernel_ms": q["res"]["svm_s"] * 1e3, "refine_ms": q["res"]["stage_ms"].get("refine"),
                                    "recheck_ms": q["res"]["stage_ms"].get("recheck"),
                                    "positive_label_share": (positive_share(q["model"]) if (world == 1 and args.full and not args.no_label_stats)
                                                             else None),
                                    "best": {"eval": q["res"]["out"]["eval"], "row": q["res"]["out"]["best_row"],
                                             "col": q["res"]["out"]["best_col"], "roll": q["res"]["out"]["best_roll"]}}
                                   for q in runs]},
            "stage_ms_per_step": res["stage_ms"],
            "prestages_hbm": (lambda ms, b: {"kernels": "k_bin + k_integral + k_mask_count/k_scan/k_compact + k_vote_cells/k_vote_pick",
                                             "algorithmic_bytes": b, "ms": ms, "GBps": b / ms / 1e6, "peak_GBps": 8000.0,
                                             "frac": b / ms / 1e6 / 8000.0,
                                             "note": "SURVEY 8(d): 12 B per cell per roll + 12 B per point per roll.  About twenty launches of "
                                                     "5-50 us (bucket sort + tile binning without global atomics, exactness-checked parallel "
                                                     "integral image, mask/scan/compact, vote) with 4-5 us gaps: 1.5 % of the step"})(
                res["stage_ms"]["bin"] + res["stage_ms"]["integral"] + res["stage_ms"]["mask"] + res["stage_ms"]["vote"],
                12.0 * args.rolls * (G * G + xyz.shape[0])),
            "rechecked_per_step": {"three_pass_tier": res["refined"], "exact_integer_tier": res["exact_integer"],
                                   "fp64_mfma_tier": res["fp64"], "strict_order_tier": res["strict"],
                                   "note": "evaluations per step that ENTER each tier behind the screening pass: three-pass fp16 kernel (PRECISE "
                                           "form), exact-integer tier (int8 digit planes, csrc/exact8.hip), fp64 MFMA tier, libsvm-order tier"},
            "best": {"eval": res["out"]["eval"], "row": res["out"]["best_row"], "col": res["out"]["best_col"],
                     "roll": res["out"]["best_roll"]},
        }
        if args.full and args.precision == "f16s":
            # Context for `roofline.frac`: what THIS GPU sustains on a bare loop of the same MFMA instruction (random operands in
            # registers, two 4-wave workgroups per CU, ~20 ms; libhafgrasp_testing.so, testkernels.hip).  The chip runs the matrix
            # pipe at the clock it can hold under the load, and that differs between the boxes of a pool.
            try:
                tl = capi.testlib()
                probe = []
                tf = C.c_double()
                for _ in range(3):
                    if tl.haf_test_mfma_rate(local_rank, 36000, C.byref(tf)) == 0:
                        probe.append(tf.value)
                if probe:
                    bare = float(np.median(probe))
                    line["roofline"]["box_bare_mfma_tflops"] = bare
                    line["roofline"]["executed_over_box_bare"] = line["roofline"]["executed_tflops"] / bare
                    line["roofline"]["box_note"] = ("bare v_mfma_f32_16x16x32_f16 loop on this GPU in this run: the executed rate of "
                                                    "k_svm_screen (MFMA + one v_exp_f32 and one fma per evaluation x SV + LDS/DMA "
                                                    "traffic) against what the matrix pipe alone sustains here")
            except Exception as ex:      # noqa: BLE001 -- context only
                line["roofline"]["box_bare_mfma_tflops"] = None
                line["roofline"]["box_note"] = "probe unavailable: %r" % (ex,)
        if world == 1 and args.full and not args.no_f32_side:
            for other in [m for m in ("f16x3", "f32") if m != args.precision]:
                e2 = make_engine(other)
                r2 = run(e2, 2, 1, False)
                e2.close()
                line[other + "_mode"] = {"value": r2["evals"] / r2["elapsed"], "ms_per_step": 1e3 * r2["elapsed"] / 2,
                                         "roofline": roofline(r2, other, model_key="seed%d" % med["seed"]), "stage_ms_per_step": r2["stage_ms"],
                                         "same_best": bool(r2["out"]["eval"] == res["out"]["eval"] and
                                                           r2["out"]["best_row"] == res["out"]["best_row"] and
                                                           r2["out"]["best_col"] == res["out"]["best_col"] and
                                                           r2["out"]["best_roll"] == res["out"]["best_roll"])}
        if world == 1 and args.full and not args.no_f32_side and args.precision == "f16s":
            # Two requests in flight on the one GPU (two engines, each its own stream and device state, one host thread each) against
            # one engine serving the same requests one after the other: a request's tail -- the tiers behind the sweep, pre-stages,
            # vote: ~1.4 ms of short lists and small launches -- leaves most of the chip idle, the other request's kernels fill it.
            # A SERVING figure next to the headline (which stays one request at a time), never the headline itself.
            try:
                import threading
                pair = [make_engine("f16s"), make_engine("f16s")]
                n_req = max(4, args.steps)

                def serve(e_, n_, acc_):
                    ev_ = 0
                    for _ in range(n_):
                        rec_ = e_.score_rolls([cloud], [inp], 0, args.rolls)[0]
                        ev_ += int(rec_["n_evals"].sum())
                    acc_.append((ev_, e_.finalize(inp, rec_)))
                for e_ in pair:
                    serve(e_, 2, [])
                fence()
                acc1 = []
                t0 = time.perf_counter()
                serve(pair[0], 2 * n_req, acc1)
                fence()
                t_seq = time.perf_counter() - t0
                acc2 = []
                ths = [threading.Thread(target=serve, args=(e_, n_req, acc2)) for e_ in pair]
                t0 = time.perf_counter()
                for t_ in ths:
                    t_.start()
                for t_ in ths:
                    t_.join()
                fence()
                t_par = time.perf_counter() - t0
                for e_ in pair:
                    e_.close()
                v_seq, v_par = acc1[0][0] / t_seq, sum(q[0] for q in acc2) / t_par
                line["two_requests_in_flight"] = {
                    "value": v_par, "ms_per_request": 1e3 * t_par / (2 * n_req), "one_at_a_time": v_seq,
                    "ms_per_request_one_at_a_time": 1e3 * t_seq / (2 * n_req), "ratio": v_par / v_seq, "requests": 2 * n_req,
                    "same_best": bool(all(q[1]["best_vote"] == acc1[0][1]["best_vote"] and q[1]["best_roll"] == acc1[0][1]["best_roll"] for q in acc2)),
                    "note": "two engines on this GPU, one host thread each, the same cloud and model as the headline (median seed): "
                            "throughput of a server that keeps two requests in flight; the headline is one request at a time"}
            except Exception as ex:      # noqa: BLE001 -- a side measurement must never cost the main line
                line["two_requests_in_flight"] = {"value": None, "note": "unavailable: %r" % (ex,)}
        if world == 1 and args.full and not args.no_hard_side and args.precision == "f16s":
            # The headline model is benign (seeded random coefficients: decisions spread wide against sum|coef|K).  The only
            # genuinely libsvm-trained model in the repo (tests/golden/surrogate.model, svm-train -c 512: most coefficients at
            # the bound, decisions crowding around zero) is the hard case: replicated to bench size it shows what an
            # ill-conditioned model costs.  The engine finds out by itself (first call) and switches the screening kernel to
            # the variant that measures |w|_2 = sqrt(sum (coef K)^2).
            hard_path = os.path.join(tmp, "hard.model")
            models.write_replicated_model(hard_path, os.path.join(ROOT, "tests", "golden", "surrogate.model"), copies=24, jitter=0.01, seed=5)
            eh = make_engine("f16s", hard_path)
            nsv_h = eh.model_info()["n_sv"]
            form_h = eh.screen_form()
            rh = run(eh, 3, 2, False)
            eh.close()
            e3 = make_engine("f16x3", hard_path)
            r3 = run(e3, 1, 1, False)
            e3.close()
            line["hard_model"] = {"model": "tests/golden/surrogate.model (libsvm-3.12 svm-train -c 512 -g 0.0031 on real feature rows) x 24 "
                                           "jittered copies: nSV=%d" % nsv_h,
                                  "value": rh["evals"] / rh["elapsed"], "unit": "evals/s", "ms_per_step": 1e3 * rh["elapsed"] / 3,
                                  "roofline": roofline(rh, "f16s", nsv_h, model_key="hard"), "stage_ms_per_step": rh["stage_ms"],
                                  "refined_share": rh["refined"] / max(1.0, rh["evals"] / 3), "screening_form": form_h,
                                  "f16x3_ms_per_step": 1e3 * r3["elapsed"],
                                  "same_best_as_f16x3": bool(all(r3["out"][k] == rh["out"][k] for k in ("eval", "best_row", "best_col", "best_roll")))}
        if world == 1 and args.full and not args.no_trained_side and args.precision == "f16s":
            # The one question the headline cannot answer: a genuinely trained model of "full SV set" size.  The reference's
            # own model is missing from its checkout; this one was trained by the reference's svm-train the way easy.py does it
            # (tools/make_trained_model.py: 24000 feature rows harvested from every data/*.pcd, 7 % label noise, cross-validated
            # C = 2048, gamma = 2^-13): 8964 SVs, most coefficients at the bound, decisions ~1e-7 of sum|coef|K -- nothing an fp32
            # coefficient sum can decide.  The engine serves it with the centred-remainder form of the screening pass.
            tr_path = os.path.join(tmp, "trained.model")
            models.unpack_trained_model(os.path.join(ROOT, "tests", "golden", "trained.model.npz"), tr_path)
            with open(os.path.join(ROOT, "tests", "golden", "trained_model.json")) as f:
                tr_meta = json.load(f)
            et = make_engine("f16s", tr_path)
            nsv_t = et.model_info()["n_sv"]
            form = et.screen_form()
            rt = run(et, 3, 2, False)
            et.close()
            e3 = make_engine("f16x3", tr_path)
            r3 = run(e3, 1, 1, False)
            e3.close()
            rl = roofline(rt, "f16s", nsv_t, model_key="trained")
            line["trained_model"] = {
                "model": "tests/golden/trained.model.npz: libsvm-3.12 C-SVC/RBF trained by the REFERENCE svm-train (oracle/_ref) on %d feature rows "
                         "harvested from all data/*.pcd x 12 rolls (label rule + %.1f %% seeded flips), C = %g and gamma = %g from a %d-fold "
                         "cross-validation grid on %d rows (accuracy %.1f %%): nSV = %d" %
                         (tr_meta["rows"], 100 * tr_meta["flip_share"], tr_meta["C"], tr_meta["gamma"], tr_meta["folds"], tr_meta["grid_rows"],
                          tr_meta["cv_accuracy"], nsv_t),
                "value": rt["evals"] / rt["elapsed"], "unit": "evals/s", "ms_per_step": 1e3 * rt["elapsed"] / 3, "n_sv": nsv_t,
                "screening_form": form, "roofline": rl, "stage_ms_per_step": rt["stage_ms"],
                "end_to_end_frac_of_fp16_peak": rl["flop_per_launch"] / (rt["elapsed"] / 3) / 1e12 / PEAK_F16_MFMA_TFLOPS,
                "value_at_4096_sv_equivalent": rt["evals"] / rt["elapsed"] * nsv_t / 4096.0,
                "refined_share": rt["refined"] / max(1.0, rt["evals"] / 3),
                "tiers_per_step": {"three_pass_tier": rt["refined"], "exact_integer_tier": rt["exact_integer"], "fp64_mfma_tier": rt["fp64"],
                                   "strict_order_tier": rt["strict"]},
                "f16x3_ms_per_step": 1e3 * r3["elapsed"],
                "same_best_as_f16x3": bool(all(r3["out"][k] == rt["out"][k] for k in ("eval", "best_row", "best_col", "best_roll"))),
                "best": {"eval": rt["out"]["eval"], "row": rt["out"]["best_row"], "col": rt["out"]["best_col"], "roll": rt["out"]["best_roll"]},
                "note": "2.19 x the support vectors of the headline model: `value` x n_sv / 4096 is the rate at equal contraction work"}
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(feat, rng_file, model_path, xyz, args)
        else:
            line["cpu_baseline"] = None
        if world == 1 and args.full and not args.no_latency:
            tr_lat = None
            if not args.no_trained_side:
                tr_lat = os.path.join(tmp, "trained.model")
                if not os.path.exists(tr_lat):
                    models.unpack_trained_model(os.path.join(ROOT, "tests", "golden", "trained.model.npz"), tr_lat)
            line["grasp_latency"] = latency_small(feat, rng_file, local_rank,
                                               {"f32": capi.FLAG_FP32_MFMA, "f16x3": capi.FLAG_SPLIT_F16, "f16s": 0}[args.precision], tr_lat,
                                               model_path if args.nsv >= 1024 else None)
        line["ranks"] = ranks_block(world, med["per_rank"], args.shard, use_dist, dist,
                                    ".".join(str(v) for v in torch.cuda.nccl.version()) if use_dist else None,
                                    fallback=(1e3 * elapsed / args.steps, res["svm_s"] * 1e3))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        if args.full and not args.no_cabi_side:
            # every rank has let go of its engine; give the other rank processes a moment to exit, then measure the C++-host
            # path (one process driving all the GPUs through the C-ABI) in a child of its own
            del d_xyz
            torch.cuda.empty_cache()
            if world > 1:
                time.sleep(3.0)
            side = run_cabi_side(args, world, med["seed"])
            if "best" in side:
                side["same_best_as_rank0"] = bool(side["best"] == line["best"])
            line["c_abi_sharded"] = side
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
