"""haf_check_space_ref (include/hafgrasp.h; csrc/space_rules.h, csrc/space_host.cpp) against the independent mirror of space_cases.py: no
GPU.  The device call is held to haf_check_space_ref by tests/test_space_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import clearance_cases as cc
import space_cases as sc
from haf_grasping_amd import capi

CASES = sc.cases()
MIRROR = {}


def mirror_of(case):
    """computed once per case, shared and never changed"""
    if case["name"] not in MIRROR:
        MIRROR[case["name"]] = sc.mirror(case)
    return MIRROR[case["name"]]


def test_exports_and_defaults():
    L = capi.lib()
    assert L.haf_abi_version() == 2
    for name in ("haf_space_default", "haf_check_space_ref", "haf_check_space"):
        assert hasattr(L, name)
    p = capi.space_params()
    F = np.float32
    assert (F(p.sample_step), F(p.near_m), F(p.tol_abs), F(p.tol_rel)) == (F(0.004), F(0.05), F(0.004), F(0.002))
    assert (p.max_hit, p.max_unknown, p.min_between_hit) == (0, 0, 1)
    assert (capi.MAX_SPACE_VIEWS, capi.MAX_SPACE_SAMPLES) == (8, 65536)
    L.haf_space_default(None)                             # a null pointer is ignored
    # the default lattice: 20 x 5 x 15, 2 x 5 x 15 twice, 30 x 10 x 10
    rows, order, info = capi.check_space_ref(sc.scene_view("u16", 8, 6, sc.IDENTITY, np.random.default_rng(1))[0], [sc.EXACT_GRASP])
    assert info == dict(step=cc.W(np.float32(0.004)), n=[[20, 5, 15], [2, 5, 15], [2, 5, 15], [30, 10, 10]], n_samples=4800)


def test_case_names_are_unique():
    assert len({c["name"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_ref_equals_mirror(case):
    want = mirror_of(case)
    sc.same(sc.run(capi.check_space_ref, case), want, case["name"])
    got = sc.run(capi.check_space_ref, case, states=False)      # without states: the same rows
    assert len(got) == 3 and got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() and got[2] == want[2]


def test_the_cases_cover_what_they_claim():
    """a weakened case list fails here, not silently"""
    seen = np.zeros((4, 4), np.int64)
    deltas, merges = {}, set()
    for case in CASES:
        rows, order, info, states = mirror_of(case)
        seen += rows["n"].sum(axis=0)
        for g, j, state in case["expect"]:
            assert states[g, j] == state, (case["name"], g, j, state, states[g, j])
        merges |= set(case["merges"])
    assert (seen > 0).all(), seen                         # every state in every region
    for dt in (np.uint16, np.float32):
        for rel in (0.0, 0.002):
            case, expect = sc.boundary_case(dt, rel)
            states = mirror_of(case)[3]
            lat = sc.mirror_lattice(capi.gripper(**case["gripper"]), capi.space_params(**case["params"]))
            for g, j, state, what in expect:
                assert states[g, j] == state, (case["name"], what)
                deltas.setdefault((case["name"], int(lat["region"][j])), set()).add(what)
    assert len(deltas) == 16 and all(v == set(sc.DELTAS) for v in deltas.values()), deltas      # every delta in every region, kind and tol_rel
    assert merges == set(sc.MERGE_RULES)
    case = next(c for c in CASES if c["name"] == "merge_two_views")
    single = [sc.mirror_space([v], case["grasps"], capi.gripper(), capi.space_params(**case["params"]))[3] for v in case["views"]]
    decided = set()
    for g, j, state in case["expect"]:                    # the two views disagree there, and the higher rank wins
        pair = tuple(sorted((int(single[0][g, j]), int(single[1][g, j])), reverse=True))
        assert pair[0] == state and pair[1] < state
        decided.add(pair)
    assert decided == set(sc.MERGE_RULES.values())
    for field, yes, no in sc.threshold_cases():           # each threshold decides clear alone
        assert mirror_of(yes)[0]["clear"].tolist() == [1] and mirror_of(no)[0]["clear"].tolist() == [0], field
    voids = mirror_of(next(c for c in CASES if c["name"] == "voids_amid_valid"))
    assert sorted(set(voids[0]["clear"].tolist())) == [-1, 1] and not voids[0]["n"][voids[0]["clear"] == -1].any()
    assert {c["params"].get("tol_rel", None) for c in CASES if c["name"].startswith("boundary")} == {0.0, 0.002}
    sizes = {mirror_of(c)[2]["n_samples"] for c in CASES}
    assert {1, 63, 64, 65, sc.CHUNK - 1, sc.CHUNK, sc.CHUNK + 1, capi.MAX_SPACE_SAMPLES} <= sizes


def test_occluded_finger():
    """where haf_check_grasps counts no point and reports a free gripper, one view cannot vouch for the finger behind the box; the view
    from the other side can"""
    front, back, grasp = sc.occluded_scene()
    free = capi.check_grasps_ref(front[0], [grasp])[0]
    assert free["free"].tolist() == [1] and free["n_finger"].tolist() == [[0, 0]]
    rows, order, info = capi.check_space_ref([front[0]], [grasp])
    assert rows["n"][0][sc.FINGER0][sc.HIDDEN] > 0 and rows["clear"].tolist() == [0] and order.tolist() == []
    assert rows["n"][0][sc.FINGER1][sc.HIDDEN] == 0 and rows["n"][0][sc.BETWEEN][sc.HIT] > 0
    rows, order, info = capi.check_space_ref([front[0], back[0]], [grasp])
    assert rows["n"][0][:, sc.HIDDEN][1:].sum() == 0 and rows["clear"].tolist() == [1] and order.tolist() == [0]
    sc.same(capi.check_space_ref([front[0], back[0]], [grasp], states=True), sc.mirror_space([front, back], [grasp], capi.gripper(), capi.space_params()))


def test_space_paths_under_address_and_ub_sanitizers(tmp_path):
    """CPU sanitizer job of the call's host units: space_host.cpp and the units it calls, built with -fsanitize=address,undefined and
    driven by tests/sanitize/space_paths.cpp, a program of its own, over exactly sized heap blocks.  Any report fails."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    if clang is None:
        pytest.skip("no host C++ compiler with sanitizers")
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    csrc = os.path.join(root, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "space_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-ffp-contract=off"]
    units = ["space_host.cpp", "clearance_host.cpp", "transfer_host.cpp", "frames_host.cpp", "frame_stage.cpp", "parsers.cpp"]
    cmd = [clang] + flags + [os.path.join(csrc, u) for u in units] + [os.path.join(root, "tests", "sanitize", "space_paths.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "space sanitizer job ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        (p.returncode, p.stdout[-500:], p.stderr[-3000:])


def test_cli_check_space_forms_parse(tmp_path):
    """--check-space default|STEP,TOL_ABS,TOL_REL[,MAX_HIT,MAX_UNKNOWN]: a malformed form -- too few fields, four, six, something that
    is no number, something behind the last field -- is a usage error (exit 2) before anything is opened; a well-formed one is not"""
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    base = [cli, "--features", "f", "--range", "r", "--model", "m", "--intrinsics", "525", "525", "319.5", "239.5", "--depth", str(tmp_path / "none.pgm"),
            "--top-k", "4"]

    def rc(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True).returncode
    for form in ("default", "0.004,0.004,0.002", "0.008,0.01,0,3,25"):
        assert rc("--check-space", form) == 1, form       # parsed; then the missing files are the error
        assert rc("--gripper", "default", "--check-space", form) == 1, form
    for form in ("", "0.004", "0.004,0.004", "0.004,0.004,0.002,1", "0.004,0.004,0.002,1,5,6", "0.004,0.004,abc", "0.004,0.004,0.002x",
                 "0.004,0.004,0.002,1,x", "0.004,0.004,0.002,1,5x", "0.004,0.004,0.002,", "defaults"):
        assert rc("--check-space", form) == 2, form
    assert rc("--check-space") == 2                       # no argument


def raw_call(views, grasps, grip=None, params=None, n_views=None, n_grasps=None, stride=None, null=(), states=False):
    """haf_check_space_ref with every output pre-filled -> (rc, whether an output byte changed)"""
    arr, n, st = capi._grasp_array(grasps)
    frames = (capi.Frame * max(1, len(views)))(*views)
    grip = capi.gripper() if grip is None else grip
    params = capi.space_params() if params is None else params
    out, order = np.full(max(1, n), 0x5A, np.uint8).repeat(capi.SPACE_DTYPE.itemsize), np.full(max(1, n), 0x5A5A5A5A, np.int32)
    nc, info, sts = C.c_int32(0x5A5A5A5A), (C.c_int32 * 16)(*[0x5A5A5A5A] * 16), np.full(1 << 22, 0x5A, np.uint8)
    args = dict(views=frames, gripper=C.byref(grip), params=C.byref(params), grasps=arr, out=out.ctypes.data)
    for k in null:
        args[k] = None
    rc = capi.lib().haf_check_space_ref(args["views"], len(views) if n_views is None else n_views, args["gripper"], args["params"],
                                        n if n_grasps is None else n_grasps, args["grasps"], st if stride is None else stride, args["out"],
                                        order.ctypes.data, C.byref(nc), C.cast(info, C.POINTER(capi.SpaceInfo)), sts.ctypes.data if states else None)
    changed = (out != 0x5A).any() or (order != 0x5A5A5A5A).any() or nc.value != 0x5A5A5A5A or any(x != 0x5A5A5A5A for x in info) or (sts != 0x5A).any()
    return rc, bool(changed)


def test_refusals_write_nothing():
    rng = np.random.default_rng(3)
    view = sc.scene_view("u16", 8, 6, sc.IDENTITY, rng)[0]
    g = [sc.EXACT_GRASP]
    assert raw_call([view], g) == (capi.HAF_OK, True)
    ARG, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    xyz = capi.xyz_frame(np.zeros((6, 8, 3), np.float32))
    singular = sc.scene_view("u16", 8, 6, np.zeros((3, 4), np.float32), rng)[0]
    device = capi.depth_frame(4096, 100.0, 100.0, 4.0, 3.0, width=8, height=6, dtype=np.uint16)
    wide = capi.depth_frame(4096, 100.0, 100.0, 4.0, 3.0, width=40000, height=1, dtype=np.uint16)     # (a camera of more than 32768 pixels a side)
    refused = [
        (dict(null=("views", )), ARG), (dict(null=("gripper", )), ARG), (dict(null=("params", )), ARG), (dict(null=("grasps", )), ARG),
        (dict(null=("out", )), ARG),
        (dict(n_views=0), ARG), (dict(n_views=9), ARG), (dict(n_grasps=0), ARG), (dict(n_grasps=capi.MAX_CHECK_GRASPS + 1), ARG),
        (dict(stride=C.sizeof(capi.GraspOutput) - 8), ARG), (dict(stride=C.sizeof(capi.GraspOutput) + 4), ARG),
        (dict(grip=capi.gripper(opening=0.0)), ARG), (dict(grip=capi.gripper(palm_width=float("nan"))), ARG), (dict(grip=capi.gripper(finger_length=1.5)), ARG),
        (dict(params=capi.space_params(sample_step=0.0004)), ARG), (dict(params=capi.space_params(sample_step=1.5)), ARG),
        (dict(params=capi.space_params(sample_step=float("nan"))), ARG), (dict(params=capi.space_params(near_m=0.0005)), ARG),
        (dict(params=capi.space_params(near_m=17.0)), ARG), (dict(params=capi.space_params(tol_abs=-1.0)), ARG),
        (dict(params=capi.space_params(tol_abs=float("inf"))), ARG), (dict(params=capi.space_params(tol_rel=1.5)), ARG),
        (dict(params=capi.space_params(tol_rel=-0.1)), ARG),
        (dict(grip=capi.gripper(**sc.OVER_CAP), params=capi.space_params(sample_step=sc.STEP)), ARG),      # N = 65537
        (dict(grip=capi.gripper(**sc.between_only(64, 32, 32)), params=capi.space_params(sample_step=sc.STEP), states=True,
              grasps=[sc.EXACT_GRASP] * 65), CAP),                                                           # 65 x 65536 state bytes > 2^22
    ]
    for kw, code in refused:
        grasps = kw.pop("grasps", g)
        assert raw_call([view], grasps, **kw) == (code, False), kw
    for bad in (xyz, singular, device, wide, capi.depth_frame(np.zeros((6, 8), np.uint16), 0.0, 100.0, 4.0, 3.0),
                capi.depth_frame(np.zeros((6, 8), np.uint16), 100.0, 100.0, 40000.0, 3.0),
                capi.depth_frame(np.zeros((6, 8), np.uint16), 100.0, 100.0, 4.0, 3.0, depth_scale=0.0)):
        assert raw_call([view, bad], g) == (ARG, False)
        assert raw_call([bad], g) == (ARG, False)
    # the cap itself is taken, with states for as many grasps as 2^22 bytes hold
    rc, changed = raw_call([view], [sc.EXACT_GRASP] * 64, grip=capi.gripper(**sc.between_only(64, 32, 32)), params=capi.space_params(sample_step=sc.STEP),
                           states=True)
    assert (rc, changed) == (capi.HAF_OK, True)
    with pytest.raises(capi.HafError):
        capi.check_space_ref([xyz], g)
