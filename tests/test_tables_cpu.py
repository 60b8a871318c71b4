"""The model tables without a GPU: the device-free builder (csrc/model_tables.cpp, through haf_test_host_table_digest) must give, for
every engine of tests/table_cases.py, the digests that tests/golden/table_digests.json recorded ON THE DEVICE from the commit before
the table work was split -- host images under the device tables' names, every member of every parameter struct, the scalars and
flags.  Plus every refusal of the builder with its code and text, sigma_upper_bound behind its hook, and the builder under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

import models
import table_cases
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return table_cases.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("table_models")


@pytest.mark.parametrize("name", sorted(table_cases.CASES))
def test_host_tables_match_recorded_device_digests(name, fixture, data_dir, golden_dir, model_dir):
    """exp2, exp and log enter several constants, so the digests hold for the C library they were recorded with: another one skips"""
    if list(platform.libc_ver()) != fixture["libc"]:
        pytest.skip("the digests were recorded with C library %r, this is %r" % (fixture["libc"], list(platform.libc_ver())))
    want = fixture["cases"][name]
    got = table_cases.host_digests(name, data_dir, golden_dir, model_dir)
    assert sorted(got) == sorted(want)
    moved = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not moved, moved


# ---- the refusals: the smallest input that meets each, its code and its text as they were before the split ----
ONE_ROW = "0\t%d\t0\t1" + "\t0" * 12 + "\t1\t0\t0\t0\n"           # one region x1 = 0, x2 = %d, y1 = 0, y2 = 1 of weight 1


def _write(path, text):
    with open(str(path), "w") as fh:
        fh.write(text)
    return str(path)


def _tiny_model(path, body="1 1:0.5\n-1 1:-0.5\n", label="1 -1", extra=""):
    return _write(path, "svm_type c_svc\nkernel_type rbf\ngamma 1\nnr_class 2\ntotal_sv 2\nrho 0.1\nlabel %s\n%snr_sv 1 1\nSV\n%s" % (label, extra, body))


def _refused(*a, **kw):
    with table_cases.case_env({}):
        rc, got, msg = table_cases.host_build(*a, **kw)
    return rc, msg


def test_refusals_keep_code_and_text(tmp_path, data_dir, golden_dir):
    feat, rng = table_cases.files(data_dir)
    surrogate = os.path.join(golden_dir, "surrogate.model")
    one_ok = _write(tmp_path / "one.txt", ONE_ROW % 13)
    rng1 = _write(tmp_path / "r1", "x\n-1 1\n1 0 1\n")
    tiny = _tiny_model(tmp_path / "tiny.model")
    assert _refused(one_ok, rng1, tiny)[0] == 0                                   # the small inputs themselves are served

    # more than 324 rows
    many = _write(tmp_path / "many.txt", (ONE_ROW % 13) * 325)
    assert _refused(many, rng1, tiny) == (capi.HAF_E_ARG, "feature file has more than 324 rows; this build's contraction kernel is sized for 324 attributes")
    # a region outside the window: one row with x2 = 14
    wide = _write(tmp_path / "wide.txt", ONE_ROW % 14)
    assert _refused(wide, rng1, tiny) == (capi.HAF_E_IO, "feature region outside the 14x14 window in " + wide)
    # a range file lacking one non-constant attribute
    two = _write(tmp_path / "two.txt", (ONE_ROW % 13) + (ONE_ROW % 12))
    assert _refused(two, rng1, tiny) == (capi.HAF_E_ARG, "attribute 2 is missing from the range file and is not constant; per-file ranges are not supported")
    # support vectors too large: one component of 1e5 (gamma 1: c = 1.7, beyond the fp16 operands' 60000)
    big = _tiny_model(tmp_path / "big.model", body="1 1:100000\n-1 1:-0.5\n")
    assert _refused(feat, rng, big) == (capi.HAF_E_ARG, "support vectors too large for the fp16 screening pass; use HAF_FLAG_SPLIT_F16")
    assert _refused(feat, rng, big, flags=capi.FLAG_SPLIT_F16)[0] == 0            # ... as the text says
    # probability without probA / probB
    assert _refused(feat, rng, surrogate, flags=capi.FLAG_PROBABILITY) == \
        (capi.HAF_E_ARG, "HAF_FLAG_PROBABILITY needs a model with probA and probB (svm-train -b 1)")


def test_label_200_is_served_as_before(tmp_path, data_dir):
    """`label 200 1`: the grid value of a label is atoi of the first TWO characters of its "%g" text (label_grid_value: what the
    reference's show_predicted_gps reads), here 20.  No label text reaches the refusal "model labels out of range" (|value| <= 99 <
    127): the builder keeps that check with its code and text, and like the code before the split it serves this model."""
    feat, rng = table_cases.files(data_dir)
    m200 = _tiny_model(tmp_path / "l200.model", label="200 1")
    assert _refused(feat, rng, m200) == (0, "")


def test_sigma_upper_bound_is_served_unchanged():
    L = capi.testlib()
    one = np.array([[3.0]])
    # one entry: every squaring after the first normalisation is 1 x 1 = 1, so the bound is sqrt(exp(log 9)) (1 + 1e-9) in the C library's functions
    assert L.haf_test_sigma_upper(one.ctypes.data, 1, 1) == math.sqrt(math.exp(math.log(9.0) + math.log(1.0) / 128.0)) * (1.0 + 1e-9)
    assert L.haf_test_sigma_upper(np.zeros((3, 4)).ctypes.data, 3, 4) == 0.0
    rng = np.random.RandomState(3)
    M = np.ascontiguousarray(rng.uniform(-1, 1, size=(37, 19)))
    got, want = L.haf_test_sigma_upper(M.ctypes.data, 37, 19), np.linalg.svd(M, compute_uv=False)[0]
    assert want <= got <= want * 19 ** (1.0 / 128.0) * (1 + 1e-6)


def test_table_paths_under_address_and_ub_sanitizers(tmp_path, data_dir, golden_dir, model_dir):
    """CPU sanitizer job of the table builder: model_tables.cpp + parsers.cpp built with -fsanitize=address,undefined and driven by
    tests/sanitize/table_paths.cpp, a program of its own, over cases a, b, g and h of tests/table_cases.py (every stage: screening slots,
    the centred-remainder and low-rank tables, tier 1, the int8 planes, ragged tiles, sparse rows, a model narrower than the feature
    file) and the refusal inputs.  Any report fails."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    if clang is None:
        pytest.skip("no host C++ compiler with sanitizers")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    csrc = os.path.join(ROOT, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "table_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc]
    cmd = [clang] + flags + [os.path.join(csrc, "model_tables.cpp"), os.path.join(csrc, "parsers.cpp"),
                             os.path.join(ROOT, "tests", "sanitize", "table_paths.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    feat, rng = table_cases.files(data_dir)
    lines = []
    for name in "abgh":
        kind, flags_, grid, extra = table_cases.CASES[name]
        assert not extra
        lines.append((feat, rng, table_cases.model_path(kind, golden_dir, model_dir), flags_, grid, 0))
    rng1 = _write(tmp_path / "r1", "x\n-1 1\n1 0 1\n")
    tiny = _tiny_model(tmp_path / "tiny.model")
    lines += [(_write(tmp_path / "many.txt", (ONE_ROW % 13) * 325), rng1, tiny, 0, 56, capi.HAF_E_ARG),
              (_write(tmp_path / "wide.txt", ONE_ROW % 14), rng1, tiny, 0, 56, capi.HAF_E_IO),
              (_write(tmp_path / "two.txt", (ONE_ROW % 13) + (ONE_ROW % 12)), rng1, tiny, 0, 56, capi.HAF_E_ARG),
              (feat, rng, _tiny_model(tmp_path / "big.model", body="1 1:100000\n-1 1:-0.5\n"), 0, 56, capi.HAF_E_ARG),
              (feat, rng, os.path.join(golden_dir, "surrogate.model"), capi.FLAG_PROBABILITY, 56, capi.HAF_E_ARG),
              (feat, rng, _tiny_model(tmp_path / "l200.model", label="200 1"), 0, 56, 0)]
    manifest = _write(tmp_path / "manifest", "".join(" ".join(str(x) for x in ln) + "\n" for ln in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, manifest], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "table sanitizer job ok (10 cases)" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
