"""CPU test of the sensor-frame staging code that needs no device (csrc/frame_stage.h): the host sanitizer job of pack_rows, unpack_rows,
stage_rows, describe_frame, staged_bytes, describe_image, describe_output and check_frame_batch.  The wiring into the engine needs a GPU: tests/test_frame_stage_gpu.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

import frame_cases as fc
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_paths_under_address_and_ub_sanitizers(tmp_path):
    """frame_stage.cpp + frames_host.cpp + parsers.cpp built with -fsanitize=address,undefined by the ROCm clang and driven by
    tests/sanitize/stage_paths.cpp as a program of its own: every kind, width 1 / 3 / 61 / 64, height 1 / 5, padded rows, point strides
    12 / 16 / 20 and masks against a byte-by-byte loop in exactly sized heap blocks; unpack_rows of 1 / 2 / 4-byte elements into padded
    targets whose last row ends at its last element and whose bytes between the rows must stay; the pieces of frames around 256 KB against
    the upload loop the code replaced; the descriptors of frames, side images and output images; the batch checks over every refusal of frame_cases.refusal_frames().  Any report fails."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    if clang is None:
        pytest.skip("no host C++ compiler with sanitizers")
    refusals = fc.refusal_frames()
    assert len(refusals) >= 60
    path = tmp_path / "refusal_frames.bin"
    with open(path, "wb") as f:
        for _, frame, code, arr in refusals:
            data = 0 if not frame.data else 2 if frame.data == arr.ctypes.data + 1 else 1
            assert data != 1 or frame.data == arr.ctypes.data
            f.write(struct.pack("=ii", code, data) + bytes(frame))
    assert os.path.getsize(path) == len(refusals) * (8 + C.sizeof(capi.Frame))
    csrc = os.path.join(ROOT, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "stage_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-ffp-contract=off"]
    cmd = [clang] + flags + [os.path.join(csrc, "frame_stage.cpp"), os.path.join(csrc, "frames_host.cpp"), os.path.join(csrc, "parsers.cpp"),
                             os.path.join(ROOT, "tests", "sanitize", "stage_paths.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "stage sanitizer job ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        (p.returncode, p.stdout[-500:], p.stderr[-3000:])
