"""CPU tests of the sensor-frame entry points that need no engine (include/hafgrasp.h: haf_frame): struct layout, exports, defaults,
haf_frame_points against an independent numpy-fp32 mirror word for word, the refusals, the 16-bit PGM reader and the host sanitizer
job.  haf_score_frames and the device kernel need a GPU: tests/test_frames_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_cases as fc
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["data", "kind", "width", "height", "on_device", "row_stride_bytes", "point_stride_bytes", "fx", "fy", "cx", "cy", "depth_scale",
          "min_depth", "max_depth", "sensor_to_base"]
NEW_NAMES = {"haf_frame_default", "haf_frame_points", "haf_score_frames", "haf_debug_fetch_points", "haf_pgm16_load"}


def test_frame_struct_layout_matches_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hafgrasp.h"\nint main(void) {\n printf("%zu", sizeof(haf_frame));\n' +
                   "".join(' printf(" %%zu", offsetof(haf_frame, %s));\n' % f for f in FIELDS) +
                   ' printf(" %d %d %d\\n", HAF_FRAME_DEPTH_U16, HAF_FRAME_DEPTH_F32, HAF_FRAME_XYZ_F32);\n return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    want = [C.sizeof(capi.Frame)] + [capi.Frame.__dict__[f].offset for f in FIELDS] + \
           [capi.FRAME_DEPTH_U16, capi.FRAME_DEPTH_F32, capi.FRAME_XYZ_F32]
    assert got == want
    assert C.sizeof(capi.Frame) == 120 and capi.Frame.sensor_to_base.offset == 68      # (LP64)


def test_frame_names_exported_by_both_libraries():
    with open(os.path.join(ROOT, "include", "hafgrasp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert NEW_NAMES <= set(re.findall(r"\b(haf_[a-z_0-9]+)\s*\(", text))
    assert "#define HAF_ABI_VERSION 2" in text
    for L in (capi.lib(), capi.testlib()):
        for name in NEW_NAMES:
            assert hasattr(L, name), name
        assert L.haf_abi_version() == 2


def test_frame_default():
    f = capi.Frame()
    C.memset(C.byref(f), 0xFF, C.sizeof(f))
    capi.lib().haf_frame_default(C.byref(f))
    assert f.data is None and (f.kind, f.width, f.height, f.on_device, f.row_stride_bytes, f.point_stride_bytes) == (0, 0, 0, 0, 0, 0)
    assert (f.fx, f.fy, f.cx, f.cy, f.min_depth, f.max_depth) == (0, 0, 0, 0, 0, 0)
    assert np.float32(f.depth_scale) == np.float32(0.001)
    assert list(f.sensor_to_base) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert bytes(f)[capi.Frame.sensor_to_base.offset + 48:] == b"\0" * (C.sizeof(f) - capi.Frame.sensor_to_base.offset - 48)   # padding too
    with pytest.raises(TypeError):
        capi.default_frame(focal=1.0)


CASES = fc.cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_frame_points_equal_numpy_mirror_word_for_word(name):
    _, frame, image = next(c for c in CASES if c[0] == name)
    got = fc.words(capi.frame_points(frame))
    want = fc.mirror_points(frame, image)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])
    nan = np.isnan(got.view(np.float32))
    assert (got[nan] == fc.NAN_WORD).all()                 # one NaN pattern only
    if frame.width * frame.height > 64:
        assert 0.2 < (~nan.any(axis=1)).mean() < 0.95      # the comparison is not one of NaN with NaN


def test_frame_points_special_values_one_by_one():
    """what the header says of each special input, spelt out (the mirror above would agree with a shared misreading)"""
    def one(value, **kw):
        img = np.array([[value]], dtype=kw.pop("dtype", np.float32))
        kw.setdefault("depth_scale", 1.0)
        p = capi.frame_points(capi.depth_frame(img, 500.0, 500.0, 0.0, 0.0, **kw))
        return fc.words(p)[0], p[0]
    inv = [fc.NAN_WORD] * 3
    for v in (np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0):
        assert list(one(v)[0]) == inv, v
    sub = np.float32(1e-41)
    assert one(sub)[1][2] == sub                           # a subnormal depth is a depth
    lo, hi = np.float32(0.5), np.float32(2.5)
    up, down = np.float32(np.inf), np.float32(0)
    for d in (lo, np.nextafter(lo, up), np.nextafter(hi, down), hi):              # on a limit and one ulp inside: valid
        assert one(d, min_depth=lo, max_depth=hi)[1][2] == d
    for d in (np.nextafter(lo, down), np.nextafter(hi, up)):                      # one ulp outside: invalid
        assert list(one(d, min_depth=lo, max_depth=hi)[0]) == inv
    assert one(np.nextafter(lo, down), max_depth=hi)[1][2] < lo                   # 0 = no limit on that side
    assert one(np.nextafter(hi, up), min_depth=lo)[1][2] > hi
    assert list(one(0, dtype=np.uint16)[0]) == inv
    assert one(1, dtype=np.uint16, depth_scale=0.001)[1][2] == np.float32(1) * np.float32(0.001)
    assert one(65535, dtype=np.uint16, depth_scale=0.001)[1][2] == np.float32(65535) * np.float32(0.001)
    assert list(one(65535, dtype=np.uint16, depth_scale=0.001, max_depth=60.0)[0]) == inv
    # pixel (2, 1) of a 3 x 2 frame through a pose: every step by hand
    img = np.full((2, 3), 2000, np.uint16)
    t = np.array([0, -1, 0, 0.5, 1, 0, 0, -0.25, 0, 0, 1, 0.125], np.float32)
    p = capi.frame_points(capi.depth_frame(img, 400.0, 300.0, 1.5, 0.25, sensor_to_base=t))[5]
    z = np.float32(2000) * np.float32(0.001)
    xc = ((np.float32(2) - np.float32(1.5)) * (np.float32(1) / np.float32(400))) * z
    yc = ((np.float32(1) - np.float32(0.25)) * (np.float32(1) / np.float32(300))) * z
    assert list(p) == [np.float32(-1) * yc + np.float32(0.5), xc + np.float32(-0.25), z + np.float32(0.125)]


REFUSALS = fc.refusal_frames()


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_frame_points_refusals(name):
    _, frame, code, _ = next(r for r in REFUSALS if r[0] == name)
    out = np.zeros((16, 3), np.float32)
    assert capi.lib().haf_frame_points(C.byref(frame), out.ctypes.data) == code
    assert not out.any()                                   # refused before anything was written


def test_frame_points_null_arguments_and_device_frames():
    L = capi.lib()
    out = np.zeros((12, 3), np.float32)
    img = np.ones((3, 4), np.uint16)
    f = capi.depth_frame(img, 500.0, 500.0, 2.0, 1.5)
    assert L.haf_frame_points(None, out.ctypes.data) == capi.HAF_E_ARG
    assert L.haf_frame_points(C.byref(f), None) == capi.HAF_E_ARG
    f.on_device = 1                                        # valid for haf_score_frames; this function reads host memory only
    assert L.haf_frame_points(C.byref(f), out.ctypes.data) == capi.HAF_E_ARG
    f.on_device = 0
    assert L.haf_frame_points(C.byref(f), out.ctypes.data) == capi.HAF_OK and np.isfinite(out).all()
    # an XYZ frame ignores intrinsics, scale and limits: garbage there is no refusal
    pts = np.ones((3, 4, 3), np.float32)
    g = capi.xyz_frame(pts)
    g.fx, g.depth_scale, g.min_depth = 0.0, float("nan"), float("inf")
    assert L.haf_frame_points(C.byref(g), out.ctypes.data) == capi.HAF_OK and (out == 1).all()


def test_pgm16_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    for k, (w, h) in enumerate([(1, 1), (7, 3), (640, 480)]):
        img = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        img.reshape(-1)[0] = 0x0A23                        # a sample whose bytes are white space and '#'
        p = str(tmp_path / ("d%d.pgm" % k))
        fc.write_pgm16(p, img, maxval=65535 if k else 256, comment=bool(k % 2))
        got = capi.load_pgm16(p)
        assert got.dtype == np.uint16 and got.shape == (h, w) and (got == img).all()


def hostile_pgms(tmp_path):
    """-> {name: path}: files haf_pgm16_load must refuse with HAF_E_IO and a message"""
    img = np.arange(12, dtype=np.uint16).reshape(3, 4) * 1000
    good = str(tmp_path / "good.pgm")
    head = fc.write_pgm16(good, img, comment=False)
    raw = open(good, "rb").read()
    files = {"truncated_header": raw[:len(head) - 4], "header_only_no_terminator": raw[:len(head) - 1], "magic_only": b"P5",
             "empty": b"", "truncated_body": raw[:-1], "half_body": raw[:len(head) + 12], "over_long": raw + b"\0",
             "junk_magic": b"P6" + raw[2:], "junk_magic_text": b"hello world, this is no image\n",
             "maxval_255": b"P5\n4 3\n255\n" + bytes(12), "maxval_70000": b"P5\n4 3\n70000\n" + raw[len(head):],
             "maxval_0": b"P5\n4 3\n0\n" + raw[len(head):],
             "product_overflows_int32": b"P5\n65536 65536\n65535\n" + bytes(64),
             "product_overflows_int64": b"P5\n999999999 999999999\n65535\n" + bytes(64),
             "digits_without_end": b"P5\n" + b"9" * 40 + b" 3\n65535\n" + bytes(64),
             "width_0": b"P5\n0 3\n65535\n", "negative_width": b"P5\n-4 3\n65535\n" + raw[len(head):],
             "comment_without_end": b"P5\n# never ends", "letters_for_height": b"P5\n4 x\n65535\n" + raw[len(head):]}
    out = {}
    for name, data in files.items():
        p = str(tmp_path / (name + ".pgm"))
        with open(p, "wb") as f:
            f.write(data)
        out[name] = p
    out["missing_file"] = str(tmp_path / "no_such_file.pgm")
    return good, out


def test_pgm16_hostile_files(tmp_path):
    good, bad = hostile_pgms(tmp_path)
    assert capi.load_pgm16(good).shape == (3, 4)
    for name, path in bad.items():
        with pytest.raises(capi.HafError) as ei:
            capi.load_pgm16(path)
        assert ei.value.code == capi.HAF_E_IO, name
        assert len(str(ei.value)) > len("hafgrasp error -2: "), name
    L = capi.lib()
    p, w, h = C.POINTER(C.c_uint16)(), C.c_int32(), C.c_int32()
    assert L.haf_pgm16_load(None, C.byref(p), C.byref(w), C.byref(h), None, 0) == capi.HAF_E_ARG
    assert L.haf_pgm16_load(good.encode(), None, C.byref(w), C.byref(h), None, 0) == capi.HAF_E_ARG
    assert L.haf_pgm16_load(bad["junk_magic"].encode(), C.byref(p), C.byref(w), C.byref(h), None, 0) == capi.HAF_E_IO   # no buffer for the text


def test_frame_paths_under_address_and_ub_sanitizers(tmp_path):
    """CPU sanitizer job of the frame entry points (host only): frames_host.cpp + parsers.cpp built with -fsanitize=address,undefined by
    the ROCm clang and driven by tests/sanitize/frame_paths.cpp over the hostile PGM files above, bit-flipped ones, and frames of every
    kind, stride and refusal into exactly sized heap buffers.  Any report fails."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    if clang is None:
        pytest.skip("no host C++ compiler with sanitizers")
    csrc = os.path.join(ROOT, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "frame_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-ffp-contract=off"]
    cmd = [clang] + flags + [os.path.join(csrc, "frames_host.cpp"), os.path.join(csrc, "parsers.cpp"),
                             os.path.join(ROOT, "tests", "sanitize", "frame_paths.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    scratch = tmp_path / "fuzz"
    scratch.mkdir()
    good, bad = hostile_pgms(scratch)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, good, str(scratch)] + sorted(bad.values()), capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "frame sanitizer job ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        (p.returncode, p.stdout[-500:], p.stderr[-3000:])
