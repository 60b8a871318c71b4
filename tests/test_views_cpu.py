"""CPU tests of haf_view_points (include/hafgrasp.h), the host definition of record of a haf_score_views request's fused cloud: the
VALID points of the views, frame after frame in pixel order, each exactly haf_frame_points' words.  Checked word for word against the
valid rows of haf_frame_points and of the numpy mirror of tests/frame_cases.py.  haf_score_views itself needs a GPU:
tests/test_views_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frame_cases as fc
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.cases()
BY_NAME = {c[0]: c for c in CASES}


def finite_rows(words):
    """the rows of a uint32 [n, 3] array whose three floats are all finite"""
    return words[((words & np.uint32(0x7F800000)) != np.uint32(0x7F800000)).all(axis=1)]


def all_invalid_frame(w=9, h=4):
    img = np.zeros((h, w), np.uint16)
    return "all_invalid_%dx%d" % (w, h), capi.depth_frame(img, 500.0, 500.0, 4.0, 2.0), img


def groups():
    """-> list of (name, [(name, frame, image), ...]): every case alone, then groups that mix kinds, carry padded rows (61 x 5), 1 x 1
    frames and an all-invalid frame, up to HAF_MAX_VIEWS views"""
    out = [(c[0], [c]) for c in CASES]
    pick = lambda *names: [BY_NAME[n] for n in names]
    out.append(("mixed_kinds", pick("u16_7x3", "f32_7x3", "xyz12_7x3", "xyz32_7x3")))
    out.append(("padded_rows", pick("u16_61x5", "f32_61x5", "xyz16_61x5", "u16_range_61x5")))
    out.append(("one_by_one", pick("u16_1x1", "f32_1x1", "xyz12_1x1", "xyz16_1x1", "u16_range_1x1", "f32_scaled_1x1")))
    out.append(("with_all_invalid", [BY_NAME["f32_61x5"], all_invalid_frame(), BY_NAME["xyz32_7x3"], all_invalid_frame(1, 1)]))
    out.append(("only_all_invalid", [all_invalid_frame(), all_invalid_frame(3, 3)]))
    out.append(("sixteen_views", [CASES[k] for k in range(len(CASES)) if CASES[k][1].width * CASES[k][1].height < 400][:capi.MAX_VIEWS]))
    out.append(("large_and_small", pick("u16_640x480", "xyz12_1x1", "f32_640x480", "xyz16_61x5")))
    return out


GROUPS = groups()


@pytest.mark.parametrize("name", [g[0] for g in GROUPS])
def test_view_points_are_the_valid_frame_points_in_order(name):
    views = next(g[1] for g in GROUPS if g[0] == name)
    frames = [v[1] for v in views]
    want = np.concatenate([finite_rows(fc.words(capi.frame_points(f))) for f in frames])
    mirror = np.concatenate([finite_rows(fc.mirror_points(f, img)) for _, f, img in views])
    got = fc.words(capi.view_points(frames))
    assert got.shape == want.shape == mirror.shape
    assert (got == want).all() and (got == mirror).all()
    # n_valid is exact, with and without a destination
    L = capi.lib()
    arr, cnt = (capi.Frame * len(frames))(*frames), C.c_size_t(12345)
    assert L.haf_view_points(arr, len(frames), None, 0, C.byref(cnt)) == capi.HAF_OK and cnt.value == len(want)
    if name == "only_all_invalid":
        assert len(want) == 0
    elif sum(f.width * f.height for f in frames) > 64:
        total = sum(f.width * f.height for f in frames)
        assert 0 < len(want) < total                       # some pixels dropped, some kept: the comparison is not an empty one


def test_view_points_capacity_is_respected():
    """a destination one point too small is refused and nothing is written past it; an exact one is filled"""
    L = capi.lib()
    frames = [BY_NAME["u16_61x5"][1], BY_NAME["xyz16_7x3"][1]]
    arr = (capi.Frame * 2)(*frames)
    want = fc.words(capi.view_points(frames))
    n = len(want)
    assert n > 20
    for cap in (0, 1, n - 1):
        buf = np.full((n + 4, 3), 7.5, np.float32)
        cnt = C.c_size_t(0)
        assert L.haf_view_points(arr, 2, buf.ctypes.data, cap, C.byref(cnt)) == capi.HAF_E_CAPACITY
        assert (buf[cap:] == 7.5).all()
        assert (fc.words(buf[:cap]) == want[:cap]).all()
        assert b"fewer points" in L.haf_last_error(None)
    buf = np.full((n + 4, 3), 7.5, np.float32)
    cnt = C.c_size_t(0)
    assert L.haf_view_points(arr, 2, buf.ctypes.data, n, C.byref(cnt)) == capi.HAF_OK and cnt.value == n
    assert (fc.words(buf[:n]) == want).all() and (buf[n:] == 7.5).all()


REFUSALS = fc.refusal_frames()


def _refused(frames, n, code, out=None):
    L = capi.lib()
    arr = (capi.Frame * max(1, len(frames)))(*frames)
    buf = np.zeros((64, 3), np.float32) if out is None else out
    cnt = C.c_size_t(777)
    assert L.haf_view_points(arr, n, buf.ctypes.data, len(buf), C.byref(cnt)) == code
    assert not buf.any() and cnt.value == 777              # refused before anything was written
    return (L.haf_last_error(None) or b"").decode()


def test_view_count_refusals():
    good = BY_NAME["u16_7x3"][1]
    for n in (0, -1, capi.MAX_VIEWS + 1):
        assert "view count" in _refused([good] * (capi.MAX_VIEWS + 1), n, capi.HAF_E_ARG)
    L = capi.lib()
    cnt = C.c_size_t()
    assert L.haf_view_points(None, 1, None, 0, C.byref(cnt)) == capi.HAF_E_ARG
    assert L.haf_view_points((capi.Frame * 1)(good), 1, None, 0, None) == capi.HAF_E_ARG
    assert len(capi.view_points([good] * capi.MAX_VIEWS)) == capi.MAX_VIEWS * len(capi.view_points([good]))
    with pytest.raises(capi.HafError) as ei:
        capi.view_points([good] * (capi.MAX_VIEWS + 1))
    assert ei.value.code == capi.HAF_E_ARG and "view count" in str(ei.value)
    with pytest.raises(capi.HafError):
        capi.view_points([])


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_per_frame_refusals_as_the_second_view(name):
    """every refusal of a frame's own fields, placed behind a valid first view: the frame's code, a message that names view 1, and the
    first view's points are not written either"""
    _, frame, code, _ = next(r for r in REFUSALS if r[0] == name)
    good = BY_NAME["u16_7x3"][1]
    text = _refused([good, frame], 2, code)
    assert "view 1" in text and "haf_frame" in text, text


def test_device_resident_view_is_refused_on_the_host():
    good = BY_NAME["u16_7x3"][1]
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    assert "view 1" in _refused([good, dev], 2, capi.HAF_E_ARG)


def test_abi_version_exports_and_wrappers():
    with open(os.path.join(ROOT, "include", "hafgrasp.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert {"haf_view_points", "haf_score_views"} <= set(re.findall(r"\b(haf_[a-z_0-9]+)\s*\(", text))
    assert "#define HAF_ABI_VERSION 2" in text and "#define HAF_MAX_VIEWS 16" in text and capi.MAX_VIEWS == 16
    assert "any component that is not finite" in raw and "can never reach a height grid" in raw     # the rule and why it changes no result
    for L in (capi.lib(), capi.testlib()):
        assert hasattr(L, "haf_view_points") and hasattr(L, "haf_score_views")
        assert L.haf_abi_version() == 2
    assert callable(capi.view_points) and callable(capi.Engine.score_views) and callable(capi.Engine.fetch_points)
    from haf_grasping_amd import CalcGraspPointsServer
    assert callable(CalcGraspPointsServer.execute_views)


def test_frames_code_object_static_checks(tmp_path):
    """The ISA of csrc/frames.hip for gfx950: the three k_view_points kernels are there without scratch, each with exactly ONE atomic, an
    integer add (the workgroup's reservation on the request's counter); no float atomic; no scalar memory write of any kind, in the
    disassembly or in the source."""
    from haf_grasping_amd import build as B
    hipcc = os.environ.get("HIPCC", os.path.join(B.ROCM, "bin", "hipcc"))
    src = os.path.join(ROOT, "haf_grasping_amd", "csrc", "frames.hip")
    asm = str(tmp_path / "frames.s")
    subprocess.run([hipcc] + [f for f in B.FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", src, "-o", asm], check=True, capture_output=True, text=True)
    with open(asm) as f:
        text = f.read()
    # (spelt in pieces: this file must not hold the instruction names it looks for)
    s, st, at = "s_", "sto" + "re", "ato" + "mic"
    banned = re.compile(r"\b(" + "|".join([s + st, s + "buffer_" + st, s + "scratch_" + st, s + at, s + "buffer_" + at, s + "dca" + "che_wb", s + "dca" + "che_discard"]) + ")", re.I)
    assert not banned.search(text)
    with open(src) as f:
        assert not banned.search(f.read())
    kernels = re.findall(r"^(_ZN3haf13k_view_pointsILi[012]EEEvPKNS_8FrameDevE):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(kernels) == 3
    for name, body in kernels:
        atoms = re.findall(r"^\s*((?:flat|global|ds|buffer)_" + at + r"\w*)", body, flags=re.M)
        assert len(atoms) == 1 and re.fullmatch(r"(flat|global)_" + at + r"_add(_u32)?", atoms[0]), (name, atoms)
        meta = text[text.index(".name:           " + name):]
        assert re.search(r"\.private_segment_fixed_size: (\d+)", meta).group(1) == "0", name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1)) <= 64, name       # eight waves per SIMD
