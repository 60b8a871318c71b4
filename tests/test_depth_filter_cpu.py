"""The host definition of record of the depth filter (include/hafgrasp.h: haf_filter_depth_ref): no device, no engine.  Against an
independent numpy-fp32 mirror word for word, its properties, the flying-pixel scene it exists for, every refusal, and the host units
under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_filter_cases as dc
import frame_cases as fc
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stacks():
    return dc.stacks()


def test_defaults_and_struct_layout():
    p = capi.depth_filter()
    assert (p.radius, p.min_support, p.min_valid) == (2, 6, 1)
    assert np.float32(p.tol_abs) == np.float32(0.004) and np.float32(p.tol_rel) == np.float32(0.01)
    assert C.sizeof(capi.DepthFilter) == 20 and capi.MAX_STACK == 8
    with pytest.raises(TypeError):
        capi.depth_filter(support=3)
    for L in (capi.lib(), capi.testlib()):
        assert hasattr(L, "haf_filter_depth") and hasattr(L, "haf_filter_depth_ref") and hasattr(L, "haf_depth_filter_default")
    assert capi.lib().haf_abi_version() == 2
    capi.lib().haf_depth_filter_default(None)


def test_reference_equals_numpy_mirror_word_for_word(stacks):
    """every stack of depth_filter_cases under its whole parameter sweep, and the tie cases against their written-out images"""
    seen = set()
    for name, frames, images in stacks:
        for p in dc.sweep(len(frames)):
            got, stats = capi.filter_depth_ref(frames, p)
            want, want_stats = dc.mirror_filter(frames[0], images, p)
            assert (dc.words(got) == dc.words(want)).all() and stats == want_stats, (name, dc.param_id(p), stats, want_stats)
            if "one_dead" not in name and images[0].size > 1000 and p.min_valid == 1 and p.min_support not in (0, (2 * p.radius + 1) ** 2 - 1):
                assert 0 < stats[2] < stats[1] < stats[0], (name, dc.param_id(p), stats)      # (the sweep decides something)
            seen.add((len(frames), p.radius, p.min_valid))
    assert len(seen) == 3 * (1 + 2 + 2 + 2)
    for name, frames, images, p, want in dc.tie_cases():
        got, stats = capi.filter_depth_ref(frames, p)
        mirror, mirror_stats = dc.mirror_filter(frames[0], images, p)
        assert (dc.words(got) == dc.words(want)).all() and (dc.words(mirror) == dc.words(want)).all(), name
        assert stats == mirror_stats == [21, 3, 2 if p.min_support == 1 else 0], (name, stats)


def test_every_count_of_valid_samples_occurs(stacks):
    """the stacks are what the issue asks for: a pixel's number of valid samples takes every value 0..n"""
    for name, frames, images in stacks:
        n = len(frames)
        if images[0].size < 4000 or "one_dead" in name:
            continue
        counts = set()
        for mv in range(1, n + 1):
            _, s = dc.mirror_filter(frames[0], images, capi.depth_filter(min_support=0, min_valid=mv))
            counts.add(s[1])
        assert len(counts) == n and 0 < min(counts) and max(counts) < images[0].size, (name, counts)


def test_single_exposure_without_support_canonicalises_the_input(stacks):
    for name, frames, images in stacks:
        if len(frames) != 1:
            continue
        got, stats = capi.filter_depth_ref(frames, capi.depth_filter(min_support=0))
        valid = np.isfinite(capi.frame_points(frames[0])).all(axis=1).reshape(got.shape)      # the frame's own validity (identity pose)
        if got.dtype == np.uint16:
            assert (got == np.where(valid, images[0], 0)).all(), name
        else:
            assert (dc.words(got) == np.where(valid, dc.words(images[0]), dc.NAN_WORD)).all(), name
        assert stats == [got.size, int(valid.sum()), int(valid.sum())]


def test_output_samples_are_input_samples_and_the_kept_set_shrinks(stacks):
    for name, frames, images in stacks:
        for radius in (1, 2, 3):
            prev = None
            for s in range(0, (2 * radius + 1) ** 2, max(1, radius * radius)):
                p = capi.depth_filter(radius=radius, min_support=s, tol_abs=0.3, tol_rel=0.1)
                got, stats = capi.filter_depth_ref(frames, p)
                w = dc.words(got)
                kept = (w != 0) if got.dtype == np.uint16 else (w != dc.NAN_WORD)
                assert int(kept.sum()) == stats[2]
                among = np.zeros(got.shape, bool)
                for img in images:
                    among |= dc.words(img) == w
                assert among[kept].all(), name                       # every valid output sample is one of its pixel's inputs
                if prev is not None:
                    assert not (kept & ~prev).any(), (name, radius, s)
                prev = kept


def test_padding_of_a_wide_output_keeps_its_sentinel(stacks):
    for name, frames, images in stacks:
        h, w = images[0].shape
        wide = np.full((h, w + 5), 0x5A5A if images[0].dtype == np.uint16 else 12345.0, images[0].dtype)
        p = capi.depth_filter(radius=1, min_support=1, tol_abs=0.3, tol_rel=0.1)
        got, stats = capi.filter_depth_ref(frames, p, out=wide[:, :w])
        packed, packed_stats = capi.filter_depth_ref(frames, p)
        assert (dc.words(wide[:, :w]) == dc.words(packed)).all() and stats == packed_stats, name
        assert (wide[:, w:] == (0x5A5A if images[0].dtype == np.uint16 else np.float32(12345.0))).all(), name


SCENE_PARAMS = [(1, 3), (2, 6), (3, 6)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("radius,support", SCENE_PARAMS)
def test_flying_pixels_are_removed_and_nothing_else(n, radius, support):
    """The condition the filter exists for.  A planted pixel has at most two planted neighbours in its window and lies 40 mm or more from
    both surfaces, against a tolerance of at most 4 + 0.01 x 960 mm; every surface pixel, image corners included, has at least
    `support` neighbours of its own surface, whose noise (sigma 1.5 mm) stays far inside 4 + 0.01 x 800 = 12 mm."""
    exposures, planted = dc.flying_pixel_scene()
    frames = [capi.depth_frame(img, 525.0, 525.0, 47.5, 31.5) for img in exposures[:n]]
    p = capi.depth_filter(radius=radius, min_support=support, tol_abs=0.004, tol_rel=0.01)
    got, stats = capi.filter_depth_ref(frames, p)
    assert planted.sum() == 32
    assert ((got == 0) == planted).all()
    assert stats == [6144, 6144, 6112]
    mirror, mirror_stats = dc.mirror_filter(frames[0], exposures[:n], p)
    assert (mirror == got).all() and mirror_stats == stats


def _refused(frames, p, out, stride, code):
    L = capi.lib()
    n = len(frames) if frames is not None else 1
    arr = (capi.Frame * max(1, n))(*(frames or []))
    before = None if out is None else out.tobytes()
    st = (C.c_int64 * 3)(-7, -7, -7)
    rc = L.haf_filter_depth_ref(arr if frames is not None else None, n, C.byref(p) if p is not None else None,
                                out.ctypes.data if out is not None else None, stride, st)
    assert rc == code, (rc, code)
    assert list(st) == [-7, -7, -7]
    if out is not None:
        assert out.tobytes() == before                               # a refused call writes nothing


def depth_stack_refusals():
    """-> ([(name, frames, params)] that both entry points refuse with HAF_E_ARG, the 3 x 4 image behind the frames); shared with the GPU suite"""
    img = np.full((3, 4), 1000, np.uint16)
    good = lambda **kw: capi.depth_frame(img, 500.0, 500.0, 2.0, 1.5, **kw)
    fimg = np.ones((3, 4), np.float32)
    nan, inf = float("nan"), float("inf")
    P = capi.depth_filter
    out = [("xyz_frame", [capi.xyz_frame(np.ones((3, 4, 3), np.float32))], P()),
           ("second_is_xyz", [good(), capi.xyz_frame(np.ones((3, 4, 3), np.float32))], P()),
           ("kind_differs", [good(), capi.depth_frame(fimg, 500.0, 500.0, 2.0, 1.5, depth_scale=0.001)], P()),
           ("width_differs", [good(), capi.depth_frame(np.ones((3, 5), np.uint16), 500.0, 500.0, 2.0, 1.5)], P()),
           ("height_differs", [good(), capi.depth_frame(np.ones((4, 4), np.uint16), 500.0, 500.0, 2.0, 1.5)], P()),
           ("scale_differs", [good(), good(depth_scale=0.002)], P()),
           ("min_depth_differs", [good(), good(min_depth=0.1)], P()),
           ("max_depth_differs", [good(max_depth=2.0), good()], P()),
           ("nine_frames", [good()] * 9, P()),
           ("radius_0", [good()], P(radius=0)), ("radius_4", [good()], P(radius=4)),
           ("support_negative", [good()], P(min_support=-1)), ("support_25_at_radius_2", [good()], P(min_support=25)),
           ("support_9_at_radius_1", [good()], P(radius=1, min_support=9)),
           ("tol_abs_negative", [good()], P(tol_abs=-0.001)), ("tol_abs_nan", [good()], P(tol_abs=nan)), ("tol_abs_inf", [good()], P(tol_abs=inf)),
           ("tol_rel_negative", [good()], P(tol_rel=-1.0)), ("tol_rel_nan", [good()], P(tol_rel=nan)), ("tol_rel_inf", [good()], P(tol_rel=inf)),
           ("min_valid_0", [good()], P(min_valid=0)), ("min_valid_above_n", [good(), good()], P(min_valid=3))]
    return out, img


def test_every_refusal_has_its_code_and_writes_nothing():
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    cases, img = depth_stack_refusals()
    out = np.full((3, 4), 0x7777, np.uint16)
    for name, frames, p in cases:
        _refused(frames, p, out, 8, A)
    good = capi.depth_frame(img, 500.0, 500.0, 2.0, 1.5)
    p = capi.depth_filter()
    _refused(None, p, out, 8, A)
    _refused([good], None, out, 8, A)
    _refused([], p, out, 8, A)
    # everything check_frame refuses for a frame, as the first and as the second exposure
    for name, frame, code, _ in fc.refusal_frames():
        if frame.kind == capi.FRAME_XYZ_F32:
            code = code if code == CAP else A
        _refused([frame], p, out, 8, code)
        if frame.kind == capi.FRAME_DEPTH_U16:
            _refused([good, frame], p, out, 8, code)
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    _refused([dev], p, out, 8, A)                                    # the _ref form touches no device
    _refused([good, dev], p, out, 8, A)
    # the output image
    _refused([good], p, None, 8, A)
    _refused([good], p, out, 6, A)                                   # a stride smaller than a row
    wide = np.full((3, 5), 0x7777, np.uint16)
    _refused([good], p, wide, 9, A)                                  # ... not a multiple of the element
    odd = np.full(32, 0x77, np.uint8)
    L = capi.lib()
    arr = (capi.Frame * 1)(good)
    assert L.haf_filter_depth_ref(arr, 1, C.byref(p), odd.ctypes.data + 1, 8, None) == A and (odd == 0x77).all()      # ... misaligned
    before = img.copy()
    assert L.haf_filter_depth_ref(arr, 1, C.byref(p), img.ctypes.data, 8, None) == A and (img == before).all()        # out is an input
    assert L.haf_filter_depth_ref(arr, 1, C.byref(p), out.ctypes.data, 8, None) == capi.HAF_OK                       # (stats may be NULL)


def test_filter_paths_under_address_and_ub_sanitizers(tmp_path):
    """CPU sanitizer job of the filter's host units: depthfilter_host.cpp + frames_host.cpp + parsers.cpp built with
    -fsanitize=address,undefined and driven by tests/sanitize/filter_paths.cpp, a program of its own, over exactly sized heap blocks:
    widths 1 / 3 / 61 / 64, heights 1 / 5, padded input and output rows whose last row ends with its allocation, every radius, stacks
    of 1 and 8, and the refusals that must come before the first sample is read.  Any report fails."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    if clang is None:
        pytest.skip("no host C++ compiler with sanitizers")
    csrc = os.path.join(ROOT, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "filter_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-ffp-contract=off"]
    cmd = [clang] + flags + [os.path.join(csrc, "depthfilter_host.cpp"), os.path.join(csrc, "frames_host.cpp"), os.path.join(csrc, "parsers.cpp"),
                             os.path.join(ROOT, "tests", "sanitize", "filter_paths.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "filter sanitizer job ok" in p.stdout and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        (p.returncode, p.stdout[-500:], p.stderr[-3000:])
