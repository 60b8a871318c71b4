"""haf_filter_depth on the MI355X (include/hafgrasp.h; csrc/depthfilter.hip): the kernel against haf_filter_depth_ref word for word on
every case of depth_filter_cases -- host, device-resident and mixed exposures, into host memory, into the caller's padded device image
and into the engine's own -- a 640 x 480 stack, the composition with the scoring calls, the engine's state, the refusals and the CLI.
Testing build, with the canary check after every test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import depth_filter_cases as dc
import frame_cases as fc
import pcdio
from haf_grasping_amd import capi
from test_depth_filter_cpu import depth_stack_refusals
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, _files, assert_same, device_copy, make_engine, pose, render_depth, snapshot, tilt

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE


@pytest.fixture(scope="module")
def surrogate(golden_dir):
    return os.path.join(golden_dir, "surrogate.model")


@pytest.fixture(autouse=True)
def _canaries():
    yield
    bad, report, n = capi.check_canaries()
    assert bad == 0, report


@pytest.fixture(scope="module")
def eng(data_dir, surrogate):
    e = make_engine(data_dir, surrogate, max_points=1 << 21)
    yield e
    e.close()


@pytest.fixture(scope="module")
def stacks():
    return dc.stacks()


_hip = None


def fetch(ptr, nbytes):
    """device memory -> uint8 [nbytes]"""
    global _hip
    if _hip is None:
        # the HIP runtime this process has loaded already (the engine's): a second copy from another path would not share its state
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        _hip = C.CDLL(path)
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    assert _hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0
    return out


def rows_of(flat, frame, dtype):
    """the pixels of a fetched image whose rows are frame.row_stride_bytes apart -> (image, the padding bytes between the rows)"""
    h, w, stride, e = frame.height, frame.width, frame.row_stride_bytes, np.dtype(dtype).itemsize
    img = np.stack([flat[v * stride:v * stride + w * e].view(dtype) for v in range(h)])
    pad = np.concatenate([flat[v * stride + w * e:(v + 1) * stride] for v in range(h - 1)] + [np.empty(0, np.uint8)])
    return img, pad


def device_image(frame, dtype, pad_elems=3):
    """a caller's device image for exposures like `frame`: padded rows, filled with SENTINEL -> (tensor, pointer, stride, bytes)"""
    import torch
    e = np.dtype(dtype).itemsize
    stride = (frame.width + pad_elems) * e
    nbytes = (frame.height - 1) * stride + frame.width * e
    t = torch.full((nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = t.data_ptr() + (-t.data_ptr() % 16) + e                    # one element past a 16-byte boundary
    return t, ptr, stride, nbytes


def check_outputs(eng, use, p, want, want_stats, dtype, name, modes=("host", "device", "engine")):
    for mode in modes:
        if mode == "host":
            wide = np.full((want.shape[0], want.shape[1] + 2), 0x5A5A if dtype == np.uint16 else 12345.0, dtype)
            frame, stats = eng.filter_depth(use, p, host_out=wide[:, :want.shape[1]])
            got = frame.image
            assert frame.on_device == 0 and frame.data == wide.ctypes.data
            assert (wide[:, want.shape[1]:] == (0x5A5A if dtype == np.uint16 else np.float32(12345.0))).all(), (name, mode)
        elif mode == "device":
            keep, ptr, stride, nbytes = device_image(use[0], dtype)
            frame, stats = eng.filter_depth(use, p, device_out=(ptr, stride))
            assert frame.on_device == 1 and frame.data == ptr and frame.row_stride_bytes == stride
            got, pad = rows_of(fetch(ptr, nbytes), frame, dtype)
            assert (pad == SENTINEL).all(), (name, mode)
            whole = keep.cpu().numpy()
            off = ptr - keep.data_ptr()
            assert (whole[:off] == SENTINEL).all() and (whole[off + nbytes:] == SENTINEL).all(), (name, mode)
        else:
            frame, stats = eng.filter_depth(use, p)
            assert frame.on_device == 1 and frame.row_stride_bytes == frame.width * np.dtype(dtype).itemsize
            got, _ = rows_of(fetch(frame.data, frame.height * frame.row_stride_bytes), frame, dtype)
        bad = np.flatnonzero(dc.words(got).reshape(-1) != dc.words(want).reshape(-1))
        assert bad.size == 0 and stats == want_stats, (name, mode, dc.param_id(p), bad[:5], stats, want_stats)
        assert (frame.kind, frame.width, frame.height, frame.depth_scale, frame.min_depth, frame.max_depth) == \
            (use[0].kind, use[0].width, use[0].height, use[0].depth_scale, use[0].min_depth, use[0].max_depth)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", ["%dx%d" % s for s in dc.SHAPES])
def test_kernel_equals_host_definition_word_for_word(eng, stacks, kind, shape):
    """every stack of this kind and shape under its whole parameter sweep: host exposures, device-resident ones (a base that is not a
    multiple of 16, the host's row padding) and a mix of the two, each into all three kinds of output in turn"""
    seen = 0
    for name, frames, images in stacks:
        if not name.startswith("%s_%s_" % (kind, shape)):
            continue
        dtype = images[0].dtype
        dev = [device_copy(f, i) for f, i in zip(frames, images)]
        mixed = [d if k % 2 == 0 else f for k, (f, d) in enumerate(zip(frames, dev))]
        for j, p in enumerate(dc.sweep(len(frames))):
            want, want_stats = capi.filter_depth_ref(frames, p)
            order = ("host", "device", "engine")
            for i, (label, use) in enumerate((("host", frames), ("device", dev), ("mixed", mixed))):
                # (every source into one kind of output per parameter set, all nine pairs within any three consecutive sets)
                check_outputs(eng, use, p, want, want_stats, dtype, name + "/" + label, modes=(order[(i + j) % 3],))
            seen += 1
        check_outputs(eng, mixed, dc.sweep(len(frames))[1], *capi.filter_depth_ref(frames, dc.sweep(len(frames))[1]), dtype, name + "/all outputs")
    assert seen >= 9 + 3 * 18


def test_tie_cases_and_the_flying_pixel_scene(eng):
    for name, frames, images, p, want in dc.tie_cases():
        ref, ref_stats = capi.filter_depth_ref(frames, p)
        assert (dc.words(ref) == dc.words(want)).all()
        check_outputs(eng, frames, p, want, ref_stats, images[0].dtype, name)
        check_outputs(eng, [device_copy(frames[0], images[0])], p, want, ref_stats, images[0].dtype, name + "/device", modes=("engine",))
    exposures, planted = dc.flying_pixel_scene()
    for n in (1, 3):
        frames = [capi.depth_frame(img, 525.0, 525.0, 47.5, 31.5) for img in exposures[:n]]
        for radius, support in ((1, 3), (2, 6), (3, 6)):
            frame, stats = eng.filter_depth(frames, capi.depth_filter(radius=radius, min_support=support), host_out=True)
            assert ((frame.image == 0) == planted).all() and stats == [6144, 6144, 6112]


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_vga_stack_of_three(eng, kind):
    rng = np.random.default_rng(5)
    if kind == "u16":
        images = [fc.u16_image(rng, 640, 480) for _ in range(3)]
        frames = [capi.depth_frame(i, **K525, **dc.U16_KW) for i in images]
    else:
        images = [fc.f32_image(rng, 640, 480, (0.5, 2.5)) for _ in range(3)]
        frames = [capi.depth_frame(i, **K525, **dc.F32_KW) for i in images]
    p = capi.depth_filter(radius=2, min_support=6, tol_abs=0.3, tol_rel=0.1)
    want, want_stats = capi.filter_depth_ref(frames, p)
    assert 0 < want_stats[2] < want_stats[1] < want_stats[0] == 640 * 480
    dev = [device_copy(f, i) for f, i in zip(frames, images)]
    check_outputs(eng, frames, p, want, want_stats, images[0].dtype, "vga/host")
    check_outputs(eng, [dev[0], frames[1], dev[2]], p, want, want_stats, images[0].dtype, "vga/mixed")


def _table1_with_flying_pixels(data_dir):
    xyz = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    s2b = pose(tilt(0.05, -0.1, 0.2), (0.13, 0.2, 0.9))
    depth = render_depth(xyz, s2b)
    rng = np.random.default_rng(3)
    valid = np.argwhere(depth[1:-1, 1:-1] > 0) + 1
    pick = valid[rng.choice(len(valid), 400, replace=False)]
    planted = depth.copy()
    planted[pick[:, 0], pick[:, 1]] = (depth[pick[:, 0], pick[:, 1]].astype(np.int64) - rng.integers(60, 200, len(pick))).astype(np.uint16)
    return planted, s2b


def test_filtered_frame_composes_with_the_scoring_calls(data_dir, surrogate):
    """filter_depth on the device, then score_frames / score_frames_roi on the returned device frame == the same calls on a host frame
    built from filter_depth_ref's image"""
    planted, s2b = _table1_with_flying_pixels(data_dir)
    kw = dict(sensor_to_base=s2b, min_depth=0.2, max_depth=1.5, **K525)
    raw = capi.depth_frame(planted, **kw)
    p = capi.depth_filter()
    want, want_stats = capi.filter_depth_ref([raw], p)
    assert 400 <= want_stats[1] - want_stats[2] < 1000 and want_stats[2] > 40000          # the 400 planted pixels go, the surfaces stay
    host = capi.depth_frame(want, **kw)
    e = make_engine(data_dir, surrogate, max_points=1 << 20, **C3_CFG)
    inp = capi.default_input(**C3_IN)
    mask = np.zeros(planted.shape, np.uint8)
    mask[120:400, 150:520] = 1
    a = snapshot(e, e.score_frames([host], [inp])[0])
    a_roi = snapshot(e, e.score_frames_roi([host], [mask], [inp])[0])
    assert a["out"]["n_evals"] >= 10000 and a["out"]["eval"] > -20 and 0 < a_roi["out"]["n_evals"] < a["out"]["n_evals"]
    frame, stats = e.filter_depth([raw], p)
    assert stats == want_stats and frame.on_device == 1
    assert_same(snapshot(e, e.score_frames([frame], [inp])[0]), a)
    frame, stats = e.filter_depth([device_copy(raw, planted)], p)
    assert_same(snapshot(e, e.score_frames_roi([frame], [mask], [inp])[0]), a_roi)
    # the Python mirror of the action interface
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(*_files(data_dir), surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    res = srv.execute_frame_filtered(goal, [raw], p)
    assert srv.last_filter_stats == want_stats and res == srv.execute_frame(goal, host) and res.eval == a["out"]["eval"]
    srv.close()
    e.close()


def test_filter_leaves_the_last_batch_alone_and_needs_none(data_dir, golden_dir, surrogate, tmp_path):
    import json
    import models
    planted, s2b = _table1_with_flying_pixels(data_dir)
    raw = capi.depth_frame(planted, sensor_to_base=s2b, **K525)
    p = capi.depth_filter()
    want, want_stats = capi.filter_depth_ref([raw], p)
    e = make_engine(data_dir, surrogate, max_points=1 << 20, **C3_CFG)
    got, stats = e.filter_depth([raw], p, host_out=True)                     # a fresh engine, before any request
    assert (got.image == want).all() and stats == want_stats
    inp = capi.default_input(**C3_IN)
    out = e.score_frames([raw], [inp])[0]
    before, map_before, ms_before = snapshot(e, out), e.grasp_map(0, raw), e.stage_ms()
    for kw in (dict(host_out=True), dict(), dict()):
        e.filter_depth([raw, device_copy(raw, planted)], capi.depth_filter(radius=3, min_valid=2), **kw)
    assert_same(snapshot(e, out), before)
    map_after = e.grasp_map(0, raw)
    assert all((map_before[k] == map_after[k]).all() for k in map_before) and e.stage_ms() == ms_before
    e.close()
    with open(os.path.join(golden_dir, "surrogate_prob.json")) as f:
        pj = json.load(f)
    mp = models.write_probability_model(str(tmp_path / "surrogate_prob.model"), surrogate, pj["probA"], pj["probB"])
    e = make_engine(data_dir, mp, capi.FLAG_PROBABILITY, max_points=1 << 20)
    got, stats = e.filter_depth([raw], p, host_out=True)
    assert (got.image == want).all() and stats == want_stats
    e.close()


def test_engine_side_refusals_do_no_device_work(data_dir, surrogate):
    """every refusal returns its code and a text that names the call, writes nothing and leaves the engine usable: the next valid call
    gives the right image"""
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    e = make_engine(data_dir, surrogate, max_points=4096)
    L, h = e._L, e._h
    rng = np.random.default_rng(9)
    img = fc.u16_image(rng, 61, 5)
    good = capi.depth_frame(img, **K525)
    p = capi.depth_filter(radius=1, min_support=1, tol_abs=0.3, tol_rel=0.1)
    want, want_stats = capi.filter_depth_ref([good], p)
    canvas = np.full((64, 80), 0x7777, np.uint16)

    def refused(frames, params, code, out=canvas, stride=160, on_device=0, n=None):
        n = (len(frames) if frames is not None else 1) if n is None else n
        arr = (capi.Frame * max(1, len(frames or [])))(*(frames or []))
        st, of = (C.c_int64 * 3)(-7, -7, -7), capi.Frame()
        rc = L.haf_filter_depth(h, arr if frames is not None else None, n, C.byref(params) if params is not None else None,
                                out.ctypes.data if isinstance(out, np.ndarray) else out, stride, on_device, C.byref(of), st)
        text = (L.haf_last_error(h) or b"").decode()
        assert rc == code and text.startswith("haf_filter_depth: "), (rc, code, text)
        assert list(st) == [-7, -7, -7] and of.data is None and (canvas == 0x7777).all()
        got, stats = e.filter_depth([good], p, host_out=True)
        assert (got.image == want).all() and stats == want_stats
        return text

    cases, small = depth_stack_refusals()
    for name, frames, params in cases:
        text = refused(frames, params, A)
        if name.endswith("_differs") or name == "second_is_xyz":
            assert "frame 1: " in text, (name, text)                          # the message names the frame
        elif name == "xyz_frame":
            assert "frame 0: " in text, (name, text)
    for name, frame, code, _ in fc.refusal_frames():
        assert "frame 0" in refused([frame], p, code if frame.kind != capi.FRAME_XYZ_F32 or code == CAP else A)
        if frame.kind == capi.FRAME_DEPTH_U16:
            assert "frame 1" in refused([capi.depth_frame(np.ones((3, 4), np.uint16), 500.0, 500.0, 2.0, 1.5), frame], p, code)
    refused(None, p, A)
    refused([good], None, A)
    refused([good], p, A, n=0)
    assert L.haf_filter_depth(None, (capi.Frame * 1)(good), 1, C.byref(p), canvas.ctypes.data, 160, 0, None, None) == A
    refused([good], p, A, on_device=2)
    refused([good], p, A, on_device=-1)
    refused([good], p, A, out=None)                                          # no host image
    refused([good], p, A, stride=120)                                        # 61 samples need 122 bytes
    refused([good], p, A, stride=123)
    refused([good], p, A, out=canvas.ctypes.data + 1)
    refused([good], p, A, out=img.ctypes.data, stride=122)                   # out is an input
    # capacities: 4096 points
    big = capi.depth_frame(np.ones((64, 65), np.uint16), **K525)             # 4160 pixels
    assert "max_points" in refused([big], p, CAP, out=None, on_device=1)
    half = [capi.depth_frame(np.ones((42, 50), np.uint16), **K525) for _ in range(2)]      # 2 x 2100 host pixels
    assert "max_points" in refused(half, p, CAP, out=None, on_device=1)
    assert "max_points" in refused(half[:1], p, CAP)                          # one host exposure and the host image
    dev = [device_copy(half[0], np.ones((42, 50), np.uint16)) for _ in range(2)]
    got, stats = e.filter_depth(dev, p)                                      # device-resident exposures into the engine's image: no staging
    assert stats[0] == 2100
    got, stats = e.filter_depth([half[0], dev[0]], p)
    assert stats[0] == 2100
    e.close()


def test_cli_filters_a_stack_and_prints_the_python_path_grasp(data_dir, surrogate, tmp_path):
    """haf_grasp_cli --depth A --stack B --stack C --depth-filter default --filtered-out F writes the reference's image and prints the
    grasp the Python path gives for the same stack; without --depth-filter the --stack files change nothing"""
    f_, r_ = _files(data_dir)
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "haf_grasp_cli")
    planted, s2b = _table1_with_flying_pixels(data_dir)
    rng = np.random.default_rng(11)
    exposures = []
    for j in range(3):
        img = planted.copy()
        img[img > 0] += rng.integers(0, 3, int((img > 0).sum())).astype(np.uint16)
        img[rng.random(img.shape) < 0.1 * j] = 0
        exposures.append(img)
    paths = [str(tmp_path / ("e%d.pgm" % j)) for j in range(3)]
    for path, img in zip(paths, exposures):
        fc.write_pgm16(path, img)
    frames = [capi.depth_frame(img, sensor_to_base=s2b, min_depth=0.2, max_depth=1.5, **K525) for img in exposures]
    want, want_stats = capi.filter_depth_ref(frames)
    common = [cli, "--features", f_, "--range", r_, "--model", surrogate, "--rolls", "20", "--roll-step", "9", "--center", "0.13", "0.25", "0",
              "--search-size", "42", "42"]
    src = ["--depth", paths[0], "--stack", paths[1], "--stack", paths[2], "--intrinsics", "525", "525", "319.5", "239.5", "--depth-range", "0.2", "1.5",
           "--sensor-pose"] + ["%.9g" % v for v in s2b]
    out_pgm = str(tmp_path / "filtered.pgm")
    a = subprocess.run(common + src + ["--depth-filter", "default", "--filtered-out", out_pgm], check=True, capture_output=True, text=True)
    assert (capi.load_pgm16(out_pgm) == want).all()
    assert "3 exposure(s) filtered: %d of %d pixels valid, %d kept" % (want_stats[1], want_stats[0], want_stats[2]) in a.stderr
    from haf_grasping_amd import CalcGraspPointsServer, GraspInputMsg
    srv = CalcGraspPointsServer(f_, r_, surrogate, max_points=1 << 20, **C3_CFG)
    goal = GraspInputMsg(grasp_area_center=(0.13, 0.25, 0.0), grasp_area_length_x=56, grasp_area_length_y=56)
    res = srv.execute_frame_filtered(goal, frames)
    final = a.stdout.strip().splitlines()
    assert len(final) == 1 and int(final[0].split()[0]) == res.eval > -20
    unfiltered = subprocess.run(common + src, check=True, capture_output=True, text=True)
    plain = subprocess.run(common + src[:2] + src[6:], check=True, capture_output=True, text=True)
    assert unfiltered.stdout == plain.stdout and int(plain.stdout.split()[0]) == srv.execute_frame(goal, frames[0]).eval
    srv.close()
    bad = subprocess.run(common + src + ["--depth-filter", "2,99,0.004,0.01"], capture_output=True, text=True)
    assert bad.returncode == 1 and "min_support" in bad.stderr
    assert subprocess.run(common + src + ["--depth-filter", "2,6"], capture_output=True, text=True).returncode == 2      # usage
