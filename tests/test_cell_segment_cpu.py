"""The host definition of record of the top-down cell clustering (include/hafgrasp.h: haf_segment_cells_ref): no device, no engine.
Against an independent numpy mirror word for word, the rules one at a time, the special values of every comparison, its independence
of the order of the points, organised against unorganised, the table1 fixture as a cloud, agreement with haf_segment_ref where both
apply, every refusal, and the host units under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cell_segment_cases as cc
import frame_cases as fc
import pcdio
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_defaults_exports_and_struct_layout(tmp_path):
    p = capi.cell_segment_params()
    assert list(p.plane) == [0.0, 0.0, 1.0, 0.0] and (p.nx, p.ny, p.connectivity, p.min_points, p.max_labels) == (1024, 1024, 8, 50, 255)
    assert F(p.min_height) == F(0.01) and p.max_height == 0.0 and F(p.cell) == F(0.01) and p.max_step == 0.0
    assert F(p.x0) == F(-5.12) and F(p.y0) == F(-5.12)
    with pytest.raises(TypeError):
        capi.cell_segment_params(gap=3)
    for L in (capi.lib(), capi.testlib()):
        assert all(hasattr(L, f) for f in ("haf_segment_cells", "haf_segment_cells_ref", "haf_cell_segment_default"))
        assert L.haf_abi_version() == 2
    capi.lib().haf_cell_segment_default(None)
    # the ctypes mirrors against the C compiler: size and the offset of every field
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    fields = [("haf_cell_segment_params", capi.CellSegmentParams), ("haf_cell_segment_info", capi.CellSegmentInfo)]
    src = "#include <cstdio>\n#include <cstddef>\n#include \"hafgrasp.h\"\nint main() {\n"
    for cname, cls in fields:
        src += "  printf(\"%%zu\", sizeof(%s));\n" % cname
        for name, _ in cls._fields_:
            src += "  printf(\" %%zu\", offsetof(%s, %s));\n" % (cname, name)
        src += "  printf(\"\\n\");\n"
    src += "  return 0;\n}\n"
    (tmp_path / "layout.cpp").write_text(src)
    exe = str(tmp_path / "layout")
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", exe], check=True, capture_output=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    for (cname, cls), line in zip(fields, lines):
        want = [C.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
        assert [int(x) for x in line.split()] == want, (cname, line, want)
    assert C.sizeof(capi.CellSegmentParams) == 60 and C.sizeof(capi.CellSegmentInfo) == 36


@pytest.mark.parametrize("grid", cc.GRIDS, ids=lambda g: "%dx%d" % g)
def test_reference_equals_numpy_mirror_on_every_grid(grid):
    """every pattern on the grid, 4- and 8-connectivity where they differ, uint8 and uint16: labels, cell_labels, infos and stats"""
    cases = cc.grid_cases([grid])
    assert len(cases) >= 3
    for name, frame, image, kw in cases:
        for dtype, cap in ((np.uint8, 255), (np.uint16, capi.MAX_LABELS)):
            p = capi.cell_segment_params(**dict(kw, max_labels=cap))
            got = capi.segment_cells_ref(frame, p, dtype, cell_labels=True)
            want = cc.mirror_cells(frame, image, p, dtype)
            assert cc.same(got, want), (name, dtype, got[2], want[2])


def test_components_cross_every_kind_of_seam():
    """the cases are what they are meant to be: on 130 x 33 the serpentine, the full grid and both staircases are ONE component each
    with 8-connectivity -- through vertical and horizontal tile seams and through the corner (63, 15) | (64, 16) in both diagonal
    directions -- and the staircases and the checkerboard fall apart with 4-connectivity"""
    seen = 0
    for name, frame, image, kw in cc.grid_cases([(130, 33)]):
        labels, infos, stats = capi.segment_cells_ref(frame, capi.cell_segment_params(**kw), np.uint16)
        if name.startswith(("serpentine", "full")) or name in ("diag_dr_130x33_c8", "diag_dl_130x33_c8", "checker_130x33_c8"):
            assert stats[4] == 1 and infos[0]["n_cells"] == stats[3], (name, stats)
            seen += 1
        if name in ("diag_dr_130x33_c8", "diag_dl_130x33_c8"):
            box = (48, 0, 80, 32) if "dr" in name else (47, 0, 79, 32)
            assert (infos[0]["ix_min"], infos[0]["iy_min"], infos[0]["ix_max"], infos[0]["iy_max"]) == box, (name, infos[0])
        if name in ("diag_dr_130x33_c4", "diag_dl_130x33_c4", "checker_130x33_c4"):
            assert stats[4] == stats[3] > 30, (name, stats)
            seen += 1
    assert seen == 8


def test_the_rules_one_at_a_time_frames_and_lines():
    for name, frame, image, kw, want in cc.rule_cases():
        p = capi.cell_segment_params(**kw)
        got = capi.segment_cells_ref(frame, p, cell_labels=True)
        assert (len(got[1]), got[2][4], got[2][5]) == want, (name, got[2])
        assert cc.same(got, cc.mirror_cells(frame, image, p)), name
        if name == "min_points_counts_points":
            assert list(got[1]["n_points"]) == [50] and list(got[1]["n_cells"]) == [1] and (got[1]["anchor_ix"][0], got[1]["anchor_iy"][0]) == (15, 7)
        if name == "max_labels_cap":
            assert int(got[0].max()) == 5 and int((got[3] != 0).sum()) == 5
    for name, frame, image, kw in cc.frame_cases() + cc.line_cases():
        p = capi.cell_segment_params(**kw)
        got = capi.segment_cells_ref(frame, p, np.uint16, cell_labels=True)
        assert cc.same(got, cc.mirror_cells(frame, image, p, np.uint16)), name
        assert name == "line_1" or got[2][3] > 0, (name, got[2])


def _one(points, **kw):
    """the labels of a few far-apart points on a 4 x 4 grid of 1 m cells from (1, 1), every foreground point kept"""
    image = np.asarray(points, F).reshape(1, -1, 3)
    base = dict(plane=[0, 0, 1, 0], min_height=0.25, max_height=0.75, cell=1.0, x0=1.0, y0=1.0, nx=4, ny=4, connectivity=4, min_points=1)
    base.update(kw)
    p = capi.cell_segment_params(**base)
    got = capi.segment_cells_ref(capi.xyz_frame(image), p, cell_labels=True)
    assert cc.same(got, cc.mirror_cells(capi.xyz_frame(image), image, p))
    return got


def test_special_values_one_at_a_time():
    below, above = (lambda v: float(np.nextafter(F(v), F(-np.inf)))), (lambda v: float(np.nextafter(F(v), F(np.inf))))
    # x == x0 is cell 0; the float just below x0 is outside, never cell 0; x0 + nx * cell is outside, the float below it is the last cell
    labels, infos, stats, grid = _one([(1.0, 1.0, 0.5), (below(1.0), 1.0, 0.5), (5.0, 3.5, 0.5), (below(5.0), 3.5, 0.5), (3.5, below(1.0), 0.5), (3.5, 5.0, 0.5)])
    assert list(labels[0]) == [1, 0, 0, 2, 0, 0] and stats == [6, 6, 4, 2, 2, 2]
    assert (infos["anchor_ix"][0], infos["anchor_iy"][0], infos["anchor_ix"][1], infos["anchor_iy"][1]) == (0, 0, 3, 2)
    assert grid[0, 0] == 1 and grid[2, 3] == 2 and int((grid != 0).sum()) == 2
    # -0.0 against an origin of 0 is cell 0, and the largest negative float is outside
    labels, infos, stats, grid = _one([(-0.0, -0.0, 0.5), (-1e-45, 0.5, 0.5)], x0=0.0, y0=0.0)
    assert list(labels[0]) == [1, 0] and stats[2] == 1 and grid[0, 0] == 1
    # |w| == 16 is usable, its successor is not: in x (the grid reaches it), and in z with a plane that still puts the point in the band
    labels, infos, stats, grid = _one([(16.0, 14.5, 0.5), (above(16.0), 14.5, 0.5), (-16.0, 14.5, 0.5)], x0=13.0, y0=13.0, nx=4)
    assert list(labels[0]) == [1, 0, 0] and stats[1:3] == [2, 1]
    labels, infos, stats, grid = _one([(1.5, 1.5, 16.0), (3.5, 1.5, above(16.0)), (1.5, 3.5, -16.0), (3.5, 3.5, below(-16.0))], plane=[0, 0, 0, 0.5])
    assert list(labels[0]) == [1, 0, 2, 0] and stats[1] == 2
    # a NaN or an infinity in any one word
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            q = [1.5, 1.5, 0.5]
            q[k] = bad
            labels, infos, stats, grid = _one([q, (3.5, 3.5, 0.5)], plane=[0, 0, 0, 0.5])
            assert list(labels[0]) == [0, 1] and stats == [2, 1, 0, 1, 1, 1], (bad, k)
    # h == min_height and h == max_height are foreground, their float neighbours outside the band are not
    zs = [below(0.25), 0.25, above(0.25), below(0.75), 0.75, above(0.75)]
    labels, infos, stats, grid = _one([(1.5 + 0.5 * i, 1.5 if i % 2 == 0 else 3.5, z) for i, z in enumerate(zs)], cell=0.5, nx=8, ny=8)
    assert list(labels[0] != 0) == [False, True, True, True, True, False] and stats[1] == 4
    # |top_a - top_b| == max_step links, the float below does not
    pair = [(1.5, 1.5, 0.25), (2.5, 1.5, 0.75)]
    assert _one(pair, max_step=0.5)[2][4] == 1 and _one(pair, max_step=below(0.5))[2][4] == 2


def test_a_permutation_of_the_points_permutes_the_labels_and_nothing_else():
    name, frame, image, kw = cc.grid_case("random", 130, 33)
    p = capi.cell_segment_params(**dict(kw, max_labels=capi.MAX_LABELS))
    base = capi.segment_cells_ref(frame, p, np.uint16, cell_labels=True)
    assert base[2][5] > 20
    perm = np.random.default_rng(5).permutation(image.shape[1])
    shuffled = np.ascontiguousarray(image[:, perm])
    got = capi.segment_cells_ref(capi.xyz_frame(shuffled), p, np.uint16, cell_labels=True)
    assert (got[0][0] == base[0][0][perm]).all() and got[1].tobytes() == base[1].tobytes() and got[2] == base[2] and (got[3] == base[3]).all()


@pytest.fixture(scope="module")
def table1(data_dir):
    from test_frames_gpu import K525, TABLE1, render_depth
    from test_views_gpu import CAM_A
    cloud = pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))
    da = render_depth(cloud, CAM_A)
    return np.ascontiguousarray(cloud[:, :3], F), capi.depth_frame(da, sensor_to_base=CAM_A, **K525), da, K525, CAM_A


def test_organised_and_unorganised_agree_point_for_point(table1):
    """the rendered table1 depth frame, and frame_points of it as an N x 1 XYZ frame under the identity pose"""
    xyz, fa, da, K525, CAM_A = table1
    p = capi.cell_segment_params(plane=[0, 0, 1, 0], min_height=0.03)
    organised = capi.segment_cells_ref(fa, p, cell_labels=True)
    pts = capi.frame_points(fa)
    flat = capi.segment_cells_ref(capi.cloud_frame(pts), p, cell_labels=True)
    assert len(organised[1]) >= 2 and (flat[0].reshape(-1) == organised[0].reshape(-1)).all()
    assert flat[1].tobytes() == organised[1].tobytes() and flat[2] == organised[2] and (flat[3] == organised[3]).all()


def test_table1_as_a_cloud(table1):
    """plane (0, 0, 1, 0), min_height 0.03, defaults otherwise: 8 objects of 559 points or more from 30 260 foreground points"""
    xyz = table1[0]
    p = capi.cell_segment_params(plane=[0, 0, 1, 0], min_height=0.03)
    labels, infos, stats, grid = capi.segment_cells_ref(capi.cloud_frame(xyz), p, cell_labels=True)
    assert len(infos) >= 2 and stats[2] == 0
    assert int(infos["n_points"].sum()) == stats[1] == int((labels != 0).sum())       # no component is dropped there
    assert stats[1] == 30260 and len(infos) == stats[4] == stats[5] == 8 and int(infos["n_points"].min()) >= 559, (stats, infos["n_points"])
    assert int((grid != 0).sum()) == stats[3] == int(infos["n_cells"].sum())
    assert cc.same((labels, infos, stats, grid), cc.mirror_cells(capi.cloud_frame(xyz), xyz.reshape(1, -1, 3), p))


def test_agrees_with_the_pixel_segmenter_on_well_separated_boxes():
    """a camera straight down on boxes two cells and more apart: the two references partition the foreground pixels identically up to
    numbering"""
    w, h, fx = 160, 120, 400.0
    z = np.full((h, w), 0.8, F)
    for k, (u0, v0, du, dv, top) in enumerate(((10, 10, 30, 25, 0.10), (60, 12, 20, 40, 0.06), (100, 20, 45, 20, 0.15), (20, 70, 50, 35, 0.08), (95, 65, 40, 40, 0.12))):
        z[v0:v0 + dv, u0:u0 + du] = F(0.8 - top)
    down = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0.8], F)                  # the camera 0.8 m above the plane z = 0, looking down
    frame = capi.depth_frame(z, fx, fx, (w - 1) / 2.0, (h - 1) / 2.0, sensor_to_base=down)
    a = capi.segment_ref(frame, capi.segment_params(plane=[0, 0, 1, 0], min_height=0.03, max_gap=0.01, min_pixels=20), np.uint8)
    b = capi.segment_cells_ref(frame, capi.cell_segment_params(plane=[0, 0, 1, 0], min_height=0.03, cell=0.005, x0=-1.0, y0=-1.0, nx=400, ny=400, min_points=20))
    assert len(a[1]) == len(b[1]) == 5 and a[2][1] == b[2][1] and b[2][2] == 0
    assert ((a[0] != 0) == (b[0] != 0)).all()
    pairs = np.unique(np.stack([a[0][a[0] != 0], b[0][a[0] != 0]]), axis=1)
    assert pairs.shape[1] == 5 and len(np.unique(pairs[0])) == len(np.unique(pairs[1])) == 5


def cell_refusals():
    """-> [(name, params kw, elem_bytes)] that both entry points refuse with HAF_E_ARG on a valid frame; shared with the GPU suite"""
    nan, inf = float("nan"), float("inf")
    return [("plane_nan", dict(plane=[0, nan, 1, 0]), 1), ("plane_inf", dict(plane=[0, 0, 1, inf]), 1), ("min_height_nan", dict(min_height=nan), 1),
            ("max_height_inf", dict(max_height=inf), 1), ("cell_0", dict(cell=0.0), 1), ("cell_small", dict(cell=0.0009), 1), ("cell_large", dict(cell=1.01), 1),
            ("cell_nan", dict(cell=nan), 1), ("cell_negative", dict(cell=-0.01), 1), ("x0_65", dict(x0=65.0), 1), ("y0_minus_65", dict(y0=-65.0), 1),
            ("x0_nan", dict(x0=nan), 1), ("y0_inf", dict(y0=inf), 1), ("nx_0", dict(nx=0), 1), ("ny_0", dict(ny=0), 1), ("nx_4097", dict(nx=4097, ny=1), 1),
            ("ny_4097", dict(nx=1, ny=4097), 1), ("cells_over", dict(nx=2048, ny=2049), 1), ("connectivity_6", dict(connectivity=6), 1),
            ("connectivity_0", dict(connectivity=0), 1), ("max_step_nan", dict(max_step=nan), 1), ("max_step_inf", dict(max_step=inf), 1),
            ("min_points_0", dict(min_points=0), 1), ("max_labels_0", dict(max_labels=0), 2), ("max_labels_256_uint8", dict(max_labels=256), 1),
            ("max_labels_4097", dict(max_labels=capi.MAX_LABELS + 1), 2), ("elem_bytes_0", {}, 0), ("elem_bytes_3", {}, 3), ("elem_bytes_4", {}, 4)]


def _refused(frame, p, out, elem, stride, code, n_ptr=True):
    before = None if out is None else out.tobytes()
    info = np.full(8, -7, capi.CELL_SEGMENT_INFO_DTYPE)
    grid = np.full((1024, 1024), 0x7777, np.uint16)
    n, st = C.c_int32(-7), (C.c_int64 * 6)(*[-7] * 6)
    rc = capi.lib().haf_segment_cells_ref(C.byref(frame) if frame is not None else None, C.byref(p) if p is not None else None,
                                          out.ctypes.data if out is not None else None, elem, stride, grid.ctypes.data, info.ctypes.data,
                                          C.byref(n) if n_ptr else None, st)
    assert rc == code, (rc, code)
    assert n.value == -7 and list(st) == [-7] * 6 and (info["n_points"] == -7).all() and (grid == 0x7777).all()
    if out is not None:
        assert out.tobytes() == before                               # a refused call writes nothing


def test_every_refusal_has_its_code_and_writes_nothing():
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    img = np.full((3, 4), 650, np.uint16)
    good = capi.depth_frame(img, 500.0, 500.0, 2.0, 1.5)
    out = np.full((3, 4), 0x77, np.uint8)
    out16 = np.full((3, 4), 0x7777, np.uint16)
    p = capi.cell_segment_params()
    for name, kw, elem in cell_refusals():
        _refused(good, capi.cell_segment_params(**kw), out16 if elem == 2 else out, elem, 8 if elem == 2 else 4, A)
    _refused(None, p, out, 1, 4, A)
    _refused(good, None, out, 1, 4, A)
    _refused(good, p, out, 1, 4, A, n_ptr=False)
    for name, frame, code, _ in fc.refusal_frames():                 # everything check_frame refuses for a frame
        _refused(frame, p, out, 1, 4 if code != CAP else 65536, code)
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    _refused(dev, p, out, 1, 4, A)                                   # the _ref form touches no device
    _refused(good, p, None, 1, 4, A)
    _refused(good, p, out, 1, 3, A)                                  # a stride smaller than a row
    wide = np.full((3, 5), 0x7777, np.uint16)
    _refused(good, p, wide, 2, 9, A)                                 # ... not a multiple of the element
    odd = np.full(32, 0x77, np.uint8)
    n = C.c_int32(-7)
    L = capi.lib()
    assert L.haf_segment_cells_ref(C.byref(good), C.byref(p), odd.ctypes.data + 1, 2, 8, None, None, C.byref(n), None) == A and (odd == 0x77).all()
    before = img.copy()
    assert L.haf_segment_cells_ref(C.byref(good), C.byref(p), img.ctypes.data, 2, 8, None, None, C.byref(n), None) == A and (img == before).all()
    assert n.value == -7
    # the edges of the ranges are accepted (the grid, info and stats may be NULL)
    for kw in (dict(cell=0.001), dict(cell=1.0), dict(x0=64.0, y0=-64.0), dict(nx=4096, ny=1024), dict(nx=1, ny=1), dict(connectivity=4), dict(max_step=-1.0)):
        assert L.haf_segment_cells_ref(C.byref(good), C.byref(capi.cell_segment_params(**kw)), out.ctypes.data, 1, 4, None, None, C.byref(n), None) == capi.HAF_OK, kw


def test_cell_paths_under_address_and_ub_sanitizers(tmp_path):
    """CPU sanitizer job of the cell segmenter's host units: cellsegment_host.cpp + segment_host.cpp + frames_host.cpp + parsers.cpp built
    with -fsanitize=address,undefined and driven by tests/sanitize/cell_paths.cpp, a program of its own, over exactly sized heap blocks:
    N x 1 clouds with N = 1 / 63 / 65 / 1000, small frames of all three kinds with padded input and output rows, grids down to one row
    and one column, a label grid of exactly nx * ny words, an info table of exactly max_labels entries, and the refusals that must come
    before the first point is read.  Any report fails."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = shutil.which("clang++") or shutil.which("g++")
    if clang is None:
        pytest.skip("no host C++ compiler with sanitizers")
    csrc = os.path.join(ROOT, "haf_grasping_amd", "csrc")
    exe = str(tmp_path / "cell_paths")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-ffp-contract=off"]
    cmd = [clang] + flags + [os.path.join(csrc, f) for f in ("cellsegment_host.cpp", "segment_host.cpp", "frames_host.cpp", "parsers.cpp")] + \
          [os.path.join(ROOT, "tests", "sanitize", "cell_paths.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "cell segment sanitizer job ok" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
        (r.returncode, r.stdout[-500:], r.stderr[-3000:])
