"""CPU tests of haf_score_frames_roi's host side (include/hafgrasp.h): the haf_roi layout, the exports, the numpy mirror of the record
rule pinned to the CPU oracle, haf_roi_cells -- the host definition of record of the ROI cell sets -- against the numpy mirror for every
mask kind on the golden scene's frames, the choice of the C3 rectangle, and the refusals.  Every comparison is an equality.  The engine
path needs a GPU: tests/test_roi_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import pcdio
import roi_cases as rc
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import oracle_input
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1, render_depth
from test_grasp_map_cpu import TILTED_IN, scene_frames
from test_views_gpu import CAM_A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 56
NEW_NAMES = {"haf_roi_cells", "haf_score_frames_roi"}


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


@pytest.fixture(scope="module")
def orc(data_dir, golden_dir):
    return O.Oracle(os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures"),
                    os.path.join(golden_dir, "surrogate.model"))


def test_roi_struct_layout_matches_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    fields = ["mask", "row_stride_bytes", "on_device"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hafgrasp.h"\nint main(void) {\n printf("%zu", sizeof(haf_roi));\n' +
                   "".join(' printf(" %%zu", offsetof(haf_roi, %s));\n' % f for f in fields) + ' printf("\\n");\n return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.Roi)] + [capi.Roi.__dict__[f].offset for f in fields]
    assert C.sizeof(capi.Roi) == 24 and capi.Roi.on_device.offset == 16       # (LP64)


def test_roi_names_exported_by_both_libraries():
    with open(os.path.join(ROOT, "include", "hafgrasp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert NEW_NAMES <= set(re.findall(r"\b(haf_[a-z_0-9]+)\s*\(", text))
    assert "#define HAF_ABI_VERSION 2" in text
    for L in (capi.lib(), capi.testlib()):
        for name in NEW_NAMES:
            assert hasattr(L, name), name
        assert L.haf_abi_version() == 2


def test_record_mirror_reproduces_the_oracle_records(orc, data_dir):
    """The numpy mirror of the record rule (roi_cases.mirror_record) on the unmasked vote grids of an oracle run of pcd2, three rolls:
    the oracle's own (row, col, vote) of every roll.  The GPU suite applies the same mirror to the gated grids."""
    xyz = capi.load_pcd(os.path.join(data_dir, "pcd2.pcd"))
    want = orc.run(xyz, O.make_cfg(n_rolls=3), O.make_input(length_x=32, length_y=32))
    assert want["top"] > 0
    for roll in range(3):
        vote, row, col = rc.mirror_record(want["graspseval"][roll])
        assert [row, col, vote] == [int(v) for v in want["roll_best"][roll]], roll
    # an all-zero grid: the run of zeros of row 0 (what the reference's loop leaves for a roll without a positive vote)
    assert rc.mirror_record(np.zeros((H, W), np.float32)) == (0, 0, W - 1 - W // 2)
    # the first longest run wins, in row-major order; a longer run later beats it
    g = np.zeros((8, 16), np.float32)
    g[2, 3:5], g[5, 1:3], g[6, 9:12] = 9, 9, 9
    assert rc.mirror_record(g) == (9, 6, 11 - 3 // 2)
    g[6, 11] = 0
    assert rc.mirror_record(g) == (9, 2, 4 - 2 // 2)


def test_dilation_is_the_29_taps():
    one = np.zeros((11, 13), bool)
    one[5, 6] = True
    d = rc.dilate(one)
    assert d.sum() == 29 and d[5, 2:11].all() and d[3:8, 4:9].all() and not d[4, 3] and not d[2, 6]
    corner = np.zeros((11, 13), bool)
    corner[0, 0] = True
    assert rc.dilate(corner).sum() == 3 * 3 + 2


@pytest.mark.parametrize("in_kw", [C3_IN, TILTED_IN], ids=["c3", "tilted_width2"])
def test_roi_cells_equal_the_numpy_mirror(table1, in_kw):
    """haf_roi_cells == the mirror (frame_cases.mirror_points -> grasp_map_cases.mirror_cells on the ORACLE's roll transforms -> the
    explicit 29-tap dilation) for the golden scene in every kind (padded rows, 16-byte points, 1 x 1, all-invalid frames), every mask
    kind and three rolls.  The conditions below make the comparison non-vacuous."""
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**in_kw)
    rolls = (0, 7, 19)
    Ms = rc.oracle_transforms(C3_CFG, in_kw, 0, 20)[list(rolls)]
    cells, kinds = {}, 0
    for name, frame, img in scene_frames(table1):
        words = fc.mirror_points(frame, img)
        kinds |= 1 << frame.kind
        for mname, mask in rc.masks(words, frame.height, frame.width):
            S = rc.mirror_roi(Ms, words, mask, H, W)
            E = rc.dilate(S)
            for k, roll in enumerate(rolls):
                got = capi.roi_cells(cfg, inp, roll, frame, mask)
                assert (got["roi"] == S[k]).all(), (name, mname, roll, int((got["roi"] != S[k]).sum()))
                assert (got["eval"] == E[k]).all(), (name, mname, roll)
                assert set(np.unique(got["roi"])) <= {0, 1} and set(np.unique(got["eval"])) <= {0, 1}
            cells[name, mname] = int(S.sum())
            if mname in ("zeros", "invalid_only") or name.endswith("all_invalid"):
                assert S.sum() == 0 and E.sum() == 0, (name, mname)
            only = capi.roi_cells(cfg, inp, 7, frame, mask, want=("eval",))       # either output may be left out
            assert list(only) == ["eval"] and (only["eval"] == E[1]).all()
    assert kinds == 7
    for name in ("table1_xyz", "u16_cam_a", "u16_cam_a_padded", "f32_cam_b_padded", "xyz16_cam_b", "xyz_padded"):
        assert cells[name, "ones"] >= 3 * 1000 and 0 < cells[name, "rect"] < cells[name, "ones"], (name, cells[name, "ones"], cells[name, "rect"])
        assert cells[name, "rect_padded"] == cells[name, "rect"] and 0 < cells[name, "scattered"] <= 3 * 200 and 0 < cells[name, "one_pixel"] <= 3
    assert cells["u16_single_pixel", "ones"] == 3


def test_c3_rectangle_restricts_the_request_and_keeps_a_grasp(orc, table1):
    """The rectangle the GPU suite scores at C3 (roi_cases.C3_RECT on table1 rendered from CAM_A), on the CPU oracle's grids: it selects
    some but fewer than half of the full request's evaluations, its best vote is positive, and that vote is the maximum of the full
    request's grasp map over the masked pixels -- the consequence the header states."""
    da = render_depth(table1, CAM_A)
    fa = capi.depth_frame(da, sensor_to_base=CAM_A, **K525)
    full = orc.run(capi.frame_points(fa), O.make_cfg(**C3_CFG), oracle_input(C3_IN))
    words = fc.mirror_points(fa, da)
    rect = dict(rc.masks(words, 480, 640, rect=rc.C3_RECT))["rect"]
    S = rc.mirror_roi(full["M"], words, rect, H, W)
    E = rc.dilate(S) & (full["mask"] != 0)
    gated = np.where(S, full["graspseval"], 0)
    print("full n_evals %d, ROI cells %d, ROI evaluations %d, best ROI vote %d" % (full["n_evals"], S.sum(), E.sum(), gated.max()))
    assert 0 < E.sum() < full["n_evals"] / 2 and gated.max() > 0
    vote, _, _ = gm.mirror_map(full["M"], full["graspseval"], 0, words, H, W)
    assert gated.max() == vote.reshape(480, 640)[rect != 0].max()
    # what a vote reads lies in E or outside the full request's mask: the gated grid is the vote of the labels restricted to E
    lab = np.where(E, full["labels"], -1)
    assert (lab[E] == full["labels"][E]).all() and ((full["labels"] >= 0) <= (full["mask"] != 0)).all()


def test_roi_cells_refuses_what_it_must():
    L = capi.lib()
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    img = np.full((3, 4), 900, np.uint16)
    good = capi.depth_frame(img, **K525)
    mask = np.ones((3, 4), np.uint8)
    roi, ev = np.full((H, W), 7, np.uint8), np.full((H, W), 7, np.uint8)

    def call(cfg_=cfg, inp_=inp, roll=0, frame=good, m=mask.ctypes.data, stride=4):
        return L.haf_roi_cells(C.byref(cfg_) if cfg_ else None, C.byref(inp_) if inp_ else None, roll, C.byref(frame) if frame else None, m, stride,
                               roi.ctypes.data, ev.ctypes.data)
    assert call() == capi.HAF_OK and set(np.unique(roi)) <= {0, 1} and set(np.unique(ev)) <= {0, 1}
    assert L.haf_roi_cells(C.byref(cfg), C.byref(inp), 0, C.byref(good), mask.ctypes.data, 4, None, None) == capi.HAF_OK
    roi[:], ev[:] = 7, 7
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    for kw in (dict(cfg_=None), dict(inp_=None), dict(frame=None), dict(m=None), dict(roll=-1), dict(roll=cfg.n_rolls), dict(stride=3), dict(stride=0),
               dict(cfg_=capi.default_config(grid_h=0)), dict(cfg_=capi.default_config(grid_w=-3)), dict(cfg_=capi.default_config(n_rolls=0)), dict(frame=dev)):
        assert call(**kw) == A, kw
    seen = set()
    for name, frame, code, _ in fc.refusal_frames():
        assert call(frame=frame) == code, name
        seen.add(code)
    assert seen == {A, CAP}
    assert (roi == 7).all() and (ev == 7).all()
