"""The host definition of record of the best grasp per instance label (include/hafgrasp.h: haf_label_best_ref): no device, no engine.
Against the numpy expectation of label_cases.py built on grasp_map_cases.mirror_map with the CPU oracle's roll transforms and vote
grids of table1 at C3; the layouts of haf_label_image and haf_label_pick against the C compiler; the exports; every refusal.  Every
comparison is an equality.  The engine call needs a GPU: tests/test_labels_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_cases as fc
import grasp_map_cases as gm
import label_cases as lc
import pcdio
from haf_grasping_amd import capi
from oracle import oracle as O
from test_engine_gpu import oracle_input
from test_frames_gpu import C3_CFG, C3_IN, K525, TABLE1
from test_grasp_map_cpu import scene_frames
from test_views_gpu import CAM_A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 56
NEW_NAMES = {"haf_label_best_ref", "haf_grasp_map_labels"}


@pytest.fixture(scope="module")
def table1(data_dir):
    return pcdio.load_pcd(os.path.join(data_dir, TABLE1 + ".pcd"))


@pytest.fixture(scope="module")
def scene(data_dir, golden_dir, table1):
    """table1 at C3 (56 x 56, 20 rolls of 9 degrees) as the CPU oracle scores it"""
    orc = O.Oracle(os.path.join(data_dir, "Features.txt"), os.path.join(data_dir, "range21062012_allfeatures"),
                   os.path.join(golden_dir, "surrogate.model"))
    return orc.run(table1, O.make_cfg(**C3_CFG), oracle_input(C3_IN))


@pytest.fixture(scope="module")
def cam_a(table1, scene):
    """the 640 x 480 U16 frame of CAM_A with its mirror map on the oracle's transforms and grids -> (frame, vote, roll, cell)"""
    _, frame, img = scene_frames(table1)[1]
    assert frame.kind == capi.FRAME_DEPTH_U16 and (frame.width, frame.height) == (640, 480)
    vote, roll, cell = gm.mirror_map(scene["M"], scene["graspseval"], 0, fc.mirror_points(frame, img), H, W)
    return frame, vote.reshape(480, 640), roll.reshape(480, 640), cell.reshape(480, 640)


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    return cc or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")


@pytest.mark.parametrize("ctype,cls,fields,size", [
    ("haf_label_image", capi.LabelImage, ["data", "elem_bytes", "on_device", "row_stride_bytes"], 24),
    ("haf_label_pick", capi.LabelPick, ["found", "u", "v", "vote", "roll", "cell", "n_pixels"], 28)])
def test_label_struct_layouts_match_the_c_compiler(tmp_path, ctype, cls, fields, size):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hafgrasp.h"\nint main(void) {\n printf("%%zu", sizeof(%s));\n' % ctype +
                   "".join(' printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f) for f in fields) + ' printf(" %d\\n", HAF_MAX_LABELS);\n return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call([_cc(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(cls)] + [cls.__dict__[f].offset for f in fields] + [capi.MAX_LABELS]
    assert C.sizeof(cls) == size                                             # (LP64)
    if cls is capi.LabelPick:
        assert capi.LABEL_PICK_DTYPE.itemsize == size and [capi.LABEL_PICK_DTYPE.fields[f][1] for f in fields] == [cls.__dict__[f].offset for f in fields]


def test_label_names_exported_by_both_libraries():
    with open(os.path.join(ROOT, "include", "hafgrasp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert NEW_NAMES <= set(re.findall(r"\b(haf_[a-z_0-9]+)\s*\(", text))
    assert "#define HAF_ABI_VERSION 2" in text and "#define HAF_MAX_LABELS 4096" in text
    for L in (capi.lib(), capi.testlib()):
        for name in NEW_NAMES:
            assert hasattr(L, name), name
        assert L.haf_abi_version() == 2


def test_label_best_ref_equals_the_numpy_expectation(scene, cam_a):
    """haf_label_best_ref on the oracle's grids == key_argmax per label on the mirror map, every field of every pick and the order:
    blocks80 as uint8 and as uint16 in a padded view, interleave(7), out-of-range labels, an all-zero image, one label against the plain
    mask, min_vote at 1, 71 and one above the map's maximum."""
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    frame, vote, roll, cell = cam_a
    top = int(vote.max())
    ref = lambda labels, n=None, mv=1: capi.label_best_ref(cfg, inp, 0, scene["graspseval"], frame, labels, n_labels=n, min_vote=mv)
    b80 = lc.blocks80()
    found = {}
    for mv in (1, 71, top + 1):
        want = lc.expect(vote, roll, cell, b80, 48, mv)
        got = ref(b80, mv=mv)
        lc.assert_picks_equal(got, want, "blocks80 uint8 min_vote %d" % mv)
        lc.assert_picks_equal(ref(lc.padded_view(b80.astype(np.uint16), 5), mv=mv), want, "blocks80 uint16 padded min_vote %d" % mv)
        found[mv] = len(got["order"])
    picks, order = lc.expect(vote, roll, cell, b80, 48, 1)
    no_cell = sum(1 for l in range(1, 49) if not (roll[b80 == l] >= 0).any())
    tops = sorted(int(picks["vote"][l - 1]) for l in order)
    print("blocks80: found", found, "labels without a cell", no_cell, "top votes", tops[::-1])
    # measured with haf_grasp_map_ref on the oracle grids, CAM_A: 18 of 48 found at min_vote 1, 7 at 71, 23 labels without a cell
    assert found[1] >= 15 and 48 - found[1] >= 20 and found[71] >= 1 and found[71] < found[1] and found[top + 1] == 0
    assert no_cell >= 20
    assert len(set(tops)) < len(tops)                                        # two found labels share a top vote: the order's tie-break decides
    assert int(picks["n_pixels"].sum()) == int(((roll >= 0) & (vote >= 1)).sum())
    # neighbouring pixels with different labels
    i7 = lc.interleave(7)
    want = lc.expect(vote, roll, cell, i7, 7, 1)
    lc.assert_picks_equal(ref(i7), want, "interleave(7)")
    assert len(want[1]) == 7
    # labels above n_labels are ignored like background, 65535 included
    odd = lc.interleave(7)
    odd[100:300, 200:400] = 65535
    odd[0:200, 0:100] = 6
    want = lc.expect(vote, roll, cell, odd, 5, 1)
    lc.assert_picks_equal(ref(odd, n=5), want, "labels above n_labels")
    assert int(want[0]["n_pixels"].sum()) < int(((roll >= 0) & (vote >= 1)).sum())
    # nothing labelled
    zero = np.zeros((480, 640), np.uint8)
    got = ref(zero, n=3)
    lc.assert_picks_equal(got, lc.expect(vote, roll, cell, zero, 3, 1), "all zero")
    assert got["order"] == [] and (got["picks"]["found"] == 0).all() and (got["picks"]["vote"] == gm.NO_CELL).all() and (got["picks"]["u"] == -1).all()
    got = ref(zero)                                                          # n_labels left to its default: one label, not found
    assert got["order"] == [] and len(got["picks"]) == 1 and got["picks"]["found"][0] == 0
    # one label: the plain mask of haf_grasp_map_best
    rect = np.zeros((480, 640), np.uint8)
    rect[100:300, 200:500] = 1
    got = ref(rect, n=1)
    u, v = gm.key_argmax(vote, roll, rect, 1)
    p = got["picks"][0]
    assert (p["found"], p["u"], p["v"], p["vote"], p["roll"], p["cell"]) == (1, u, v, vote[v, u], roll[v, u], cell[v, u]) and got["order"] == [1]
    assert p["n_pixels"] == ((roll >= 0) & (vote >= 1) & (rect != 0)).sum()
    # order and n_found may be left out; a roll sub-range answers with global roll indices
    L = capi.lib()
    img, n = capi.label_image(b80, frame)
    only = np.zeros(48, capi.LABEL_PICK_DTYPE)
    assert L.haf_label_best_ref(C.byref(cfg), C.byref(inp), 0, 20, scene["graspseval"].ctypes.data, C.byref(frame), C.byref(img), n, 1,
                                only.ctypes.data, None, None) == capi.HAF_OK
    assert (only == lc.expect(vote, roll, cell, b80, 48, 1)[0]).all()
    sub = gm.mirror_map(scene["M"][5:12], scene["graspseval"][5:12], 5, fc.mirror_points(frame, scene_frames_image(frame)), H, W)
    got = capi.label_best_ref(cfg, inp, 5, scene["graspseval"][5:12], frame, b80)
    lc.assert_picks_equal(got, lc.expect(*[a.reshape(480, 640) for a in sub], b80, 48, 1), "rolls 5..11")
    assert set(got["picks"]["roll"][got["picks"]["found"] == 1]) <= set(range(5, 12))


def scene_frames_image(frame):
    """the pixels of a host U16 frame with packed rows, read back through its pointer"""
    assert frame.row_stride_bytes == frame.width * 2
    return np.frombuffer(C.string_at(frame.data, frame.width * frame.height * 2), np.uint16).reshape(frame.height, frame.width)


def test_interleave_4096_fills_nearly_every_label(scene, cam_a):
    """HAF_MAX_LABELS labels, each spread over the whole image: measured 3 989 of 4 096 found"""
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    frame, vote, roll, cell = cam_a
    labels = lc.interleave(4096)
    want = lc.expect(vote, roll, cell, labels, 4096, 1)
    got = capi.label_best_ref(cfg, inp, 0, scene["graspseval"], frame, labels)
    lc.assert_picks_equal(got, want, "interleave(4096)")
    print("interleave(4096): found", len(want[1]))
    assert len(want[1]) >= 3500 and len(got["picks"]) == 4096


def test_small_and_odd_frames(table1, scene, cam_a):
    """a 1 x 1 frame, 13 x 7 frames of every kind around the map's best pixel, and the golden scene's F32 and XYZ frames with padded rows,
    each with labels that change from pixel to pixel"""
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    frames = {name: (frame, img) for name, frame, img in scene_frames(table1)}
    bu, bv = gm.key_argmax(cam_a[1], cam_a[2], None, 1)
    small = lc.small_frames(scene_frames_image(cam_a[0]), CAM_A, min(max(bu - 6, 0), 640 - 13), min(max(bv - 3, 0), 480 - 7))
    hits = {}
    for name, frame, img in [("u16_single_pixel",) + frames["u16_single_pixel"], ("f32_cam_b_padded",) + frames["f32_cam_b_padded"],
                             ("xyz_padded",) + frames["xyz_padded"]] + small:
        h, w = frame.height, frame.width
        vote, roll, cell = (a.reshape(h, w) for a in gm.mirror_map(scene["M"], scene["graspseval"], 0, fc.mirror_points(frame, img), H, W))
        for dtype in (np.uint8, np.uint16):
            labels = lc.interleave(5, w, h).astype(dtype)
            for mv in (1, -100):
                want = lc.expect(vote, roll, cell, labels, 5, mv)
                lc.assert_picks_equal(capi.label_best_ref(cfg, inp, 0, scene["graspseval"], frame, labels, n_labels=5, min_vote=mv), want, (name, dtype, mv))
                hits[name] = hits.get(name, 0) + len(want[1])
    print(hits)
    assert hits["u16_single_pixel"] >= 2 and all(hits[n] >= 10 for n, _, _ in small) and hits["f32_cam_b_padded"] == 20 and hits["xyz_padded"] == 20


def test_label_best_ref_refuses_what_it_must():
    """Every HAF_E_ARG / HAF_E_CAPACITY case; a refused call writes nothing"""
    L = capi.lib()
    A, CAP = capi.HAF_E_ARG, capi.HAF_E_CAPACITY
    cfg, inp = capi.default_config(**C3_CFG), capi.default_input(**C3_IN)
    grids = np.zeros((cfg.n_rolls, H, W), np.float32)
    good = capi.depth_frame(np.full((3, 4), 900, np.uint16), **K525)
    lab16 = np.ones((3, 8), np.uint16)
    picks = np.full(8, 7, capi.LABEL_PICK_DTYPE)
    order, nf = np.full(8, 7, np.int32), C.c_int32(7)

    def image(data=lab16.ctypes.data, eb=2, dev=0, stride=16):
        return capi.LabelImage(data, eb, dev, stride)

    def ref(cfg_=cfg, inp_=inp, first=0, count=cfg.n_rolls, g=grids.ctypes.data, frame=good, img=image(), n=4, out=picks.ctypes.data):
        return L.haf_label_best_ref(C.byref(cfg_) if cfg_ else None, C.byref(inp_) if inp_ else None, first, count, g,
                                    C.byref(frame) if frame else None, C.byref(img) if img else None, n, 1, out, order.ctypes.data, C.byref(nf))
    assert ref() == capi.HAF_OK and (picks["found"][:4] == 0).all() and nf.value == 0 and (picks["found"][4:] == 7).all()
    assert ref(count=0, g=None) == capi.HAF_OK
    assert ref(img=image(eb=1, stride=4)) == capi.HAF_OK and ref(img=image(stride=8)) == capi.HAF_OK and ref(n=capi.MAX_LABELS, out=np.zeros(4096, capi.LABEL_PICK_DTYPE).ctypes.data) == capi.HAF_OK
    picks[:], order[:], nf.value = 7, 7, 7
    dev = capi.Frame.from_buffer_copy(good)
    dev.on_device = 1
    for kw in (dict(cfg_=None), dict(inp_=None), dict(frame=None), dict(g=None), dict(first=-1), dict(count=-1), dict(first=1), dict(count=cfg.n_rolls + 1),
               dict(cfg_=capi.default_config(grid_h=0)), dict(frame=dev),
               dict(img=None), dict(img=image(data=None)), dict(out=None), dict(img=image(eb=0)), dict(img=image(eb=3)), dict(img=image(eb=4)),
               dict(img=image(stride=6)), dict(img=image(stride=9)), dict(img=image(eb=1, stride=3)), dict(img=image(data=lab16.ctypes.data + 1)),
               dict(img=image(dev=1)), dict(img=image(dev=2)), dict(img=image(dev=-1)), dict(n=0), dict(n=-1), dict(n=capi.MAX_LABELS + 1)):
        assert ref(**kw) == A, kw
    seen = set()
    for name, frame, code, _ in fc.refusal_frames():
        assert ref(frame=frame) == code, name
        seen.add(code)
    assert seen == {A, CAP}
    assert all((picks[f] == 7).all() for f in lc.FIELDS) and (order == 7).all() and nf.value == 7
