"""CPU test of the sensor-frame staging code that needs no device (csrc/frame_stage.h): the host sanitizer job of pack_rows, unpack_rows,
stage_rows, describe_frame, staged_bytes, describe_image, describe_output, image_span / frame_span / spans_overlap, load_label /
store_label, check_label_image, check_output_image, check_label_output and check_frame_batch; and the one table of malformed label
images through every host reader of one.  The wiring into the engine needs a GPU: tests/test_frame_stage_gpu.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frame_cases as fc
from haf_grasping_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = dict(fx=525.0, fy=525.0, cx=30.0, cy=2.0)


def malformed_label_images(width, height):
    """-> (list of (name, LabelImage, n_labels) that check_label_image must refuse for an image `width` x `height`, the arrays they point
    into): null data, elem_bytes 0 / 3 / 4, on_device 2 / -1, a stride one byte short for uint8 and uint16, an odd stride for uint16, uint16
    data at an odd address, n_labels 0 and HAF_MAX_LABELS + 1"""
    lab8, lab16 = np.ones((height, width + 8), np.uint8), np.ones((height + 1, width + 8), np.uint16)
    s8, s16 = lab8.strides[0], lab16.strides[0]
    img = lambda data=lab16.ctypes.data, eb=2, dev=0, stride=s16: capi.LabelImage(data, eb, dev, stride)
    out = [("null_data", img(data=None), 3)]
    out += [("elem_bytes_%d" % eb, img(eb=eb), 3) for eb in (0, 3, 4)]
    out += [("on_device_%d" % dev, img(dev=dev), 3) for dev in (2, -1)]
    out += [("u8_stride_short", img(data=lab8.ctypes.data, eb=1, stride=width - 1), 3), ("u16_stride_short", img(stride=2 * width - 1), 3),
            ("u16_stride_odd", img(stride=2 * width + 1), 3), ("u16_data_odd", img(data=lab16.ctypes.data + 1), 3),
            ("n_labels_0", img(), 0), ("n_labels_above", img(), capi.MAX_LABELS + 1)]
    return out, (lab8, lab16)


def test_one_table_of_malformed_label_images_through_every_host_reader():
    """haf_label_best_ref, haf_measure_labels_ref and haf_transfer_labels_ref each refuse every entry of malformed_label_images() with
    HAF_E_ARG and leave their outputs' canary bytes.  The frame is 61 x 5; transfer's camera is 7 x 3, so its label image is checked
    against the CAMERA's width: one of exactly 7 elements a row is accepted (the depth frame's width would refuse it), and with the two
    shapes exchanged one of 7 elements a row is refused (the depth frame's width would accept it)."""
    L, A = capi.lib(), capi.HAF_E_ARG
    frame = capi.depth_frame(np.full((5, 61), 900, np.uint16), **K)
    small = capi.depth_frame(np.full((3, 7), 900, np.uint16), **K)
    cfg, inp = capi.default_config(n_rolls=2), capi.default_input()
    grids = np.zeros((cfg.n_rolls, cfg.grid_h, cfg.grid_w), np.float32)
    picks, order, nf = np.full(8, 7, capi.LABEL_PICK_DTYPE), np.full(8, 7, np.int32), C.c_int32(7)
    shapes = np.full(8 * capi.LABEL_SHAPE_DTYPE.itemsize, 0x77, np.uint8)
    canvas, zb = np.full((5, 80), 0x77, np.uint8), np.full((5, 61), -7, np.int32)
    p = capi.transfer_params()

    def best(img, n):
        return L.haf_label_best_ref(C.byref(cfg), C.byref(inp), 0, cfg.n_rolls, grids.ctypes.data, C.byref(frame), C.byref(img), n, 1,
                                    picks.ctypes.data, order.ctypes.data, C.byref(nf))

    def measure(img, n):
        return L.haf_measure_labels_ref(C.byref(frame), C.byref(img), n, None, shapes.ctypes.data)

    def transfer(img, n, depth=frame, cam=capi.camera(7, 3, 5.0, 5.0, 3.0, 1.0)):
        st = (C.c_int64 * 5)(*[-7] * 5)
        rc = L.haf_transfer_labels_ref(C.byref(depth), C.byref(cam), C.byref(img), n, C.byref(p), canvas.ctypes.data, 1, 80, zb.ctypes.data, st)
        assert rc != capi.HAF_OK or list(st) != [-7] * 5
        assert rc == capi.HAF_OK or list(st) == [-7] * 5
        return rc

    def untouched():
        return all((picks[f] == 7).all() for f in picks.dtype.names) and (order == 7).all() and nf.value == 7 and (shapes == 0x77).all() and \
            (canvas == 0x77).all() and (zb == -7).all()

    wide, keep_wide = malformed_label_images(61, 5)
    narrow, keep_narrow = malformed_label_images(7, 3)
    assert len(wide) == len(narrow) == 12
    for name, img, n in wide:
        assert best(img, n) == A and measure(img, n) == A, name
    for name, img, n in narrow:
        assert transfer(img, n) == A, name
    assert untouched()
    # the camera's width, in both directions
    for dtype in (np.uint8, np.uint16):
        eb = np.dtype(dtype).itemsize
        lab7, lab61 = np.ones((5, 7), dtype), np.ones((5, 61), dtype)
        short = capi.LabelImage(lab61.ctypes.data, eb, 0, 7 * eb)                  # 7 elements a row
        assert transfer(short, 3, depth=small, cam=capi.camera(61, 5, 5.0, 5.0, 30.0, 2.0)) == A and untouched()
        assert best(short, 3) == A and measure(short, 3) == A and untouched()
        exact = capi.LabelImage(lab7.ctypes.data, eb, 0, 7 * eb)
        assert transfer(exact, 3) == capi.HAF_OK and not (canvas[:, :61] == 0x77).any() and (canvas[:, 61:] == 0x77).all()
        canvas[:], zb[:] = 0x77, -7
    # the accepted twins of the table's strides: exactly a row
    exact8, exact16 = np.ones((5, 61), np.uint8), np.ones((5, 61), np.uint16)
    for arr in (exact8, exact16):
        img = capi.LabelImage(arr.ctypes.data, arr.itemsize, 0, 61 * arr.itemsize)
        assert best(img, 3) == capi.HAF_OK and measure(img, 3) == capi.HAF_OK


def test_stage_paths_under_address_and_ub_sanitizers(tmp_path):
    """frame_stage.cpp + frames_host.cpp + parsers.cpp built with -fsanitize=address,undefined by the ROCm clang and driven by
    tests/sanitize/stage_paths.cpp as a program of its own: every kind, width 1 / 3 / 61 / 64, height 1 / 5, padded rows, point strides
    12 / 16 / 20 and masks against a byte-by-byte loop in exactly sized heap blocks; unpack_rows of 1 / 2 / 4-byte elements into padded
    targets whose last row ends at its last element and whose bytes between the rows must stay; the pieces of frames around 256 KB against
    the upload loop the code replaced; the descriptors of frames, side images and output images and the LabelImage an output hands back;
    spans_overlap back to back, one byte shared, inside the padding behind a last row, height 1 and an XYZ frame of point stride 20;
    store_label / load_label round trips of 0 / 1 / 255 / 256 / 65535 in exactly sized blocks whose bytes between the rows must stay;
    check_label_image, check_output_image and check_label_output over one accepted case and every refusal; the batch checks over every refusal of frame_cases.refusal_frames().  Any report fails."""
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
