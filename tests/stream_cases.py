"""Shared by tests/test_streams_gpu.py (haf_set_stream / haf_get_stream, the stream contract of include/hafgrasp.h): the detector that
makes a wrong stream visible, and the one small scene every row of the table runs on.

Every call synchronises before it returns, so equal results prove nothing about streams.  The detector does:

  late input    a device-resident input starts as synchronised ZEROS.  On the caller's stream the test enqueues a delay and, behind it, the
                copy of the real content from pinned memory, then the event `late`; the call is issued at once.  Work on any other
                stream runs during the delay and reads zeros -- for a frame: every pixel unusable, a case the suite feeds every call --
                and the result differs from the expected one.
  late poison   a caller-owned device output starts as synchronised filler; a fill with POISON goes behind the same delay.  A write on
                any other stream lands during the delay and is overwritten by the poison.

Neither can fail a correct engine: work ordered on the caller's stream runs behind the copies and the fills.  `late` must not have
happened just before the call (else the case proves nothing: it FAILS, it is never skipped or retried) and must have happened when the
call returns.

The scene is object_cases': 160 x 120 pixels, 19 200 points, 75 blocks of 256 -- the smallest the suite has on which binning, the ROI
marking and the label passes span several workgroups."""
import ctypes as C
import functools

import numpy as np

import clearance_cases as cc
import object_cases as oc
import plane_cases as pc
import transfer_cases as tc
from haf_grasping_amd import capi

# The delay behind which late inputs and poison are enqueued, in milliseconds.  profiles/stream_delay.json: every call of the table on
# this scene, timed on an MI355X at the commit before the stream contract with the engine on its own stream, takes 0.05 - 0.55 ms
# (haf_score_objects is the slowest; 1.27 ms on its first call, with the first-use allocations); 2 000 000 cycles of
# torch.cuda._sleep took 0.853 ms there, 93.8 M cycles 39.2 ms.  The rule: at least ten times the slowest call and at least 20 ms, so
# that a wrongly streamed call ends well inside the delay; at most 200 ms, so that nothing looks like a hang.  40 ms is 73 times the
# slowest call and 31 times the slowest first call.  The cycle count is calibrated by every run (calibrate_sleep).
MEASURED_SLOWEST_MS = 1.27
DELAY_MS = 40.0
assert 20.0 <= DELAY_MS <= 200.0 and DELAY_MS >= 10.0 * MEASURED_SLOWEST_MS
POISON = 0xEE
FILLER = 0x11
PX = oc.W * oc.H
ENGINE_KW = dict(max_points=3 * PX, max_clouds=8, grid_h=oc.GRID, grid_w=oc.GRID, **oc.CFG_KW)
MODES = ("torch", "null", "own")


def calibrate_sleep(torch, stream):
    """torch.cuda._sleep counts cycles of a clock nobody promises: time a fixed count between two events on `stream` and scale it
    -> (cycles for DELAY_MS, dict of what was measured)"""
    probe = 2_000_000
    torch.cuda._sleep(1000)                               # (the kernel's first launch loads it)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        torch.cuda._sleep(probe)
        b.record()
    b.synchronize()
    probe_ms = a.elapsed_time(b)
    assert probe_ms > 0.05, probe_ms
    cycles = int(probe * DELAY_MS / probe_ms)
    with torch.cuda.stream(stream):
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
    b.synchronize()
    got_ms = a.elapsed_time(b)
    assert 0.9 * DELAY_MS <= got_ms <= 200.0, (probe_ms, cycles, got_ms)
    return cycles, dict(probe_cycles=probe, probe_ms=probe_ms, cycles=cycles, delay_ms=got_ms)


class Late:
    """One armed call.  Register the device-resident inputs and the caller-owned device outputs first (they are allocated, zeroed or
    filled, and synchronised), then run the call inside `with late:`.

    stream   the torch stream that is the engine's current stream (modes "torch" and "null"): delay, copies and fills go there;
    joined   mode "own": the engine runs on its own stream, which the test cannot enqueue on.  The delay, the copies and the fills go to
             `stream`, which is then joined the documented old way -- the engine's stream waits for it (wait_stream) and the host
             synchronises it once -- before the call;
    control  the control test: the engine is on ANOTHER stream on purpose, so the call is not expected to wait for `late`."""
    host = False

    def __init__(self, torch, stream, cycles, joined=None, control=False):
        self.torch, self.stream, self.cycles, self.joined, self.control = torch, stream, cycles, joined, control
        self.inputs, self.outputs, self.late = [], [], None

    # ---- inputs ----
    def span(self, host_bytes, offset=0):
        """host bytes -> the address of as many device bytes, `offset` bytes past a 256-byte boundary, zero until the late copy"""
        t = self.torch
        host = np.zeros(offset + len(host_bytes) + 16, np.uint8)
        host[offset:offset + len(host_bytes)] = host_bytes
        pinned = t.from_numpy(host).pin_memory()
        dev = t.zeros(len(host), dtype=t.uint8, device="cuda")
        self.inputs.append((dev, pinned))
        return dev.data_ptr() + offset

    def frame(self, frame, image):
        """the frame's pixels late in device memory: the same address modulo 16, rows and points as far apart as on the host"""
        last = 12 if frame.kind == capi.FRAME_XYZ_F32 else image.itemsize
        elem = frame.point_stride_bytes if frame.kind == capi.FRAME_XYZ_F32 else image.itemsize
        n = (frame.height - 1) * frame.row_stride_bytes + (frame.width - 1) * elem + last
        g = capi.Frame.from_buffer_copy(frame)
        g.data, g.on_device = self.span(np.frombuffer(C.string_at(frame.data, n), np.uint8), frame.data % 16), 1
        return g

    def rows(self, array):
        """a host image [height, width] of 1- or 2-byte elements (rows may be padded) late on the device -> (pointer, row stride in bytes)"""
        stride = array.strides[0] if array.shape[0] > 1 else array.shape[1] * array.itemsize
        n = (array.shape[0] - 1) * stride + array.shape[1] * array.itemsize
        return self.span(np.frombuffer(C.string_at(array.ctypes.data, n), np.uint8), 2 * array.itemsize), stride

    def labels(self, array):
        ptr, stride = self.rows(array)
        return capi.LabelImage(ptr, array.itemsize, 1, stride)

    def cloud(self, xyz):
        """float32 [n, stride] -> the (pointer, n, stride) tuple Engine.score takes for a device-resident cloud"""
        a = np.ascontiguousarray(xyz, np.float32)
        return (self.span(a.view(np.uint8).reshape(-1)), a.shape[0], a.shape[1])

    # ---- outputs ----
    def output(self, nbytes, offset=0):
        """a caller-owned device buffer of nbytes, filled with FILLER now and with POISON late -> its address"""
        t = self.torch
        dev = t.full((offset + nbytes + 16,), FILLER, dtype=t.uint8, device="cuda")
        self.outputs.append((dev, offset, nbytes))
        return dev.data_ptr() + offset

    def alias(self, ptr, nbytes):
        """the engine's own device image at `ptr` as an output of this call: poisoned late like a caller's"""
        class Raw:
            __cuda_array_interface__ = dict(shape=(nbytes,), typestr="|u1", data=(int(ptr), False), version=2)
        self.outputs.append((self.torch.as_tensor(Raw(), device="cuda"), 0, nbytes))

    def read(self, k):
        """output k after the call -> uint8 [nbytes]; everything of the buffer around it must still be poison"""
        dev, offset, nbytes = self.outputs[k]
        whole = dev.cpu().numpy()
        if len(whole) > nbytes:
            assert (whole[:offset] == POISON).all() and (whole[offset + nbytes:] == POISON).all(), "a write outside the output"
        return whole[offset:offset + nbytes]

    # ---- the call ----
    def __enter__(self):
        t = self.torch
        t.cuda.synchronize()                              # zeros and filler are in place, nothing else is running
        self.late = t.cuda.Event()
        with t.cuda.stream(self.stream):
            t.cuda._sleep(self.cycles)
            for dev, pinned in self.inputs:
                dev.copy_(pinned, non_blocking=True)
            for dev, _, _ in self.outputs:
                dev.fill_(POISON)
            self.late.record()
        if self.joined is not None:
            self.joined.wait_stream(self.stream)
            self.stream.synchronize()
        else:
            assert not self.late.query(), "the delay ended before the call was issued: the case would prove nothing"
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None and not self.control:
                assert self.late.query(), "the call returned before the work enqueued in front of it on its stream"
        finally:
            self.stream.synchronize()                     # nothing of this call's is freed while the stream still uses it
        return False


# ---- the scene ------------------------------------------------------------------------------------------------------------------------

SEGMENT_KW = dict(plane=[0.0, 0.0, 1.0, 0.0], min_height=0.03, max_gap=0.02, min_pixels=50, max_labels=255)
CELL_KW = dict(plane=[0.0, 0.0, 1.0, 0.0], min_height=0.03, cell=0.01, x0=-0.64, y0=-0.48, nx=128, ny=96, min_points=50, max_labels=255)
N_GRASPS = 65


def exposure_stack():
    """three u16 exposures of the scene, rows padded: the scene's own depth, and two with a millimetre of noise and other dropouts"""
    rng = np.random.default_rng(20260101)
    z = oc.scene_z()
    out = [pc.depth_frame_of(z, "u16", oc.POSE, 3)]
    for _ in range(2):
        zk = z + rng.uniform(-0.001, 0.001, z.shape)
        zk.reshape(-1)[rng.random(PX) < 0.03] = np.nan
        out.append(pc.depth_frame_of(zk, "u16", oc.POSE, 3))
    return out


@functools.lru_cache(maxsize=None)
def scene():
    """everything the rows share, built once: the frames of all three kinds with padded rows, the label image and the masks with padded
    rows, the requests, the grasps, the exposures, the transfer case, and the expectations that are host definitions"""
    s = dict(frames={k: oc.frame_of(k, pad) for k, pad in (("u16", 3), ("f32", 5), ("xyz", 2))})
    frame, image = s["frames"]["u16"]
    labels = pc.padded_mask(oc.labels_u8(), 5)
    s["labels"] = labels
    s["labels16"] = np.ascontiguousarray(labels).astype(np.uint16)
    s["inputs"] = oc.object_inputs(frame, np.ascontiguousarray(labels))
    s["masks"] = {l: pc.padded_mask((labels == l).astype(np.uint8), 3) for l in oc.OBJECT_LABELS}
    s["mask_any"] = pc.padded_mask((labels != 0).astype(np.uint8), 7)
    pts = capi.frame_points(frame)
    pts = pts[np.isfinite(pts).all(axis=1)]
    s["points"] = pts
    cloud = np.zeros((len(pts), 4), np.float32)
    cloud[:, :3] = pts
    s["clouds"] = [cloud, np.ascontiguousarray(cloud[::2, :3])]
    rng = np.random.default_rng(20260102)
    s["grasps"] = cc.random_grasps(rng, cc.base_points(frame, image), N_GRASPS)
    s["exposures"] = exposure_stack()
    # host definitions
    s["filtered"], s["filter_stats"] = capi.filter_depth_ref([f for f, _ in s["exposures"]])
    s["segment"] = capi.segment_ref(frame, capi.segment_params(**SEGMENT_KW))
    s["cells"] = capi.segment_cells_ref(frame, capi.cell_segment_params(**CELL_KW))
    s["plane"] = capi.fit_plane_ref(frame, None, s["mask_any"], debug=True)
    s["plane_all"] = capi.fit_plane_ref(frame, None, None, debug=True)
    s["shapes"] = capi.measure_labels_ref(frame, np.ascontiguousarray(labels), oc.N_LABELS, [0.0, 0.0, 1.0, 0.0])
    s["clearance"] = capi.check_grasps_ref(frame, s["grasps"], None, s["mask_any"])
    assert len(s["segment"][1]) >= 2 and len(s["cells"][1]) >= 2 and s["plane"]["found"] and s["plane_all"]["found"]
    assert s["shapes"]["found"].sum() >= 5 and 0 < len(s["clearance"][1]) < N_GRASPS
    # haf_transfer_labels: the smallest size case whose expected image is not all background (a late input must be able to change it)
    for case in tc.size_cases():
        name, tframe, timage, cam, cam_labels, n_labels, kw = case
        want = capi.transfer_labels_ref(tframe, cam, cam_labels, n_labels, capi.transfer_params(**kw), dtype=np.uint8)
        if want[0].any():
            s["transfer"], s["transfer_want"] = case, want
            break
    return s


def zero_frame_results():
    """what haf_segment_frame and haf_check_grasps return for the scene's frame with every pixel zero (unusable): the control test's
    wrongly streamed engine must return exactly this"""
    s = scene()
    frame, image = s["frames"]["u16"]
    zero = np.zeros_like(np.ascontiguousarray(image))
    zf = capi.depth_frame(zero, frame.fx, frame.fy, frame.cx, frame.cy, sensor_to_base=list(frame.sensor_to_base))
    return capi.segment_ref(zf, capi.segment_params(**SEGMENT_KW)), capi.check_grasps_ref(zf, s["grasps"])
