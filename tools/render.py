"""The synthetic pinhole camera of the latency tools (frame_latency.py, view_latency.py): a 16-bit depth image rendered from a cloud."""
import numpy as np


def tilted_pose(angles, position):
    """sensor_to_base (3 x 4, row-major, float32) of a camera at `position` that looks straight down and is then rotated about the
    base frame's x, y, z axes by `angles` (rad)"""
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    rot = rz @ ry @ rx @ np.diag([1.0, -1.0, -1.0])
    return np.concatenate([rot, np.asarray(position, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(-1)


def render_depth(xyz, s2b, w, h, fx, fy, cx, cy):
    """nearest depth per pixel, millimetres as uint16 (0 = nothing seen), of a pinhole camera at sensor_to_base s2b"""
    m = np.asarray(s2b, np.float64).reshape(3, 4)
    pc = (np.asarray(xyz, np.float64) - m[:, 3]) @ m[:, :3]
    pc = pc[np.isfinite(pc).all(axis=1) & (pc[:, 2] > 0.05)]
    u = np.rint(fx * pc[:, 0] / pc[:, 2] + cx).astype(np.int64)
    v = np.rint(fy * pc[:, 1] / pc[:, 2] + cy).astype(np.int64)
    mm = np.rint(pc[:, 2] * 1000.0).astype(np.int64)
    ok = (u >= 0) & (u < w) & (v >= 0) & (v < h) & (mm > 0) & (mm < 65536)
    img = np.full(w * h, 65536, np.int64)
    np.minimum.at(img, v[ok] * w + u[ok], mm[ok])
    img[img == 65536] = 0
    return img.astype(np.uint16).reshape(h, w)
