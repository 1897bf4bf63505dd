"""Inputs the depth filter's tests share: the driver-like kernels, frames cut from a builder's target cloud, the statement fed
with associations from any source, and the row-class clouds of row_classes.py dressed as keyframe + frames."""
import numpy as np

import np_depthfilter as npd
from unified_cvo_amd import synth


def rot(angle_deg, axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rotated_kernel(scale=6.0):
    """test_non_isotropic_association's kernel, scaled so that clouds of a few hundred points have rows with several entries."""
    Q = rot(25.0, (0.3, 1.0, -0.2))
    return (Q @ np.diag([0.05, 0.12, 0.02]) @ Q.T * scale).astype(np.float32)


def driver_kernel(normal=0.05, depth=2.0):
    """diag(n, n, d), d >> n: main_depth_filtering.cpp:210-213."""
    return np.diag([normal, normal, depth]).astype(np.float32)


def rigid(angle_deg, axis, t):
    T = np.eye(4)
    T[:3, :3] = rot(angle_deg, axis)
    T[:3, 3] = t
    return T.astype(np.float32)


def subset(pc, idx, shift=(0.0, 0.0, 0.0)):
    """Rows idx of a CvoPointCloud, moved by `shift`, as a new CvoPointCloud with the same attributes."""
    r = pc.select(idx)
    r.positions_ = (r.positions_ + np.asarray(shift, np.float32)).astype(np.float32)
    return r


def frames_of(tgt, sizes, seed=0):
    """len(sizes) frames of different sizes cut from `tgt` (seeded row choices, a small shift each) with their two matrices:
    [(cloud, T, T_depth)].  T moves the keyframe towards the frame as the builders' ground truth does; T_depth is another
    rigid motion (the driver's T_s2t is the inverse chain; any finite matrix serves the arithmetic)."""
    rs = np.random.default_rng([seed, 4242])
    n = tgt.num_points()
    out = []
    for k, m in enumerate(sizes):
        idx = np.sort(rs.choice(n, size=min(m, n), replace=False)) if m else np.zeros(0, np.int64)
        pc = subset(tgt, idx, shift=(0.01 * k, -0.015 * k, 0.02 * k))
        T = (synth.gt_motion() @ rigid(0.3 * k, (0.2, 1.0, 0.1), (0.004 * k, 0.0, -0.003 * k))).astype(np.float32)
        Td = rigid(-1.5 - k, (1.0, 0.3, -0.2), (0.02, -0.01 * k, 0.05 + 0.01 * k))
        out.append((pc, T, Td))
    return out


def statement(kf_xyz, frames, assoc, min_count=3):
    """np_depthfilter.run over `frames` = [(cloud, T, T_depth)] with assoc(k, cloud, T) -> (row_ptr, col, val)."""
    s = npd.State(len(kf_xyz))
    for k, (pc, T, Td) in enumerate(frames):
        rp, col, val = assoc(k, pc, T)
        npd.add(s, rp, col, val, pc.device_arrays()[0], Td)
    return s, npd.finish(s, kf_xyz, min_count)
