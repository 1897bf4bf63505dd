"""The statement of the keyframe depth filter (cvo_depth_filter_*) in numpy float32.  The CPU twin
(cvo_depth_filter_accumulate_host / _finish_host) and the kernels of cvo_k_depth.h equal it bit for bit.

It restates the last loops of upstream's driver src/experiments/main_depth_filtering.cpp (208-298): per later frame the
association of the keyframe with the frame under a non-isotropic kernel; for every keyframe row the depth of each associated
point, moved into the keyframe's frame, and its weight a_ij; rows with more than three observations get a weighted mean depth
and are re-projected along their ray, the others are dropped.

A function of: the keyframe's rows; per frame the association as CSR (rows = keyframe rows in original order, columns
ascending, values a) with the frame's ORIGINAL xyz and a 4x4 T_depth (row, col).

State per keyframe row: depth_sum (float32), weight_sum (float32), count (int32), zero at open.
add: for the row's entries j in ascending column order
    zj = T_depth[2,0] x_j + T_depth[2,1] y_j + T_depth[2,2] z_j + T_depth[2,3]   (CvoPointCloud::transform, cvo_pointcloud.cpp:196)
  as three separately rounded products added left to right; then depth_sum += zj * a (the product rounded, then the sum),
  weight_sum += a, count += 1.  Frames in call order: the sums run frame-major, then by ascending target index - the order in
  which upstream's depths[idx1] / weights[idx1] vectors fill and are summed.
finish(min_count): upstream's value is 3 and the comparison is strict, count > min_count.  For such a row, z0 its keyframe z:
    wbar = weight_sum / float32(count);  d = depth_sum + z0 * wbar;  w = weight_sum + wbar;  d = d / w
    xyz' = (xyz / z0) * d per component (a true division, then the product: Eigen's operator/ and operator*)
  features, labels and geometric types copied, rows kept in ascending original index.  Finish does not change the state.

No fused multiply-add anywhere: every numpy operation below is one float32 operation.

Choice where upstream's text pins nothing - THE LIBRARY'S CHOICE: a row whose d or xyz' is not finite (z0 == 0, a zero w) is
dropped and counted in n_nonfinite.  Upstream would add the point with whatever the divisions gave.

Departures from the driver's text:
  * both matrices come from the caller.  The driver derives them itself, T_t2s = T_t^-1 T_s for the association and T_s2t =
    T_s^-1 T_t for the depth, with Eigen's 4x4 float inverse, which nobody can pin here;
  * nearest_neighbors_max truncates a row's entries per frame, as upstream's kernel does (the CSR given here is already cut);
  * geometric types are off in the association, as inner_product_non_isotropic_impl forces.
"""
import numpy as np

F32 = np.float32


class State:
    def __init__(self, n):
        self.depth_sum = np.zeros(n, F32)
        self.weight_sum = np.zeros(n, F32)
        self.count = np.zeros(n, np.int32)

    def copy(self):
        s = State(len(self.count))
        s.depth_sum, s.weight_sum, s.count = self.depth_sum.copy(), self.weight_sum.copy(), self.count.copy()
        return s


def depth_of(T_depth, xyz):
    """zj of every point of a frame: float32[m]."""
    T = np.asarray(T_depth, F32).reshape(4, 4)
    y = np.asarray(xyz, F32).reshape(-1, 3)
    px, py, pz = T[2, 0] * y[:, 0], T[2, 1] * y[:, 1], T[2, 2] * y[:, 2]
    return ((px + py) + pz) + T[2, 3]


def add(state, row_ptr, col, val, target_xyz, T_depth):
    """One frame into the state, in place.  Entry k of every row at once: within a row the sums stay sequential in k."""
    rp = np.asarray(row_ptr, np.int64)
    col, val = np.asarray(col, np.int64), np.asarray(val, F32)
    n = len(state.count)
    assert len(rp) == n + 1 and rp[0] == 0 and np.all(np.diff(rp) >= 0)
    z = depth_of(T_depth, target_xyz)
    lens = np.diff(rp)
    for k in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > k)
        e = rp[rows] + k
        a = val[e]
        with np.errstate(over="ignore", invalid="ignore"):   # (an indefinite kernel's weights can be huge: inf is float32's answer)
            p = (z[col[e]] * a).astype(F32)
            state.depth_sum[rows] = state.depth_sum[rows] + p
            state.weight_sum[rows] = state.weight_sum[rows] + a
        state.count[rows] += 1
    return state


def finish(state, xyz, min_count=3):
    """-> (moved xyz of the kept rows float32[k, 3], kept original indices int64[k], refined depths float32[k], n_nonfinite)."""
    x = np.asarray(xyz, F32).reshape(-1, 3)
    rows = np.flatnonzero(state.count > min_count)
    with np.errstate(all="ignore"):
        ws, ds, z0 = state.weight_sum[rows], state.depth_sum[rows], x[rows, 2]
        wbar = ws / state.count[rows].astype(F32)
        d = ds + z0 * wbar
        w = ws + wbar
        d = d / w
        out = (x[rows] / z0[:, None]) * d[:, None]
    assert out.dtype == F32 and d.dtype == F32
    ok = np.isfinite(d) & np.isfinite(out).all(axis=1)
    return out[ok], rows[ok], d[ok], int((~ok).sum())


def run(xyz, frames, min_count=3):
    """frames: (row_ptr, col, val, target_xyz, T_depth) each -> (state, finish(...))."""
    s = State(len(np.asarray(xyz).reshape(-1, 3)))
    for f in frames:
        add(s, *f)
    return s, finish(s, xyz, min_count)
