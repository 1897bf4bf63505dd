"""Inputs of k_irls_eval on which every quantity it forms is exact in binary64, and their integer reference.

Construction: coordinates are multiples of 2^-3 in [-2, 2], pose rotation blocks have entries in {0, +-1/2, +-1} (signed
permutations, and matrices that are neither orthogonal nor symmetric: the kernel needs no orthogonality, and these
tell R from R^T and rows from columns; the permutations are 3-cycles, for the same reason), translations are multiples
of 2^-3 in [-1, 1], weights are 2^-4 .. 2^0.  Scaled
to integers (p8 = 8 p, R2 = 2 R, t8 = 8 t, w16 = 16 w) the formulas of the k_irls_eval header comment become
    e16 = R2_1 p8_1 + 2 t8_1 - R2_2 p8_2 - 2 t8_2                 |e16| <= 2 (3 * 2 * 16 + 16) = 224
    res = w16 |e16|^2                      (res / 2^12)            res <= 16 * 3 * 224^2 < 2^22
    cost term = res^2                      (/ 2^25, the 1/2 included)  < 2^44
    a32 = R2_1^T e16, J[0:3] = 8 a32, J[3:6] = p8_1 x a32   (J / 2^8)  |J| <= 2 * 16 * 1344 < 2^16
    b32 = R2_2^T e16, J[6:9] = -8 b32, J[9:12] = p8_2 x (-b32)
    g term = J res  (/ 2^20) < 2^38,   H term = J J^T  (/ 2^16) < 2^32
Every intermediate of one entry - each product and each partial sum of the dot and cross products - is an integer
multiple of its quantum below 2^44 quanta, so it is a double whatever the order and whether or not a product and a sum
are contracted into one fma.  The sums over entries are exact in every order as long as sum |term| stays below 2^53
quanta per output component: every partial sum of any subset is then a representable integer multiple of the quantum.
exact_edge() returns those sums next to the values, and the tests assert the bound before they compare bits.
"""
import math

import numpy as np

W = 91
COST_SHIFT, G_SHIFT, H_SHIFT = 25, 20, 16
SHIFTS = np.array([COST_SHIFT] + [G_SHIFT] * 12 + [H_SHIFT] * 78)
TRIU = np.triu_indices(12)
EXACT_LIMIT = 1 << 53

# the two 3-cycles: their matrices differ from their transposes in every row, so row 0 is not column 0 (with the
# identity or a transposition in R[0, 0] = +-1 a kernel that read T[4 c] for T[c] would get the same numbers)
_PERMS = [(1, 2, 0), (2, 0, 1)]


def exact_cloud(rs, n):
    """n x 3 float32, multiples of 1/8 in [-2, 2]."""
    return (rs.integers(-16, 17, (n, 3)) / 8.0).astype(np.float32)


def exact_weights(rs, n):
    return np.ldexp(1.0, -rs.integers(0, 5, n)).astype(np.float32)


def signed_permutation(rs):
    R = np.zeros((3, 3))
    R[np.arange(3), _PERMS[rs.integers(0, 2)]] = rs.choice([-1.0, 1.0], 3)
    return R


def half_matrix(rs):
    """Entries in {0, +-1/2, +-1}, full of nonzeros, not symmetric and not orthogonal."""
    while True:
        R = rs.choice([0.0, 0.5, -0.5, 1.0, -1.0], (3, 3), p=[0.2, 0.2, 0.2, 0.2, 0.2])
        if not np.array_equal(R, R.T) and not np.allclose(R @ R.T, np.eye(3)) and np.count_nonzero(R) >= 6 and \
                not np.array_equal(np.abs(R), np.abs(R.T)):
            return R


def exact_pose(rs, kind):
    R = signed_permutation(rs) if kind == "perm" else half_matrix(rs)
    t = rs.integers(-8, 9, 3) / 8.0
    return np.hstack([R, t[:, None]]).reshape(12)


def exact_poses(rs, F):
    """F poses, alternating the two rotation kinds (the first a half matrix)."""
    return np.stack([exact_pose(rs, "half" if f % 2 == 0 else "perm") for f in range(F)])


def entries(rs, n1, n2, slots, empty="none"):
    """(r, c, w) of `slots` entry slots.  empty: 'none', 'all' or 'interleaved' (about 40 % of the slots empty, between
    stored ones; an empty slot is c = -1, and half of them keep a valid row and a weight - only c < 0 says empty)."""
    r = rs.integers(0, n1, slots).astype(np.int32)
    c = rs.integers(0, n2, slots).astype(np.int32)
    w = exact_weights(rs, slots)
    if empty == "all":
        gone = np.ones(slots, bool)
    elif empty == "interleaved":
        gone = rs.random(slots) < 0.4
    else:
        gone = np.zeros(slots, bool)
    c[gone] = -1
    blank = gone & (rs.random(slots) < 0.5)
    r[blank], w[blank] = -1, 0.0
    return r, c, w


class Table:
    """A launch table in the layout of cvo_debug_irls_eval: edges (f1, f2) and their entry slots back to back."""

    def __init__(self):
        self.frames, self.off, self.r, self.c, self.w = [], [0], [], [], []

    def add(self, f1, f2, r, c, w):
        self.frames.append((f1, f2))
        self.off.append(self.off[-1] + len(r))
        self.r.append(np.asarray(r, np.int32))
        self.c.append(np.asarray(c, np.int32))
        self.w.append(np.asarray(w, np.float32))
        return self

    @property
    def n_edges(self):
        return len(self.frames)

    def arrays(self):
        z = [np.zeros(0, np.int32)]
        return (np.asarray(self.frames, np.int32).reshape(-1, 2), np.asarray(self.off, np.int32),
                np.concatenate(self.r + z), np.concatenate(self.c + z),
                np.concatenate(self.w + [np.zeros(0, np.float32)]))

    def edge(self, k):
        return self.frames[k][0], self.frames[k][1], self.r[k], self.c[k], self.w[k]


def _ints(a, scale, lim):
    v = np.asarray(a, np.float64) * scale
    i = np.rint(v).astype(np.int64)
    assert np.array_equal(i, v) and (np.abs(i) <= lim).all(), "input is not on the exact grid"
    return i


def exact_edge(x1, x2, r, c, w, T1, T2):
    """Integer evaluation of one edge over its stored entries (c >= 0).  Returns (val[91], mag[91]) as Python ints in
    quanta of 2^-SHIFTS: val = the exact (cost, g, upper H), mag = sum over entries of |term|."""
    keep = np.asarray(c) >= 0
    r, c = np.asarray(r)[keep], np.asarray(c)[keep]
    p1, p2 = _ints(x1, 8, 16)[r], _ints(x2, 8, 16)[c]
    w16 = _ints(np.asarray(w)[keep], 16, 16)
    assert (w16 > 0).all() and ((w16 & (w16 - 1)) == 0).all()
    T1, T2 = np.asarray(T1, np.float64).reshape(3, 4), np.asarray(T2, np.float64).reshape(3, 4)
    R1, R2 = _ints(T1[:, :3], 2, 2), _ints(T2[:, :3], 2, 2)
    t1, t2 = _ints(T1[:, 3], 8, 8), _ints(T2[:, 3], 8, 8)
    e = (p1 @ R1.T + 2 * t1) - (p2 @ R2.T + 2 * t2)          # / 16
    res = w16 * (e * e).sum(1)                                # / 4096
    a, b = e @ R1, -(e @ R2)                                  # / 32
    J = np.hstack([8 * a, np.cross(p1, a), 8 * b, np.cross(p2, b)])   # / 256
    assert len(r) < (1 << 18) and (np.abs(e) <= 224).all() and (np.abs(J) < (1 << 16)).all() and (res < (1 << 22)).all()
    aJ = np.abs(J)
    val = [int((res * res).sum())] + [int(v) for v in J.T @ res] + [int(v) for v in (J.T @ J)[TRIU]]
    mag = [int((res * res).sum())] + [int(v) for v in aJ.T @ res] + [int(v) for v in (aJ.T @ aJ)[TRIU]]
    return val, mag


def to_doubles(val):
    """The doubles the integers stand for (exact: every |val| is below 2^53)."""
    return np.array([math.ldexp(float(v), -int(s)) for v, s in zip(val, SHIFTS)])


def exact_table(xyz, poses, table):
    """(expected [E x 91] doubles, the largest sum |term| over all edges and components, in quanta)."""
    out = np.zeros((table.n_edges, W))
    worst = 0
    for k in range(table.n_edges):
        f1, f2, r, c, w = table.edge(k)
        val, mag = exact_edge(xyz[f1], xyz[f2], r, c, w, poses[f1], poses[f2])
        worst = max(worst, max(mag))
        out[k] = to_doubles(val)
    return out, worst
