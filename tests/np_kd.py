"""numpy statement of the spatial (k-d) ordering of an uploaded cloud - spatial_order(..., level_axes = true) of
cvo_upload.hip, which k_kd_order (cvo_k_cloud.h) computes on the device - written level by level, and the degenerate
clouds its tests share.  Shares no code with the library.

The rule: fewer than 8 points or any non-finite coordinate -> the identity.  Otherwise the root box's extents (max - min,
float32) choose one axis per LEVEL - the largest extent, decided by strict `>` in the order y then z over x, so ties go to
the lower axis - every segment of more than 4 points is put in (coordinate, original index) order along it and cut at
kd_left(points), the axis' extent is halved (float32), until a level splits nothing.  The coordinate is compared as a
float: -0.0 == +0.0, and the index decides between them."""
import numpy as np


def kd_left(nn):
    """Points that go left when a segment of nn points is cut: a multiple of 512 / 64 / 4, 0 = the segment is done."""
    if nn <= 4:
        return 0
    unit = 512 if nn > 512 else (64 if nn > 64 else 4)
    left = ((nn // 2 + unit - 1) // unit) * unit
    if left >= nn:
        left -= unit
    return max(left, 0)


def float_key(v):
    """The statement's key: the coordinate itself (numpy sorts floats by `<`: the two zeros are equal)."""
    return np.asarray(v, np.float32)


def bit_pattern_key(v):
    """What a sort of the raw bit pattern sees (sign bit flipped for positives, all bits for negatives): -0.0 < +0.0
    strictly.  NOT the statement - kept to show on which inputs the two rules part (test_kd_cpu.py)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def ordered_key(v):
    """kd_ordered (cvo_k_cloud.h) in numpy, uint32: the bit-pattern key of v + 0.0 - the two zeros are ONE key, 0x80000000 -
    so that `<` on keys is `<` on the floats and `==` on keys is `==` on the floats.  What the multi-block ordering's radix
    select works on (cvo_k_kd_wide.h); the statement itself sorts by float_key."""
    return bit_pattern_key(np.asarray(v, np.float32) + np.float32(0.0))


def key_to_float(k):
    """The inverse of ordered_key: the float32 whose key is k.  (0x7fffffff is no float's key - it would be -0.0's, which
    shares +0.0's - and keys from 0xff800000 on / up to 0x007fffff are the infinities and NaNs.)"""
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def wide_plan(n, leaf):
    """The plan of the multi-block ordering (wide_plan, cvo_upload.hip) of n points from kd_left alone: (level, lo, hi, left)
    of every cut of a segment of more than `leaf` points, level by level and by position inside a level."""
    return _wide_plan(n, leaf)[0]


def wide_plan_leaves(n, leaf):
    """... and its leaves: (level, lo, points, NP) of every segment of at most `leaf` points, with the level at which it left
    the global partitions and the power of two (>= 1024) its block sorts."""
    return _wide_plan(n, leaf)[1]


def _wide_plan(n, leaf):
    cuts, leaves, level, cur = [], [], 0, [(0, n)]
    while cur:
        nxt = []
        for lo, hi in cur:
            if hi - lo > leaf:
                left = kd_left(hi - lo)
                cuts.append((level, lo, hi, left))
                nxt += [(lo, lo + left), (lo + left, hi)]
            else:
                NP = 1024
                while NP < hi - lo:
                    NP *= 2
                leaves.append((level, lo, hi - lo, NP))
        cur, level = nxt, level + 1
    return cuts, leaves


def order(xyz, key=float_key, record=None):
    """int32 permutation: the original index of the point at every sorted position.  record (a list): receives one
    (level, axis, lo, hi, left, members) per split - `members` the original indices of the segment [lo, hi) BEFORE the
    level ordered it - and one (level, None, lo, hi, 0, None) per segment that a level found done."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = x.shape[0]
    out = np.arange(n, dtype=np.int32)
    if n < 8 or not np.isfinite(x).all():
        return out
    ext = (x.max(axis=0) - x.min(axis=0)).astype(np.float32)
    segments = [(0, n)]
    level = 0
    while True:
        axis = 0
        if ext[1] > ext[axis]:
            axis = 1
        if ext[2] > ext[axis]:
            axis = 2
        nxt, split = [], False
        for lo, hi in segments:
            left = kd_left(hi - lo)
            if left == 0:
                nxt.append((lo, hi))
                if record is not None:
                    record.append((level, None, lo, hi, 0, None))
                continue
            members = out[lo:hi].copy()
            by = np.lexsort((members, key(x[members, axis])))  # (the last key is the primary one)
            out[lo:hi] = members[by]
            nxt += [(lo, lo + left), (lo + left, hi)]
            split = True
            if record is not None:
                record.append((level, axis, lo, hi, left, members))
        if not split:
            return out
        segments = nxt
        ext[axis] = np.float32(ext[axis] * np.float32(0.5))
        level += 1


def leaf_sets(order_):
    """Every aligned run of four sorted positions is one leaf of the ordering: its point set, order-free (the rows of a
    (ceil(n / 4), 4) array, each sorted, the last padded with -1)."""
    o = np.asarray(order_)
    pad = (-len(o)) % 4
    return np.sort(np.concatenate([o, np.full(pad, -1, o.dtype)]).reshape(-1, 4), axis=1)


# ---- the degenerate clouds (n points each, float32) ----

def _slab(n, seed):
    rs = np.random.default_rng(52000 + seed)
    return (rs.uniform(-1.0, 1.0, (n, 3)) * np.array([10.0, 8.0, 1.0])).astype(np.float32)


def lattice(n):
    """rint(4 x) of a slab: an integer lattice, thousands of equal coordinates per axis.  (+ 0.0: rint leaves -0.0 for
    -0.125 < x < 0; the signed zeros have clouds of their own.)"""
    x = np.rint(4.0 * _slab(n, 1)).astype(np.float32) + np.float32(0.0)
    assert not np.signbit(x[x == 0]).any()
    return x


def identical(n):
    return np.tile(np.array([[0.3, -1.2, 7.7]], np.float32), (n, 1))


def plane(n):
    x = _slab(n, 2)
    x[:, 2] = np.float32(3.25)
    return x


def line(n):
    x = _slab(n, 3)
    x[:, 0] = np.float32(-1.5)
    x[:, 2] = np.float32(3.25)
    return x


def cube(n):
    """Three equal extents (exactly 1): the axis tie goes x, y, z, x, ..."""
    x = np.random.default_rng(52004).uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    x[0] = 0.0
    x[1] = 1.0
    return x


def wide_range(n):
    """x from 1e-40 (subnormal in float32) to 1e30, in a shuffled order."""
    x = _slab(n, 5)
    x[:, 0] = np.random.default_rng(52005).permutation(np.geomspace(1e-40, 1e30, n)).astype(np.float32)
    assert 0 < x[:, 0].min() < np.finfo(np.float32).tiny
    return x


def signed_zeros(n, level=1):
    """The widest axis (level 1; level 2: the axis of the second level, y) holds +0.0 / -0.0 alternating by index over
    the middle half of the points; the rest of it is spread over both signs, so the cuts fall among the zeros."""
    x = _slab(n, 6 + level)
    a = 0 if level == 1 else 1
    mid = np.arange(n // 4, n // 4 + n // 2)
    x[mid, a] = np.where(mid % 2 == 0, np.float32(0.0), np.float32(-0.0))
    assert np.signbit(x[mid, a]).sum() == len(mid) // 2
    return x


DEGENERATE = {
    "lattice": lattice, "identical": identical, "plane": plane, "line": line, "cube": cube, "wide-range": wide_range,
    "signed-zeros-level1": lambda n: signed_zeros(n, 1), "signed-zeros-level2": lambda n: signed_zeros(n, 2),
}
