"""The clouds that put the multi-block ordering (ORDER=wide, cvo_k_kd_wide.h) on the edges of its own bookkeeping, shared by
test_kd_wide_cases_cpu.py - which holds every case to the property it is named for, without a GPU - and
test_gpu_kd_wide_edges.py.  Shares no code with the library.

A crafted cloud has N = 20000 points: kd_left(N) = 10240 go left at level 0, out of ten tiles of 2048 positions.  Its x
coordinates are np_kd.key_to_float of a chosen multiset of ordered keys in a shuffled order - LEFT - rem of them strictly
below the pivot key P, `eqs` equal to P, the rest above - so the key of rank LEFT is P and `rem` of its equals go left; y is
uniform in [0, extent x / 4] and z in [0, extent x / 8], so level 0 cuts along x.  The radix select reads a key as four
digits from the top; P's digits decide which thread of the block scan finds the rank in every pass."""
import numpy as np

import np_kd

N = 20000
LEFT = np_kd.kd_left(N)

# name -> (P, lowest key, highest key, rem, eqs)
_AROUND = lambda P, spread, rem, eqs: (P, P - spread, P + spread, rem, eqs)
CRAFTED = {
    # every key shares the top 24 bits: passes 0 to 2 see one bucket, pass 3 alone decides
    "low-byte-only": _AROUND(0xC0FFEE80, 0x7F, 37, 100),
    # the rank is found by thread 0 of the scan in passes 1 to 3 (8.0) ...
    "digits-00": _AROUND(0xC1000000, 0x200000, 1, 1),
    # ... and by thread 255 (the float below 8.0)
    "digits-ff": _AROUND(0xC0FFFFFF, 0x200000, 5, 5),
    # negative coordinates, whose keys are the inverted bits (P: the float above -16.0)
    "negative-side": _AROUND(0x3E800000, 0x200000, 1, 3),
    # 4000 keys equal to the pivot: the first of them alone goes left / all of them do
    "first-of-equals": _AROUND(0xC0800055, 0x1000, 1, 4000),
    "all-of-equals": _AROUND(0xC0800055, 0x1000, 4000, 4000),
    # the top digit itself at its ends: x in [0, 3e38] with the pivot at 1.5 * 2^127, x in [-3e38, 0] with it at -1.5 * 2^127
    # (one side of zero each: the extent stays finite in float32)
    "top-byte-ff": (0xFF400000, 0x80000000, int(np_kd.ordered_key([3e38])[0]), 1, 1),
    "top-byte-00": (0x00BFFFFF, int(np_kd.ordered_key([-3e38])[0]), 0x7FFFFFFE, 1, 1),
}
# the digits of P the passes 0 .. 3 must pick (None: whatever P has there)
DIGITS = {
    "low-byte-only": (0xC0, 0xFF, 0xEE, 0x80), "digits-00": (None, 0x00, 0x00, 0x00), "digits-ff": (None, 0xFF, 0xFF, 0xFF),
    "negative-side": (0x3E, 0x80, 0x00, 0x00), "first-of-equals": (0xC0, 0x80, 0x00, 0x55), "all-of-equals": (0xC0, 0x80, 0x00, 0x55),
    "top-byte-ff": (0xFF, None, None, None), "top-byte-00": (0x00, None, None, None),
}


def crafted(name):
    """float32[N, 3] of the case `name`: the same array on every call."""
    P, lo, hi, rem, eqs = CRAFTED[name]
    rs = np.random.default_rng(53000 + sorted(CRAFTED).index(name))
    below, above = LEFT - rem, N - (LEFT - rem) - eqs
    keys = np.concatenate([rs.integers(lo, P, below), np.full(eqs, P), rs.integers(P + 1, hi + 1, above)]).astype(np.uint32)
    x = np.zeros((N, 3), np.float32)
    x[:, 0] = np_kd.key_to_float(rs.permutation(keys))
    ext = float(np.float32(x[:, 0].max() - x[:, 0].min()))
    x[:, 1] = rs.uniform(0.0, ext / 4, N)
    x[:, 2] = rs.uniform(0.0, ext / 8, N)
    return x


# ---- the clouds of the other edges ----

# the scatter adds up the counts of a segment's earlier tiles 256 at a trip: tile 257 of one segment is the first that takes
# a second trip, and the root segment of SCATTER_N points has 293 tiles
SCATTER_N = 600001
TILE = 2048


def slab(n, seed=11):
    """A generic cloud (np_kd._slab's box, 20 x 16 x 2)."""
    return np_kd._slab(n, seed)


# WIDE_LEAF away from its default, and the sizes it is run at: between them a leaf exactly at the capacity of the largest
# block (32769 at 16384: 16384 | 16385, the right half cut again), a leaf of 8193 points in a block of 16384 (16385 at
# 16384), and plans whose leaves leave the global levels at both parities of `level` - in either buffer.
LEAVES = (2048, 16384)
LEAF_SIZES = (16385, 20000, 32769, 40000)
LEAF_KINDS = {"generic": slab, "signed-zeros-level2": np_kd.DEGENERATE["signed-zeros-level2"]}


def leaf_plan_properties():
    """What the (leaf, n) of LEAVES x LEAF_SIZES must contain, from np_kd's plan alone: asserted by the CPU test and again
    where the device runs them, so that the set cannot stop covering it unnoticed."""
    plans = {(leaf, n): np_kd.wide_plan_leaves(n, leaf) for leaf in LEAVES for n in LEAF_SIZES}
    every = [l for p in plans.values() for l in p]
    assert any(n == 16384 == NP for _, _, n, NP in every), "no leaf exactly at the capacity of the largest block"
    assert (1, 0, 16384, 16384) in plans[16384, 32769]
    assert any(n == 8193 and NP == 16384 for _, _, n, NP in plans[16384, 16385]), "no half-full block of 16384"
    assert any({level & 1 for level, _, _, _ in p} == {0, 1} for p in plans.values()), "no plan with leaves in both buffers"
    return plans
