"""The numpy statement of the spatial ordering (np_kd.py) held to its own definition, without a GPU: a permutation, every
cut takes the smallest (coordinate, index) pairs of its segment, every aligned run of 4 / 64 / 512 positions is a segment
of some level - and the inputs on which a bit-pattern key orders differently (signed zeros), so that the device test
(test_gpu_kd_order.py) is known to tell the two rules apart."""
import numpy as np
import pytest

import np_kd
from unified_cvo_amd import synth

SIZES = (8, 9, 12, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049, 4097, 16384)


def _clouds():
    out = [(f"slab{n}", synth.geometric_pair(n, 7)[0]) for n in SIZES]
    for name, make in np_kd.DEGENERATE.items():
        out += [(f"{name}{n}", make(n)) for n in (64, 600, 4097)]
    return out


CLOUDS = _clouds()


def test_kd_left_is_a_restatement_of_the_split_rule():
    for nn in range(0, 5):
        assert np_kd.kd_left(nn) == 0
    for nn in range(5, 20000):
        left = np_kd.kd_left(nn)
        unit = 512 if nn > 512 else (64 if nn > 64 else 4)
        assert 0 < left < nn and left % unit == 0
        assert abs(left - nn / 2) < unit                 # the multiple of the unit next to the middle


@pytest.mark.parametrize("case", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_statement_holds_its_own_definition(case):
    _, x = case
    n = x.shape[0]
    rec = []
    o = np_kd.order(x, record=rec)
    assert o.dtype == np.int32 and np.array_equal(np.sort(o), np.arange(n))
    segments = {(0, n)}
    axes = {}
    for level, axis, lo, hi, left, members in rec:
        segments.add((lo, hi))
        if axis is None:
            continue
        assert axes.setdefault(level, axis) == axis       # one axis per level
        # the left part: exactly the `left` smallest (coordinate, index) pairs, compared as floats then as integers
        pairs = sorted(zip(x[members, axis].tolist(), members.tolist()))
        assert {i for _, i in pairs[:left]} == set(o[lo:lo + left].tolist()), (level, lo, hi)
        assert {i for _, i in pairs[left:]} == set(o[lo + left:hi].tolist()), (level, lo, hi)
    for unit in (4, 64, 512):
        for lo in range(0, n, unit):
            assert (lo, min(lo + unit, n)) in segments, (unit, lo)


def test_axis_ties_go_to_the_lower_axis_in_turn():
    rec = []
    np_kd.order(np_kd.cube(600), record=rec)
    axes = {}
    for level, axis, *_ in rec:
        if axis is not None:
            axes[level] = axis
    assert [axes[k] for k in sorted(axes)][:7] == [0, 1, 2, 0, 1, 2, 0]


def test_small_and_non_finite_clouds_keep_their_order():
    for n in range(0, 8):
        assert np.array_equal(np_kd.order(synth.geometric_pair(max(n, 1), 3)[0][:n]), np.arange(n))
    for bad in (np.nan, np.inf, -np.inf):
        x = synth.geometric_pair(100, 3)[0].copy()
        x[17, 1] = bad
        assert np.array_equal(np_kd.order(x), np.arange(100))


@pytest.mark.parametrize("n", [64, 600, 4097])
@pytest.mark.parametrize("level", [1, 2])
def test_signed_zeros_tell_a_bit_pattern_key_from_the_float_comparison(n, level):
    """A property of the INPUT: on the signed-zero clouds a sort of the coordinates' bit patterns (-0.0 < +0.0) fills the
    leaves differently from the float comparison (-0.0 == +0.0, then the index).  On a cloud without signed zeros the two
    keys agree - subnormals and 1e30 included."""
    x = np_kd.signed_zeros(n, level)
    want = np_kd.leaf_sets(np_kd.order(x))
    assert not np.array_equal(np_kd.leaf_sets(np_kd.order(x, key=np_kd.bit_pattern_key)), want)
    # (made equal by ordering -0.0 as +0.0 before the bits are taken)
    assert np.array_equal(np_kd.leaf_sets(np_kd.order(x, key=lambda v: np_kd.bit_pattern_key(v + np.float32(0.0)))), want)
    for other in (synth.geometric_pair(n, 7)[0], np_kd.wide_range(n), np_kd.lattice(n)):
        assert np.array_equal(np_kd.leaf_sets(np_kd.order(other, key=np_kd.bit_pattern_key)), np_kd.leaf_sets(np_kd.order(other)))
