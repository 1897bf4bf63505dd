"""The cases of kd_wide_cases.py held to what they are named for, without a GPU: a case that stopped being the edge it claims
to be would leave test_gpu_kd_wide_edges.py green and empty.  Every comparison is exact."""
import numpy as np
import pytest

import kd_wide_cases as kc
import np_kd


def test_ordered_key_states_the_float_order():
    v = np.array([-np.inf, -3e38, -16.0, -1e-45, -0.0, 0.0, 1e-45, 7.9999995, 8.0, 3e38, np.inf], np.float32)
    k = np_kd.ordered_key(v)
    assert k.dtype == np.uint32
    assert k[4] == k[5] == 0x80000000                                   # the two zeros: one key
    assert (np.diff(k.astype(np.int64)) > 0).sum() == len(v) - 2 and (np.diff(k.astype(np.int64)) >= 0).all()
    assert k[2] == 0x3E7FFFFF and k[7] == 0xC0FFFFFF and k[8] == 0xC1000000
    back = np_kd.key_to_float(k)
    assert np.array_equal(back.view(np.uint32), (v + np.float32(0.0)).view(np.uint32))
    rs = np.random.default_rng(1)
    keys = rs.integers(0x00800000, 0xFF800000, 4096).astype(np.uint32)  # every finite float but -0.0's own pattern
    keys = keys[keys != 0x7FFFFFFF]
    assert np.array_equal(np_kd.ordered_key(np_kd.key_to_float(keys)), keys)
    f = np_kd.key_to_float(np.sort(keys))
    assert np.isfinite(f).all() and (np.diff(f.astype(np.float64)) >= 0).all()


@pytest.mark.parametrize("name", list(kc.CRAFTED))
def test_a_crafted_case_is_the_edge_it_is_named_for(name):
    P, lo, hi, rem, eqs = kc.CRAFTED[name]
    x = kc.crafted(name)
    assert x.shape == (kc.N, 3) and x.dtype == np.float32 and np.isfinite(x).all()
    assert np.array_equal(x, kc.crafted(name))
    assert kc.LEFT == 10240 and len(range(0, kc.N, kc.TILE)) == 10
    ext = (x.max(axis=0) - x.min(axis=0)).astype(np.float32)
    assert np.isfinite(ext).all() and ext[0] > ext[1] > ext[2] > 0
    record = []
    np_kd.order(x, record=record)
    level, axis, lo_, hi_, left, members = record[0]
    assert (level, axis, lo_, hi_, left) == (0, 0, 0, kc.N, kc.LEFT) and np.array_equal(members, np.arange(kc.N))
    keys = np.sort(np_kd.ordered_key(x[:, 0]))
    assert keys[left - 1] == P
    assert left - int((keys < P).sum()) == rem and int((keys == P).sum()) == eqs and 1 <= rem <= eqs
    assert lo <= keys[0] and keys[-1] <= hi
    for q, want in enumerate(kc.DIGITS[name]):
        assert want is None or (P >> (24 - 8 * q)) & 0xFF == want, (q, hex(P))
    if name == "low-byte-only":
        assert len(np.unique(keys >> 8)) == 1
    if name == "negative-side":
        assert (x[:, 0] < 0).all()
    if name == "top-byte-ff":
        assert x[:, 0].min() >= 0 and np_kd.key_to_float(P) >= np.float32(2.0) ** 127
    if name == "top-byte-00":
        assert x[:, 0].max() <= 0 and np_kd.key_to_float(P) <= -(np.float32(2.0) ** 127)


def test_the_digit_cases_sit_on_the_ends_of_the_scan():
    """Thread 0 / thread 255 find the rank in passes 1 to 3, and in pass 0 (the top-byte cases)."""
    assert kc.DIGITS["digits-00"][1:] == (0, 0, 0) and kc.DIGITS["digits-ff"][1:] == (255, 255, 255)
    assert kc.DIGITS["top-byte-00"][0] == 0 and kc.DIGITS["top-byte-ff"][0] == 255
    # digits-00's pivot is the first key of its top digit and digits-ff's the last of its own: both cut between two top digits
    assert kc.CRAFTED["digits-00"][0] - 1 == kc.CRAFTED["digits-ff"][0]


def test_the_scatter_case_takes_the_second_trip():
    level, lo, hi, left = np_kd.wide_plan(kc.SCATTER_N, 1024)[0]
    assert (level, lo, hi) == (0, 0, kc.SCATTER_N)
    assert -(-(hi - lo) // kc.TILE) == 293 > 257


def test_the_leaf_cases_cover_their_edges():
    plans = kc.leaf_plan_properties()
    assert len(plans) == len(kc.LEAVES) * len(kc.LEAF_SIZES)
    for (leaf, n), leaves in plans.items():
        assert sum(m for _, _, m, _ in leaves) == n and all(0 < m <= leaf and m <= NP < max(2 * m, 2048) for _, _, m, NP in leaves)
        x = kc.LEAF_KINDS["signed-zeros-level2"](n)
        assert np.signbit(x[x[:, 1] == 0, 1]).any() and not np.signbit(x[x[:, 1] == 0, 1]).all()
