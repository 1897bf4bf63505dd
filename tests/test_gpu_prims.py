"""The device primitives the front ends' kernels share (cvo_k_prims.h, cvo_k_compact.h, cvo_k_sort.h), each on its own through
cvo_debug_prim: the scan of an ordered compaction, the radix sort of (u64, u32) pairs, wave_alloc, table_insert (with
wave_count_add), uf_unite / uf_find and the inclusive / exclusive block ranks.  The expectations are numpy's; every
comparison is exact integer equality.  The shapes are the smallest at which each primitive can go wrong: the scan's 1024
counts per pass and an uneven split, the sort's 256-pair blocks, waves that want nothing, a table exactly half full, chains
across wave edges, the first and last lane of a wave and of a block."""
import numpy as np
import pytest

import cases
from unified_cvo_amd import CvoGPU

pytestmark = pytest.mark.gpu

SCAN, SORT, WAVE_ALLOC, INSERT, UNION, RANK = range(6)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


# ---- the scan of the block counts ----
@pytest.mark.parametrize("nb", [0, 1, 2, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("kind", ["random", "last"])
def test_scan_offsets_and_total(gpu, nb, kind):
    rng = np.random.default_rng(nb)
    counts = rng.integers(0, 1025, nb).astype(np.uint32) if kind == "random" else np.zeros(nb, np.uint32)
    if kind == "last" and nb:
        counts[-1] = 1024
    _, offsets, total = gpu.debug_prim(SCAN, nb, 0, [], counts, [0xDEAD])
    run = np.cumsum(counts, dtype=np.uint64)
    assert np.array_equal(offsets, (run - counts).astype(np.uint32))
    assert total[0] == (run[-1] if nb else 0)


# ---- the radix sort ----
def _sort(gpu, keys):
    n = len(keys)
    k64 = np.zeros(2 * n, np.uint64)
    k64[:n] = keys
    val = np.zeros(2 * n, np.uint32)
    val[:n] = np.arange(n)
    k64, val, _ = gpu.debug_prim(SORT, n, 0, k64, val, np.zeros(256 * ((n + 255) // 256), np.uint32))
    return k64[:n], val[:n]


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 513])
@pytest.mark.parametrize("kind", ["all bytes", "four keys", "one key"])
def test_radix_sort_is_ordered_and_stable(gpu, n, kind):
    rng = np.random.default_rng(n)
    if kind == "all bytes":
        keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    elif kind == "four keys":
        keys = np.array([0x0102030405060708, 0x0102030405060709, 0xF102030405060708, 7], np.uint64)[rng.integers(0, 4, n)]
    else:
        keys = np.full(n, 0x8000000000000001, np.uint64)
    got_keys, got_val = _sort(gpu, keys)
    order = np.argsort(keys, kind="stable")  # (the values are the original indices: stability shows in them)
    assert np.array_equal(got_val, order.astype(np.uint32))
    assert np.array_equal(got_keys, keys[order])


# ---- wave_alloc ----
def test_wave_alloc_ranges_are_disjoint_and_in_lane_order(gpu):
    n = 3 * 256
    want = np.array([0, 1, 3], np.uint32)[np.arange(n) % 3]
    want[5 * 64:6 * 64] = 0  # a wave that wants nothing at all
    want[64:128] = 3         # ... and one whose every lane wants
    _, start, counter = gpu.debug_prim(WAVE_ALLOC, n, 0, [], want, [0])
    assert counter[0] == want.sum()
    ranges = []
    for w in range(n // 64):
        ws, ww = start[64 * w:64 * w + 64].astype(np.int64), want[64 * w:64 * w + 64].astype(np.int64)
        if ww.sum() == 0:
            continue
        excl = np.cumsum(ww) - ww
        assert np.array_equal(ws - ws[0], excl), w  # contiguous inside the wave, in lane order
        ranges.append((int(ws[0]), int(ws[0] + ww.sum())))
    ranges.sort()
    assert ranges[0][0] == 0 and ranges[-1][1] == want.sum()
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))  # disjoint, and together the whole counter


# ---- table_insert ----
def _mix(k):
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(30))
        k = k * np.uint64(0xbf58476d1ce4e5b9)
        k = k ^ (k >> np.uint64(27))
        k = k * np.uint64(0x94d049bb133111eb)
        return k ^ (k >> np.uint64(31))


def _insert_cases():
    rng = np.random.default_rng(7)
    distinct = lambda n: np.unique(rng.integers(0, 1 << 63, 2 * n + 8, dtype=np.uint64))[:n]
    yield "one key", np.array([12345], np.uint64), 2
    yield "512 lanes, one key", np.full(512, 0x123456789ABCDEF, np.uint64), 1024
    for n in (8, 64, 512):
        yield f"{n} distinct keys, {2 * n} slots", rng.permutation(distinct(n)), 2 * n
    yield "700 lanes, 90 keys", distinct(90)[rng.integers(0, 90, 700)], 2048
    yield "neighbouring keys", np.arange(300, dtype=np.uint64) + np.uint64(1 << 41), 1024


@pytest.mark.parametrize("name,keys,slots", list(_insert_cases()), ids=[c[0] for c in _insert_cases()])
def test_table_insert_claims_one_slot_per_key(gpu, name, keys, slots):
    n = len(keys)
    k64 = np.zeros(n + slots, np.uint64)
    k64[:n] = keys
    k64, slot, info = gpu.debug_prim(INSERT, n, slots, k64, np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32))
    table, fresh, visited = k64[n:], info[1:] & 1, info[1:] >> 1
    uniq = np.unique(keys)
    assert np.all(slot < slots) and np.array_equal(table[slot], keys)  # equal keys: one slot, distinct keys: distinct slots
    assert np.array_equal(np.sort(table[table != EMPTY]), uniq)        # the key array holds exactly those keys
    assert fresh.sum() == len(uniq) and info[0] == len(uniq)           # (info[0]: the same count through wave_count_add)
    home = (_mix(keys) & np.uint64(0xFFFFFFFF)).astype(np.int64) & (slots - 1)
    assert np.array_equal(visited.astype(np.int64), ((slot.astype(np.int64) - home) & (slots - 1)) + 1)  # linear, from the home slot


# ---- union-find ----
def _lowest_of_component(n, edges):
    low = np.arange(n)
    changed = True
    while changed:
        changed = False
        for a, b in edges:
            m = min(low[a], low[b])
            if low[a] != m or low[b] != m:
                low[a] = low[b] = m
                changed = True
    return low


def _union_cases():
    chain = [(i, i + 1) for i in range(129)]
    yield "chain of 130", 130, chain
    yield "chain of 130, reversed edge order", 130, chain[::-1]
    yield "chain of 130, edges turned round", 130, [(b, a) for a, b in chain]
    yield "two components and isolated cells", 70, [(3, 9), (9, 65), (65, 4), (10, 20), (20, 69), (69, 11)]
    yield "a cycle", 67, [(i, (i + 1) % 67) for i in range(67)]
    yield "no edges", 5, []


@pytest.mark.parametrize("name,n,edges", list(_union_cases()), ids=[c[0] for c in _union_cases()])
def test_union_find_roots_are_the_lowest_cells(gpu, name, n, edges):
    roots, _, _ = gpu.debug_prim(UNION, n, len(edges), np.zeros(n, np.uint64), np.array(edges, np.uint32).reshape(-1), np.zeros(n, np.uint32))
    assert np.array_equal(roots.astype(np.int64), _lowest_of_component(n, edges))


# ---- block ranks ----
def test_block_ranks_inclusive_and_exclusive(gpu):
    n = 1024 + 300  # the second block is not full
    flag = np.zeros(n, np.uint32)
    flag[[0, 63, 64, 1023, 1024, 1024 + 63, 1024 + 128, 1024 + 299]] = 1
    offset = np.array([5, 9], np.uint32)
    packed, _, _ = gpu.debug_prim(RANK, n, 0, np.zeros(n, np.uint64), flag, offset)
    incl, excl = (packed >> np.uint64(32)).astype(np.int64), (packed & np.uint64(0xFFFFFFFF)).astype(np.int64)
    want = np.concatenate([np.cumsum(flag[:1024]) + 5, np.cumsum(flag[1024:]) + 9]).astype(np.int64)
    assert np.array_equal(incl, want)
    assert np.array_equal(excl, np.where(flag != 0, want - 1, NONE))


def test_arrays_too_small_are_refused(gpu):
    with pytest.raises(Exception):
        gpu.debug_prim(INSERT, 9, 16, np.zeros(25, np.uint64), np.zeros(9, np.uint32), np.zeros(10, np.uint32))  # more than half full
    with pytest.raises(Exception):
        gpu.debug_prim(UNION, 4, 1, np.zeros(4, np.uint64), [0, 4], np.zeros(4, np.uint32))  # an edge to a cell that is not there
