"""The semantic voxel map against upstream's OWN compiled code, without a GPU.  tests/golden/bki_upstream.npz records what
upstream's bkiblock.cpp, bkioctree.cpp, bkioctree_node.cpp, point3f.cpp and rtree.h answer under oracle/bki_upstream_driver.cpp
(scripts/make_bki_upstream_golden.py; bki_upstream.py describes the arrays): keys, centres and leaf locations, the R-tree's
block membership, Semantics::update with its state rule and read-outs, and whole frames composed of the three.  The statement
(np_bki.py) and the CPU twin are held to it here, the kernels in test_gpu_bki_upstream.py: bit patterns and integers, no
tolerance.  Excluded, as DESIGN.md declares: the order of a voxel's feature sum (the frames' rows are dyadic, every order gives
one sum), the order of the cloud (both sides are put in ascending key order), blocks upstream keeps only for a neighbour's sake.
When oracle/_ref/bki_upstream is built, the fixture is also rerun and has to come out as committed."""
import os

import numpy as np
import pytest

import bki_cases as bc
import bki_upstream as bu
import np_bki
import test_bki_cpu as cpu

F32 = np.float32
FX = bu.load()
RES = range(len(FX["res"]))
CASES = bu.insert_cases(FX)
# the longest run of hits in one voxel, per insert case and frame (None: whatever the scattered hits make it): 17, 65 and 300
# are beyond bki_cases.SHORT_RUN, the last case's first frame is exactly on it
LONGEST = [[17, 65, 300], [17, 65, None], [16, 17]]


def test_fixture_names_what_made_it():
    assert str(FX["meta_generator"]) == "scripts/make_bki_upstream_golden.py"
    assert "-ffp-contract=off" in str(FX["meta_line"]) and "fast-math" not in str(FX["meta_line"]).replace("-fno-fast-math", "")
    files = [str(f) for f in FX["meta_files"]]
    assert [f for f in files if f.endswith(".cpp")] == [f"src/mapping/{n}.cpp" for n in ("bkiblock", "bkioctree", "bkioctree_node", "point3f")]
    assert "include/UnifiedCvo/mapping/rtree.h" in files and all(len(str(h)) == 64 for h in FX["meta_sha256"])


# ---- the statement against the fixture ----
@pytest.mark.parametrize("r", RES)
def test_statement_keys_and_centres(r):
    s = F32(FX["res"][r])
    for p, key, centre, loc in zip(FX[f"pts{r}"], FX[f"key{r}"], FX[f"centre{r}"], FX[f"loc{r}"]):
        k = [np_bki.k0_of(c, s) for c in p]
        assert (k[0] << 40) | (k[1] << 20) | k[2] == int(key), p
        want = bc.f32(*[F32(a - np_bki.KOFF) * s for a in k])  # the statement's centre expression (Map.cloud)
        assert np.array_equal(bc.bits(want), bc.bits(centre)) and np.array_equal(bc.bits(want), bc.bits(loc)), p


@pytest.mark.parametrize("r", RES)
def test_statement_memberships(r):
    s = F32(FX["res"][r])
    ends = np.concatenate([[0], np.cumsum(FX[f"mem_count{r}"])])
    seen = set()
    for i, p in enumerate(FX[f"pts{r}"]):
        want = sorted(int(k) for k in FX[f"mem_keys{r}"][ends[i]:ends[i + 1]])
        assert sorted(np_bki.blocks_of(p[0], p[1], p[2], s)) == want, (p, want)
        seen.add(len(want))
    assert seen == ({0, 1, 2, 4, 8} if r == 2 else {1, 2, 4, 8})  # (a rounding gap exists at bki_cases.GAP_RESOLUTION only)


def test_the_gap_point_is_in_no_block_upstream():
    r = 2
    assert F32(FX["res"][r]) == bc.GAP_RESOLUTION and bc.bits(FX[f"pts{r}"][0])[0] == bc.bits(bc.GAP_X)
    assert FX[f"mem_count{r}"][0] == 0


def test_statement_node_steps():
    """ms as the map accumulates them, state_of, the first maximum and the two read-outs after every update"""
    states = set()
    for (nc, (prior, free_t, occ_t), ybars, fbars), steps in zip(bu.node_sequences(FX), bu.node_steps(FX)):
        cfg = np_bki.Config(free_thresh=free_t, occupied_thresh=occ_t)
        ms, fs = np.full(nc, prior, F32), np.zeros(5, F32)
        for y, f, up in zip(ybars, fbars, steps):
            ms, fs = ms + y, fs + f
            assert np.array_equal(bc.bits(ms), bc.bits(up["ms"])) and np.array_equal(bc.bits(fs), bc.bits(up["fs"]))
            assert np_bki.state_of(cfg, ms) == up["state"], (nc, prior, ms)
            tot = F32(0)
            for m in ms:
                tot = F32(tot + m)
            assert int(np.argmax(ms / tot)) == up["semantics"]
            assert np.array_equal(bc.bits(ms / tot), bc.bits(up["probs"]))
            feat, occ = np_bki.read_out(ms, fs)
            assert np.array_equal(bc.bits(feat), bc.bits(up["features"])) and np.array_equal(bc.bits(occ), bc.bits(up["occ"]))
            states.add(up["state"])
    assert states == {np_bki.FREE, np_bki.OCCUPIED, np_bki.UNKNOWN}


@pytest.mark.parametrize("row", range(len(bc.THRESHOLDS)))
def test_hand_counted_states_are_upstreams(row):
    free, occupied, thresholds, want = bc.THRESHOLDS[row]
    nc, par, ybars, _ = bu.node_sequences(FX)[row]
    assert nc == 2 and par == (F32(0),) + tuple(F32(t) for t in thresholds)
    assert list(ybars.sum(axis=0)) == [free, occupied]
    assert bu.node_steps(FX)[row][-1]["state"] == want


def config_of(C, par):
    return np_bki.Config(resolution=par[0], num_classes=C, prior=par[1], free_thresh=par[2], occupied_thresh=par[3], free_resolution=100.0)


def against_upstream(i, f, table, cloud, what):
    """a map's table (keys ascending, ms, fs) and cloud after frame f of insert case i, against upstream's blocks"""
    C = CASES[i][0]
    up = {name: FX[f"ins{i}_{f}_{name}"] for name in ("key", "ms", "fs", "state", "loc", "features", "occ")}
    diff = bc.first_difference(dict(keys=table[0], ms=table[1], fs=table[2]), (up["key"], up["ms"], up["fs"]))
    assert diff is None, f"{what}, case {i}, frame {f}: {diff.replace('statement', 'upstream')}"
    occupied = up["state"] == np_bki.OCCUPIED
    assert 0 < occupied.sum() < len(occupied)
    xyz, feat, label = cloud
    assert len(xyz) == occupied.sum(), f"{what}, case {i}, frame {f}: {len(xyz)} voxels in the cloud, upstream has {occupied.sum()} OCCUPIED"
    for name, got, want in (("xyz", xyz, up["loc"]), ("feat", feat, up["features"]), ("label", label, up["occ"][:, :C])):
        assert np.array_equal(bc.bits(got), bc.bits(want[occupied])), f"{what}, case {i}, frame {f}: cloud {name} differs"


@pytest.mark.parametrize("i", range(len(CASES)))
def test_statement_inserts(i):
    C, par, frames = CASES[i]
    m = np_bki.Map(config_of(C, par))
    for f, frame in enumerate(frames):
        m.insert(*frame)
        against_upstream(i, f, m.table(), m.cloud(), "statement")
        for key, state in zip(FX[f"ins{i}_{f}_key"], FX[f"ins{i}_{f}_state"]):
            assert np_bki.state_of(m.cfg, m.voxels[int(key)][0]) == state


# ---- the CPU twin against the fixture, directly ----
@pytest.mark.parametrize("i", range(len(CASES)))
def test_twin_inserts(i):
    C, par, frames = CASES[i]
    got = cpu.run_twin((config_of(C, par), frames))
    for f, (stats, cloud, size) in enumerate(got):
        assert stats["on_device"] == 0
        against_upstream(i, f, (stats["keys"], stats["ms"], stats["fs"]), cloud, "twin")
        assert size == (len(FX[f"ins{i}_{f}_key"]), int((FX[f"ins{i}_{f}_state"] == np_bki.OCCUPIED).sum()))
        assert LONGEST[i][f] in (None, stats["longest_run"])


def threshold_run_agrees(run, row):
    """the map case of a THRESHOLDS row through `run`: its voxel holds upstream's ms and is in the cloud iff upstream's node,
    given the same counts, is OCCUPIED"""
    free, occupied, thresholds, _ = bc.THRESHOLDS[row]
    steps = bu.node_steps(FX)[row]
    got = run(bc.threshold_case(free, occupied, thresholds))
    assert len(got) == len(steps)
    for (stats, cloud, size), up in zip(got, steps):
        assert np.array_equal(bc.bits(stats["ms"]), bc.bits(up["ms"][None]))
        assert len(cloud[0]) == (1 if up["state"] == np_bki.OCCUPIED else 0) == size[1]
        if len(cloud[0]):
            assert np.array_equal(bc.bits(cloud[1][0]), bc.bits(up["features"]))


@pytest.mark.parametrize("row", range(len(bc.THRESHOLDS)))
def test_twin_thresholds(row):
    threshold_run_agrees(cpu.run_twin, row)


# ---- the fixture against the binary, where it is built ----
def test_fixture_is_what_the_binary_answers():
    if not os.path.exists(bu.BINARY):
        pytest.skip("oracle/_ref/bki_upstream is not built: build() compiles it only where a checkout of upstream is present")
    out = bu.run(FX)
    for name, want in out.items():
        assert FX[name].dtype == want.dtype and np.array_equal(FX[name].view(np.uint8), want.view(np.uint8)), name
