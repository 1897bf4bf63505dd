#!/usr/bin/env python
"""Makes tests/golden/bki_upstream.npz: what upstream's OWN compiled mapping code (bkiblock.cpp, bkioctree.cpp,
bkioctree_node.cpp, point3f.cpp, rtree.h) answers to generated inputs, so that tests/np_bki.py, the CPU twin and the kernels
of the semantic voxel map are held to upstream's object code and not to a reading of its text.

    make -C oracle bki_upstream UPSTREAM=/path/to/the/reference      (or __graft_entry__.build() with the checkout in place)
    python scripts/make_bki_upstream_golden.py [--out FILE]

The script builds the inputs, runs oracle/_ref/bki_upstream (oracle/bki_upstream_driver.cpp: the operations keys, members, node
and insert) and stores inputs, outputs and metadata (this script's name, the compiler line, the sha256 of every upstream file
the compiler read).  tests/bki_upstream.py describes the arrays.  Nothing of upstream, source or compiled, is kept.

The script asserts what the inputs must contain, the membership part on the binary's own answers:
  * keys / members, per resolution (0.5: every face an exact float; 0.05, the driver's: float(k) * 0.05f rounds;
    bki_cases.GAP_RESOLUTION): points in 1, 2 (face), 4 (edge) and 8 (corner) blocks; per axis a k0 that is the only, the upper
    and - where rounding allows it - the lower of the holding blocks; negative coordinates; |k| = 2^19 - 2; the floats next to
    a face on both sides; 300 random points.  Points in NO block exist only where `float(k) * size +/- size / 2` rounds far
    enough: at 0.5 nothing rounds, and at 0.05 no two neighbouring boxes of the whole key range leave a float between them
    (a scan of all 2^20 faces finds none), so they are asserted at GAP_RESOLUTION (bki_cases.GAP_X; that resolution has two
    such faces, 14 | 15 and -15 | -14) and asserted ABSENT at 0.5 and 0.05; likewise a k0 below its holding block is asserted
    at 0.05 and asserted absent at 0.5, where p / size is exact.
  * node: every row of bki_cases.THRESHOLDS as the updates its map case makes; num_class 2, 4 and 20; prior 0 and 0.3; a tie
    of the maximum between class 0 and another class and between two other classes; 3000 counts in one update.
  * insert: no beam samples (the origin is the one class-0 point of a frame, the library's free_resolution is 100); three
    frames that share voxels; per-voxel runs of 1, 16, 17, 64, 65 and 300 hits; hits on faces, edges and corners; label rows
    with ONE maximum (Eigen's maxCoeff is not compiled here); feature rows in multiples of 2^-6 whose absolute sum per voxel
    stays below 2^24 quanta, so that every order of the float additions gives the same sum; all three states occur."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bki_cases as bc  # noqa: E402
import bki_upstream as bu  # noqa: E402
import np_bki  # noqa: E402

F32 = np.float32
KOFF = np_bki.KOFF
KMAX = 2 ** 19 - 2
QUANTUM = F32(2.0 ** -6)


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def lower(k, s):
    return F32(F32(F32(k) * s) - s / F32(2))


def upper(k, s):
    return F32(F32(F32(k) * s) + s / F32(2))


def axis_values(s, rng):
    """-> (inside, special, found): coordinates well inside a block, and coordinates at and next to the faces of blocks near zero, far
    out on both sides, and wherever a scan of 4000 faces finds the three rounding cases (the statement only SEARCHES here;
    what the fixture asserts is counted from the binary's answers)"""
    ks = [0, 1, 2, -1, -2, -3, 7, 14, 15, -14, 1000, -1000, KMAX - 1, -KMAX]
    found = {}
    for k in sorted(range(-2000, 2000), key=abs):  # (the nearest first: the insert frames use them, and their rays stay short)
        lo, hi = lower(k + 1, s), upper(k, s)
        for p in (lo, hi, up(hi), down(lo)):
            held = np_bki.axis_blocks(p, s)
            k0 = np_bki.k0_of(p, s)
            kind = "gap" if not held else "below" if max(held) > k0 else "two" if len(held) == 2 else None
            if kind and len(found.setdefault(kind, [])) < 3:
                found[kind].append(p)
    special = [p for v in found.values() for p in v]
    for k in ks:
        lo, hi = lower(k + 1, s), upper(k, s)
        special += [lo, hi, up(hi), down(lo), up(lo), down(hi)]
    inside = [F32(F32(k) * s) for k in (0, 3, -5, KMAX, -KMAX)] + [F32(F32(k) * s + s / F32(4)) for k in (1, -2, 40)]
    return inside, special, found


def grid_points(s, rng, extra=()):
    inside, special, _ = axis_values(s, rng)
    pts = [list(e) for e in extra]
    for i, c in enumerate(special):
        a, b = inside[i % len(inside)], inside[(i + 3) % len(inside)]
        c2, c3 = special[(i + 6) % len(special)], special[(i + 13) % len(special)]
        pts += [[c, a, b], [a, c, b], [a, b, c], [c, c2, a], [a, c, c2], [c2, b, c], [c, c2, c3], [c, c, c]]
    pts += list(rng.uniform(-6, 6, (300, 3)))
    return np.array(pts, F32)


def per_axis(key):
    return [(int(key) >> 40) & 0xFFFFF, (int(key) >> 20) & 0xFFFFF, int(key) & 0xFFFFF]


def check_members(fx, out, r, exact, gap):
    """the membership cases, counted from the binary's answers"""
    pts, counts, own = fx[f"pts{r}"], out[f"mem_count{r}"], out[f"key{r}"]
    have = set(int(c) for c in counts)
    want = {0, 1, 2, 4, 8} if gap else {1, 2, 4, 8}
    assert have == want, f"resolution {fx['res'][r]}: membership multiplicities {sorted(have)}, wanted {sorted(want)}"
    ends = np.concatenate([[0], np.cumsum(counts)])
    kinds = set()
    for i in range(len(pts)):
        held = [per_axis(k) for k in out[f"mem_keys{r}"][ends[i]:ends[i + 1]]]
        k0 = per_axis(own[i])
        for a in range(3):
            ka = sorted(set(h[a] for h in held))
            if ka:
                kinds.add("only" if ka == [k0[a]] else "upper" if ka == [k0[a] - 1, k0[a]] else "lower" if ka == [k0[a], k0[a] + 1]
                          else "below" if ka == [k0[a] + 1] else "above" if ka == [k0[a] - 1] else f"other{[k - k0[a] for k in ka]}")
    wanted = {"only", "upper"} if exact else {"only", "upper", "lower"}
    assert wanted <= kinds and not [k for k in kinds if k.startswith("other")], f"resolution {fx['res'][r]}: k0 is {sorted(kinds)} of its holding blocks"
    if exact:
        assert kinds == wanted, kinds
    s = F32(fx["res"][r])
    for face in (lower(1, s), upper(0, s), lower(-13, s), upper(KMAX - 1, s)):  # the floats next to a face, both ways
        assert (pts == up(face)).any() and (pts == down(face)).any() and (pts == face).any(), face
    k = np.array([per_axis(x) for x in own]) - KOFF
    assert k.min() == -KMAX and k.max() == KMAX and (pts < 0).any()


def node_inputs(rng):
    seqs = []
    for free, occupied, thresholds, _ in bc.THRESHOLDS:  # the frames of bki_cases.threshold_case as counts
        ybars = [[1, occupied]] + [[1, 0]] * (free - 1)
        fbars = [[float(occupied)] * 5] + [[0.0] * 5] * (free - 1)
        seqs.append((2, (0.0,) + thresholds, ybars, fbars))
    for nc in (2, 4, 20):
        for prior in (0.0, 0.3):
            ybars = np.zeros((8, nc), F32)
            ybars[0, rng.integers(0, nc)] = 1
            ybars[1:6] = rng.integers(0, 4, (5, nc)) * (rng.uniform(0, 1, (5, nc)) < 0.3)
            ybars[6, rng.integers(1, nc)] = 3000
            ybars[7, 0] = 2900
            seqs.append((nc, (prior, 0.65, 0.9), ybars, rng.uniform(-3, 3, (8, 5)).astype(F32)))
    # a tie of the maximum between class 0 and class 2, and between classes 1 and 3 above class 0
    seqs.append((4, (0.0, 0.3, 0.6), [[3, 1, 3, 0], [0, 3, 0, 2], [1, 0, 1, 2]], rng.uniform(0, 1, (3, 5))))
    seqs.append((4, (0.3, 0.3, 0.6), [[1, 4, 0, 4], [2, 0, 0, 0]], rng.uniform(0, 1, (2, 5))))
    seqs.append((20, (0.3, 0.65, 0.9), [[5] + [0] * 18 + [5], [0] * 7 + [9] + [0] * 11 + [4]], rng.uniform(0, 1, (2, 5))))
    fx = dict(node_nc=np.array([s[0] for s in seqs], np.int32), node_par=np.array([s[1] for s in seqs], F32),
              node_steps=np.array([len(s[2]) for s in seqs], np.int32),
              node_in=np.concatenate([np.concatenate([np.asarray(s[2], F32), np.asarray(s[3], F32)], axis=1).reshape(-1) for s in seqs]))
    ties0 = ties = False
    for nc, _, ybars, _ in bu.node_sequences(fx):
        total = np.cumsum(ybars, axis=0)
        assert float(ybars.max()) <= 3000
        for row in total:
            top = np.flatnonzero(row == row.max())
            ties0 |= len(top) > 1 and top[0] == 0
            ties |= len(top) > 1 and top[0] > 0
    assert ties0 and ties and set(fx["node_nc"]) == {2, 4, 20} and float(fx["node_in"].max()) == 3000
    assert {float(p[0]) for p in fx["node_par"]} == {0.0, float(F32(0.3))}
    return fx


# (hits in one voxel, the frame that brings them): 17, 65 and 300 are each the longest run of their frame
RUNS = ((1, 0), (16, 0), (17, 0), (64, 1), (65, 1), (300, 2))
RUNS_005 = ((1, 0), (17, 0), (65, 1))
RUNS_NO_CLASSES = ((16, 0), (17, 1))


def insert_frames(rng, C, s, frames, runs, spread, special, near):
    """`frames` frames on a grid of size s: the runs, each in a voxel of its own (5 more hits go into the voxel of every
    earlier frame's run, so that frames share voxels), hits on faces / edges / corners, and hits on voxel centres shared between frames"""
    out, centres = [], []
    cells = [(spread + 4 + 2 * j, -3, 2) for j in range(len(runs))]
    home = np.array([1, 1, -spread - 3], F32) * s  # the origin's voxel, with `near` hits of its own in every frame
    for f in range(frames):
        xyz = []
        for j, (run, at) in enumerate(runs):
            if at == f:
                centres.append(np.array(cells[j], F32) * s)
                xyz += list(centres[-1] + rng.uniform(-0.4, 0.4, (run, 3)).astype(F32) * s)
            elif at < f:
                xyz += list(np.array(cells[j], F32) * s + rng.uniform(-0.4, 0.4, (5, 3)).astype(F32) * s)
        a = F32(F32(3) * s)
        for c, c2, c3 in zip(special, special[1:] + special[:1], special[2:] + special[:2]):
            xyz += [[c, a, a], [c, c2, a], [a, c2, c3], [c, c2, c3]]
        shared = rng.integers(-spread, spread, (100, 3)).astype(F32) * s
        xyz += list(shared) + list(rng.uniform(-spread, spread, (60, 3)).astype(F32) * s)
        xyz += list(home + rng.uniform(-0.3, 0.3, (near, 3)).astype(F32) * s)
        xyz = np.array(xyz, F32)[rng.permutation(len(xyz))]
        n = len(xyz)
        feat = (rng.integers(-256, 257, (n, 5)).astype(F32) * QUANTUM).astype(F32)
        label = rng.uniform(0, 1, (n, C)).astype(F32)
        origin = (home + np.array([0.1 * f, -0.2, 0.3], F32) * s).astype(F32)
        out.append((xyz, feat, label, origin))
    return out


def insert_inputs(rng):
    face05 = [F32(0.25), F32(-0.75), F32(1.25)]
    found = axis_values(F32(0.05), rng)[2]
    special = found["two"] + found["below"][:1]
    cases = [
        (19, (0.5, 0.3, 0.65, 0.9), insert_frames(rng, 19, F32(0.5), 3, RUNS, 6, face05, 3)),
        (3, (0.05, 0.0, 0.65, 0.9), insert_frames(rng, 3, F32(0.05), 3, RUNS_005, 5, special, 3)),
        (0, (0.5, 0.0, 0.65, 0.9), insert_frames(rng, 0, F32(0.5), 2, RUNS_NO_CLASSES, 4, face05[:1], 1)),
    ]
    fx = dict(ins_C=np.array([c[0] for c in cases], np.int32), ins_par=np.array([c[1] for c in cases], F32),
              ins_frames=np.array([len(c[2]) for c in cases], np.int32))
    for i, (C, par, frames) in enumerate(cases):
        for f, (xyz, feat, label, origin) in enumerate(frames):
            if C > 0:
                top = label.max(axis=1, keepdims=True)
                assert ((label == top).sum(axis=1) == 1).all(), "a label row has more than one maximum"
            assert np.array_equal(feat, np.round(feat / QUANTUM) * QUANTUM), "a feature is no multiple of 2^-6"
            fx.update({f"ins{i}_{f}_xyz": xyz, f"ins{i}_{f}_feat": feat, f"ins{i}_{f}_label": label, f"ins{i}_{f}_origin": origin})
    return fx


def check_insert(fx, out):
    states = set()
    for i, (C, par, frames) in enumerate(bu.insert_cases(fx)):
        quanta = {}
        for f, (xyz, feat, label, origin) in enumerate(frames):
            keys, ms = out[f"ins{i}_{f}_key"], out[f"ins{i}_{f}_ms"]
            states |= set(int(s) for s in out[f"ins{i}_{f}_state"])
            # the dyadic bound, per voxel over all frames, from the statement's membership (an over-count is harmless)
            for p, row in zip(xyz, feat):
                for key in np_bki.blocks_of(p[0], p[1], p[2], par[0]):
                    quanta[key] = quanta.get(key, 0) + int(np.abs(row / QUANTUM).sum())
            hits = ms[:, 1:].sum(axis=1) - par[1] * (ms.shape[1] - 1)
            if f == 0:
                got = set(int(round(float(h))) for h in hits[out[f"ins{i}_{f}_updated"] == 1])
                first = set(run for run, at in (RUNS, RUNS_005, RUNS_NO_CLASSES)[i] if at == 0)
                assert first <= got, f"case {i}: runs {sorted(first)} wanted in frame 0, voxels hold {sorted(got)}"
            if f > 0:
                before = set(int(k) for k in out[f"ins{i}_{f - 1}_key"])
                again = [k for k, u in zip(keys, out[f"ins{i}_{f}_updated"]) if u and int(k) in before]
                assert len(again) > 10, f"case {i}: frame {f} shares {len(again)} voxels with the frames before"
        assert max(quanta.values()) < 2 ** 24, "a voxel's feature sum could round"
        if i == 0:  # every run is there in the end, 5 further hits per later frame on top
            final = sorted(int(round(float(h))) for h in hits)
            for run, at in RUNS:
                assert run + 5 * (len(frames) - 1 - at) in final, (run, final[-10:])
    assert states == {np_bki.FREE, np_bki.OCCUPIED, np_bki.UNKNOWN}, states
    for i, name in ((0, "0.5"), (1, "0.05")):  # faces, edges, corners: voxels that share one hit's feature row exactly
        mult = set()
        C, par, frames = bu.insert_cases(fx)[i]
        for p in frames[0][0]:
            mult.add(len(np_bki.blocks_of(p[0], p[1], p[2], par[0])))
        assert {1, 2, 4, 8} <= mult, f"insert case at {name}: hits lie in {sorted(mult)} blocks"


def metadata():
    text = open(os.path.join(os.path.dirname(bu.BINARY), "bki_upstream.build")).read().splitlines()
    files = [line.split() for line in text[2:]]
    return dict(meta_generator=np.array("scripts/make_bki_upstream_golden.py"), meta_compiler=np.array(text[0].split(": ", 1)[1]),
                meta_line=np.array(text[1].split(": ", 1)[1]), meta_files=np.array([f[1] for f in files]),
                meta_sha256=np.array([f[0] for f in files]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=bu.GOLDEN)
    args = ap.parse_args()
    if not os.path.exists(bu.BINARY):
        sys.exit("oracle/_ref/bki_upstream is not built: make -C oracle bki_upstream UPSTREAM=/path/to/the/reference")
    rng = np.random.default_rng(20)
    fx = dict(res=np.array([0.5, 0.05, bc.GAP_RESOLUTION], F32))
    for r, s in enumerate(fx["res"]):
        fx[f"pts{r}"] = grid_points(F32(s), rng, extra=[(bc.GAP_X, 0.0, 0.0)] if r == 2 else ())
    fx.update(node_inputs(rng))
    fx.update(insert_inputs(rng))
    out = bu.run(fx)
    for r in range(3):
        check_members(fx, out, r, exact=(r == 0), gap=(r == 2))
    assert out["mem_count2"][0] == 0, "bki_cases.GAP_X lies in a block"
    check_insert(fx, out)
    np.savez_compressed(args.out, **fx, **out, **metadata())
    size, limit = os.path.getsize(args.out), max(os.path.getsize(os.path.join(os.path.dirname(bu.GOLDEN), f))
                                                 for f in os.listdir(os.path.dirname(bu.GOLDEN)) if f != "bki_upstream.npz" and not os.path.isdir(os.path.join(os.path.dirname(bu.GOLDEN), f)))
    assert size <= limit, f"{size} bytes: larger than the largest fixture so far ({limit})"
    print(f"{args.out}: {size} bytes; points {[len(fx[f'pts{r}']) for r in range(3)]}, {len(fx['node_nc'])} node sequences, "
          f"voxels after the insert cases {[len(out[f'ins{i}_{int(n) - 1}_key']) for i, n in enumerate(fx['ins_frames'])]}")


if __name__ == "__main__":
    main()
