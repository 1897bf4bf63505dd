"""The case file of oracle/bki_upstream_driver.cpp (upstream's compiled mapping code under a driver of this repository's) and
its result file, to and from the arrays that tests/golden/bki_upstream.npz keeps.  Used by scripts/make_bki_upstream_golden.py,
which records the results, and by tests/test_bki_upstream.py, which reruns the binary on the recorded inputs when it is there.

Inputs (the generator's) and outputs (the binary's) of the fixture:
  res (3,)                          the resolutions of `keys` and `members`
  pts{r} (n, 3)                     -> key{r} (n,) uint64, centre{r} (n, 3), loc{r} (n, 3), mem_count{r} (n,), mem_keys{r} (sum,)
  node_nc / node_par / node_steps   per sequence: num_class, (prior, free_thresh, occupied_thresh), the number of updates
  node_in                           every sequence's updates, flat: (ybars (num_class), fbars (5)) per update
                                    -> node_out, flat words: per update ms, fs, state, semantics, probs, occupied probs, features
  ins_C (cases,), ins_par (cases, 4), ins_frames (cases,)    num_classes of the library's map, (resolution, prior, free_thresh,
                                    occupied_thresh), frames
  ins{i}_{f}_xyz / _feat / _label / _origin                  a frame's hits; the origin is the frame's one class-0 training point
                                    -> ins{i}_{f}_key / _updated / _ms / _fs / _state / _loc / _features / _occ over the blocks
                                       updated so far, ascending key
Floats cross as bit patterns; nothing here computes a value that is compared."""
import os
import subprocess
import tempfile

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "oracle", "_ref", "bki_upstream")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bki_upstream.npz")
KEYS, MEMBERS, NODE, INSERT = 1, 2, 3, 4


def _w(a, dtype=None):
    """words of an array: float32 as its bits, integers as uint32"""
    a = np.ascontiguousarray(a, dtype)
    return (a.view(np.uint32) if a.dtype == F32 else a.astype(np.uint32)).reshape(-1)


def nclass_of(C):
    return max(int(C), 1) + 1


def classes_of(label, n, C):
    """class of every hit: 1 + the label row's maximum, 1 on a map without classes"""
    return 1 + np.argmax(label, axis=1) if C > 0 else np.ones(n, np.int64)


def node_sequences(fx):
    """[(num_class, (prior, free_thresh, occupied_thresh), ybars (steps, num_class), fbars (steps, 5))]"""
    out, at = [], 0
    for nc, par, steps in zip(fx["node_nc"], fx["node_par"], fx["node_steps"]):
        rows = np.asarray(fx["node_in"][at:at + steps * (nc + 5)], F32).reshape(steps, nc + 5)
        at += steps * (nc + 5)
        out.append((int(nc), tuple(F32(p) for p in par), rows[:, :nc], rows[:, nc:]))
    return out


def insert_cases(fx):
    """[(num_classes, (resolution, prior, free_thresh, occupied_thresh), [(xyz, feat, label or None, origin)])]"""
    out = []
    for i, (C, par, frames) in enumerate(zip(fx["ins_C"], fx["ins_par"], fx["ins_frames"])):
        fr = [(fx[f"ins{i}_{f}_xyz"], fx[f"ins{i}_{f}_feat"], fx[f"ins{i}_{f}_label"] if C > 0 else None, fx[f"ins{i}_{f}_origin"])
              for f in range(frames)]
        out.append((int(C), tuple(F32(p) for p in par), fr))
    return out


def encode(fx):
    """the case file's words of a fixture's inputs"""
    w = []
    for op in (KEYS, MEMBERS):
        for r, res in enumerate(fx["res"]):
            pts = fx[f"pts{r}"]
            w += [_w([op]), _w([res], F32), _w([len(pts)]), _w(pts, F32)]
    for nc, par, ybars, fbars in node_sequences(fx):
        w += [_w([NODE, nc]), _w(par, F32), _w([len(ybars)]), _w(np.concatenate([ybars, fbars], axis=1), F32)]
    for C, par, frames in insert_cases(fx):
        w += [_w([INSERT]), _w(par[:1], F32), _w([nclass_of(C)]), _w(par[1:], F32), _w([len(frames)])]
        for xyz, feat, label, origin in frames:
            n = len(xyz)
            rec = np.zeros((n + 1, 10), np.uint32)
            rec[:n, 0:3] = _w(xyz, F32).reshape(n, 3)
            rec[:n, 3] = classes_of(label, n, C)
            rec[:n, 4] = 1
            rec[:n, 5:] = _w(feat, F32).reshape(n, 5)
            rec[n, 0:3] = _w(origin, F32)  # class 0, no feature row
            w += [_w([n + 1]), rec.reshape(-1)]
    return np.concatenate(w)


def _key(lo_hi):
    lo_hi = np.asarray(lo_hi, np.uint64).reshape(-1, 2)
    return lo_hi[:, 0] | (lo_hi[:, 1] << np.uint64(32))


def decode(fx, words):
    """the outputs of a fixture's inputs from the result file's words"""
    out, at = {}, 0

    def take(n):
        nonlocal at
        assert at + n <= len(words), "the result file is too short"
        at += n
        return words[at - n:at]

    for r in range(len(fx["res"])):
        n = len(fx[f"pts{r}"])
        t = take(8 * n).reshape(n, 8)
        out[f"key{r}"], out[f"centre{r}"], out[f"loc{r}"] = _key(t[:, :2]), t[:, 2:5].view(F32).copy(), t[:, 5:8].view(F32).copy()
    for r in range(len(fx["res"])):
        counts, keys = [], []
        for _ in range(len(fx[f"pts{r}"])):
            m = int(take(1)[0])
            counts.append(m)
            keys.append(_key(take(2 * m)))
        out[f"mem_count{r}"], out[f"mem_keys{r}"] = np.array(counts, np.int32), np.concatenate(keys + [np.zeros(0, np.uint64)])
    start = at
    for nc, _, ybars, _ in node_sequences(fx):
        take(len(ybars) * node_step_words(nc))
    out["node_out"] = words[start:at].copy()
    for i, (C, _, frames) in enumerate(insert_cases(fx)):
        nc = nclass_of(C)
        for f in range(len(frames)):
            v = int(take(1)[0])
            t = take(v * (2 + 1 + nc + 5 + 1 + 3 + 5 + nc - 1)).reshape(v, -1)
            cut = np.cumsum([2, 1, nc, 5, 1, 3, 5])
            key, updated, ms, fs, state, loc, features, occ = np.split(t, cut, axis=1)
            out.update({f"ins{i}_{f}_key": _key(key), f"ins{i}_{f}_updated": updated[:, 0].astype(np.uint8),
                        f"ins{i}_{f}_state": state[:, 0].astype(np.uint8)})
            for name, a in (("ms", ms), ("fs", fs), ("loc", loc), ("features", features), ("occ", occ)):
                out[f"ins{i}_{f}_{name}"] = np.ascontiguousarray(a).view(F32)
    assert at == len(words), "the result file is too long"
    return out


def node_step_words(nc):
    return nc + 5 + 1 + 1 + nc + (nc - 1) + 5


def node_steps(fx, node_out=None):
    """[[dict(ms, fs, state, semantics, probs, occ, features)] per update] per sequence, from node_out"""
    words = np.asarray(fx["node_out"] if node_out is None else node_out, np.uint32)
    out, at = [], 0
    for nc, _, ybars, _ in node_sequences(fx):
        seq = []
        for _ in range(len(ybars)):
            t = words[at:at + node_step_words(nc)]
            at += node_step_words(nc)
            ms, fs, st, probs, occ, features = np.split(t, np.cumsum([nc, 5, 2, nc, nc - 1]))
            seq.append(dict(ms=ms.view(F32), fs=fs.view(F32), state=int(st[0]), semantics=int(st[1]), probs=probs.view(F32),
                            occ=occ.view(F32), features=features.view(F32)))
        out.append(seq)
    return out


def run(fx, binary=BINARY):
    """runs the binary on a fixture's inputs -> its outputs"""
    with tempfile.TemporaryDirectory() as tmp:
        cases, results = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "results.bin")
        encode(fx).astype("<u4").tofile(cases)
        subprocess.check_call([binary, cases, results])
        return decode(fx, np.fromfile(results, "<u4"))


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
