"""Cases of the semantic voxel map's tests (test_bki_cpu.py, test_gpu_bki.py, test_cpp_bki.py): a case is (Config, frames), a
frame (xyz, feat, label, origin).  The constants mirror unified_cvo_amd/csrc/cvo_k_bki.h (test_bki_cpu.py checks the mirror)."""
import numpy as np

import np_bki

F32 = np.float32
THREADS = 256     # BKI_THREADS: lanes (hits) per block
WAVE = 64         # BKI_WAVE
SHORT_RUN = 16    # BKI_SHORT_RUN: hits of a voxel the update kernel sums itself; longer runs take the wave kernel

# a coordinate in the rounding gap between the boxes of blocks 14 and 15 at this resolution (searched on the CPU):
# float(14 * s) + s / 2 < GAP_X < float(15 * s) - s / 2 in float32
GAP_RESOLUTION = F32(0.5460466146469116)
GAP_X = np.uint32(1090346394).view(F32)


def f32(*v):
    return np.array(v, F32)


def rows(rng, n, C):
    """feature rows with order-sensitive float sums, label rows"""
    feat = (rng.uniform(0, 1, (n, 5)) * np.exp(rng.uniform(-8, 8, (n, 5)))).astype(F32)
    label = rng.uniform(0, 1, (n, C)).astype(F32) if C else None
    return feat, label


def frame(rng, xyz, C, origin=(0.125, 0.25, -0.125)):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    feat, label = rows(rng, xyz.shape[0], C)
    return xyz, feat, label, f32(*origin)


def scattered(seed, n, C=3, resolution=0.5, spread=6.0, **cfg):
    """n hits in a cube, some on faces / edges / corners of the grid (resolution 0.5: exact floats)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-spread, spread, (n, 3)).astype(F32)
    k = min(n // 4, 40)
    xyz[:k] = (np.round(xyz[:k] * 2) / 2 + F32(0.25) * rng.integers(0, 2, (k, 3))).astype(F32)
    return np_bki.Config(resolution=resolution, num_classes=C, **cfg), [frame(rng, xyz, C)]


def one_voxel_run(seed, run, C=2, extra=5):
    """`run` hits inside ONE voxel (plus a few elsewhere), no beam samples (free_resolution beyond every ray)"""
    rng = np.random.default_rng(seed)
    inside = (f32(2.0, 1.0, -1.0) + rng.uniform(-0.2, 0.2, (run, 3))).astype(F32)
    other = rng.uniform(-5, -3, (extra, 3)).astype(F32)
    xyz = np.concatenate([inside, other])[rng.permutation(run + extra)]
    return np_bki.Config(resolution=0.5, num_classes=C, free_resolution=100.0), [frame(rng, xyz, C)]


def rays(seed=5):
    """the shortest and the longest ray in one wave: 0.4 fr and about 60 fr"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2, 2, (WAVE, 3)).astype(F32)
    xyz[3] = f32(0.125 + 0.4, 0.25, -0.125)
    xyz[40] = f32(0.125 + 35.0, 0.25 + 35.0, -0.125 + 34.0)
    return np_bki.Config(resolution=0.5, num_classes=3), [frame(rng, xyz, 3)]


def three_inserts(seed=7, C=19):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(3):
        xyz = rng.uniform(-3, 3, (300, 3)).astype(F32)
        xyz[:100] = np.round(xyz[:100])  # (voxel centres shared between the frames)
        frames.append(frame(rng, xyz, C, origin=(0.1 * f, 0.2, 0.3)))
    return np_bki.Config(resolution=0.5, num_classes=C, prior=0.3), frames


def growth(seed=9):
    rng = np.random.default_rng(seed)
    return np_bki.Config(resolution=0.25, num_classes=2), [frame(rng, rng.uniform(-4, 4, (150, 3)).astype(F32), 2),
                                                          frame(rng, rng.uniform(4, 12, (400, 3)).astype(F32), 2)]


def occupied_cloud(seed, n):
    """about n OCCUPIED voxels whose keys differ in the high (x), middle (y) and low (z) field; no beam samples"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-300, 300, (n, 3))
    k[:, 0] *= 7
    xyz = (k.astype(F32) * F32(0.5))
    return np_bki.Config(resolution=0.5, num_classes=19, free_resolution=1e4), [frame(rng, xyz, 19, origin=(0.1, 0.1, 0.1))]


def sizes():
    t = THREADS
    return [1, 63, 64, 65, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1]


RUNS = [1, 2, SHORT_RUN, SHORT_RUN + 1, 63, 64, 65, 3000]

# ---- micro cases, hand-counted in test_bki_cpu.py: name -> (Config kwargs, xyz, label or None, origin) ----
# resolution 0.5: faces at odd multiples of 0.25 are exact floats.  free_resolution 100: no beam samples unless said.
_Q = dict(resolution=0.5, free_resolution=100.0)
MICRO = {
    "centre": (dict(_Q), [[1.0, 1.0, 1.0]], None, [0.0, 0.0, 0.0]),
    "face": (dict(_Q), [[1.25, 1.0, 1.0]], None, [0.0, 0.0, 0.0]),
    "edge": (dict(_Q), [[1.25, 1.25, 1.0]], None, [0.0, 0.0, 0.0]),
    "corner": (dict(_Q), [[1.25, 1.25, 1.25]], None, [0.0, 0.0, 0.0]),
    "gap": (dict(resolution=float(GAP_RESOLUTION), free_resolution=100.0), [[float(GAP_X), 0.0, 0.0]], None, [0.0, 0.0, 0.0]),
    "hit_is_origin": (dict(_Q), [[1.0, 1.0, 1.0]], None, [1.0, 1.0, 1.0]),
    "label_tie": (dict(_Q, num_classes=3), [[1.0, 1.0, 1.0]], [[0.25, 0.75, 0.75]], [0.0, 0.0, 0.0]),
    "prior": (dict(_Q, prior=0.3), [[1.0, 1.0, 1.0]], None, [0.0, 0.0, 0.0]),
    "one_class": (dict(_Q, num_classes=1), [[1.0, 1.0, 1.0]], [[0.5]], [0.0, 0.0, 0.0]),
    "nineteen": (dict(_Q, num_classes=19), [[1.0, 1.0, 1.0]], [[0.0] * 18 + [1.0]], [0.0, 0.0, 0.0]),
}
# rays along x from the origin with free_resolution 1: l just below, at, just above fr and 2 fr -> beam samples
BELOW = float(np.nextafter(F32(1), F32(0)))
ABOVE = float(np.nextafter(F32(1), F32(2)))
BELOW2 = float(np.nextafter(F32(2), F32(0)))
ABOVE2 = float(np.nextafter(F32(2), F32(3)))
RAY_LENGTHS = {BELOW: 0, 1.0: 0, ABOVE: 2, BELOW2: 2, 2.0: 2, ABOVE2: 3}
# max_range 2: a hit at distance 2 stays, the next float goes
RANGE = {2.0: True, ABOVE2: False}


# one voxel with exactly `free` class-0 and `occupied` class-1 training points, hand-counted: (free, occupied, (free_thresh,
# occupied_thresh), the state).  1 - probs[0] just on either side of the driver's 0.9 and 0.65, and exactly on exact thresholds.
THRESHOLDS = [
    (1, 9, (0.65, 0.9), np_bki.UNKNOWN),    # 1 - 0.1f rounds to 0.9f: not above it
    (1, 10, (0.65, 0.9), np_bki.OCCUPIED),  # 10 / 11 = 0.909
    (6, 13, (0.65, 0.9), np_bki.UNKNOWN),   # 13 / 19 = 0.684
    (8, 13, (0.65, 0.9), np_bki.FREE),      # 13 / 21 = 0.619 < 0.65
    (5, 4, (0.65, 0.9), np_bki.FREE),       # the first maximum is class 0
    (1, 1, (0.5, 0.5), np_bki.FREE),        # a tie of the maximum goes to class 0
    (1, 3, (0.25, 0.75), np_bki.UNKNOWN),   # exactly 0.75: not above
    (3, 5, (0.625, 0.9), np_bki.UNKNOWN),   # exactly 0.625: not below
]


def threshold_name(free, occupied, thresholds):
    return f"state_{free}_{occupied}_{thresholds[0]}_{thresholds[1]}"


def threshold_case(free, occupied, thresholds):
    """`occupied` hits on the centre of the voxel (2, 2, 2) seen from that centre - no beam, the origin is the first class-0
    point -, then free - 1 frames without hits whose origin is the same centre"""
    centre = f32(1.0, 1.0, 1.0)
    cfg = np_bki.Config(resolution=0.5, free_resolution=100.0, free_thresh=thresholds[0], occupied_thresh=thresholds[1])
    frames = [(np.tile(centre, (occupied, 1)), np.ones((occupied, 5), F32), None, centre)]
    frames += [(np.zeros((0, 3), F32), np.zeros((0, 5), F32), None, centre) for _ in range(free - 1)]
    return cfg, frames


def range_name(distance):
    return f"range_{distance!r}"


def micro_map(name):
    kw, xyz, label, origin = MICRO[name]
    m = np_bki.Map(np_bki.Config(**kw))
    m.insert(f32(*xyz), np.ones((len(xyz), 5), F32), None if label is None else f32(*label), f32(*origin))
    return m


def all_cases():
    """name -> (Config, frames): every case the twin and the kernels are compared with the statement on"""
    out = {}
    for n in sizes():
        out[f"hits{n}"] = scattered(100 + n, n, C=3 if n % 2 else 0, prior=0.3 if n == 65 else 0.0)
    for r in RUNS:
        out[f"run{r}"] = one_voxel_run(200 + r, r)
    out["rays"] = rays()
    out["three_inserts"] = three_inserts()
    out["growth"] = growth()
    out["driver_resolution"] = scattered(11, 120, C=19, resolution=0.05, spread=1.5)
    out["max_range"] = scattered(12, 200, C=1, max_range=5.0)
    for name, (kw, xyz, label, origin) in MICRO.items():
        out["micro_" + name] = (np_bki.Config(**kw), [(f32(*xyz), np.ones((len(xyz), 5), F32), None if label is None else f32(*label), f32(*origin))])
    for l in RAY_LENGTHS:
        out[f"ray_{l!r}"] = (np_bki.Config(resolution=0.5, free_resolution=1.0), [(f32([l, 0.0, 0.0]), None, None, f32(0, 0, 0))])
    for distance in RANGE:  # max_range 2 at the bound and at the next float
        out[range_name(distance)] = (np_bki.Config(resolution=0.5, free_resolution=100.0, max_range=2.0),
                                     [(f32([distance, 0.0, 0.0]), np.ones((1, 5), F32), None, f32(0, 0, 0))])
    for free, occupied, thresholds, _ in THRESHOLDS:
        out[threshold_name(free, occupied, thresholds)] = threshold_case(free, occupied, thresholds)
    return out


def statement(case):
    """[(table, cloud, last)] of the statement after every frame of the case"""
    cfg, frames = case
    m = np_bki.Map(cfg)
    out = []
    for xyz, feat, label, origin in frames:
        m.insert(xyz, feat, label, origin)
        out.append((m.table(), m.cloud(), dict(m.last)))
    return out


_STATEMENTS = {}


def statement_of(name):
    """... computed once per test session, shared and left unchanged"""
    if name not in _STATEMENTS:
        _STATEMENTS[name] = statement(all_cases()[name])
    return _STATEMENTS[name]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def first_difference(got, want):
    """Names the first voxel of a read-back table (debug_stats(readback=True)) that differs from the statement's table."""
    keys, ms, fs = want
    if len(got["keys"]) != len(keys) or not np.array_equal(got["keys"], keys):
        n = min(len(keys), len(got["keys"]))
        d = np.flatnonzero(got["keys"][:n] != keys[:n])
        at = int(d[0]) if len(d) else n
        return f"keys differ at voxel {at} of {len(got['keys'])} (statement: {len(keys)})"
    for name, a, b in (("ms", got["ms"], ms), ("fs", got["fs"], fs)):
        d = np.flatnonzero((bits(a) != bits(b)).any(axis=1))
        if len(d):
            v = int(d[0])
            return f"{name} differs first at voxel {v} (key {int(keys[v]):#x}): {a[v]} against the statement's {b[v]}"
    return None
