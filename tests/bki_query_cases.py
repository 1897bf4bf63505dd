"""Cases of the read side of the semantic voxel map (cvo_map_query / _raycast / _render), shared by test_bki_query_cpu.py,
test_cpp_bki_query.py and test_gpu_bki_query.py: a map (configuration, kernel, frames, the table's first size), the points
queried, the rays cast and the views rendered.  A few voxels up to a few thousand; the statement of a case is computed once
per session (expected) and left unchanged."""
import numpy as np

import bki_cases as bc
import np_bki
import np_bki_query as nq
import np_bki_sparse as sp

F32 = np.float32
f32 = bc.f32
SIZES = [1, 63, 64, 65, 255, 256, 257]  # lane, wave and block edges
ALL_STATES = nq.BIT_FREE | nq.BIT_OCCUPIED | nq.BIT_UNKNOWN


class Case:
    def __init__(self, cfg, frames=(), kernel=sp.CSM, initial_voxels=0, points=None, rays=(), views=()):
        self.cfg, self.frames, self.kernel, self.initial_voxels = cfg, list(frames), kernel, initial_voxels
        self.points = np.zeros((0, 3), F32) if points is None else np.asarray(points, F32).reshape(-1, 3)
        self.rays = list(rays)    # (origin (n, 3), end (n, 3), stop_mask, max_steps)
        self.views = list(views)  # dict(pose, fx, fy, cx, cy, rows, cols, z_far, stop_mask)

    def statement_map(self):
        m = sp.Map(self.cfg, self.kernel)
        for xyz, feat, label, origin in self.frames:
            m.insert(xyz, feat, label, origin)
        return m


def key_of(kx, ky, kz):
    """the key of the voxel whose centre is (kx, ky, kz) * resolution"""
    return ((kx + np_bki.KOFF) << 40) | ((ky + np_bki.KOFF) << 20) | (kz + np_bki.KOFF)


def key_mix(k):
    """key_mix of cvo_k_prims.h: the table's home slot is key_mix(key) & (slots - 1)"""
    M = (1 << 64) - 1
    k = ((k ^ (k >> 30)) * 0xBF58476D1CE4E5B9) & M
    k = ((k ^ (k >> 27)) * 0x94D049BB133111EB) & M
    return k ^ (k >> 31)


def centres(keys, size):
    return np.array([nq.centre_of(int(k), size) for k in keys], F32).reshape(-1, 3)


def ray(o, e):
    return f32(*o), f32(*e)


def rays_of(pairs, mask, max_steps=nq.MAX_STEPS):
    return (np.array([p[0] for p in pairs], F32).reshape(-1, 3), np.array([p[1] for p in pairs], F32).reshape(-1, 3), mask, max_steps)


def around(m, rng, extra, spread):
    """the centres of every stored voxel, of their face neighbours, and `extra` random points"""
    size = m.cfg.resolution
    keys = sorted(m.voxels)
    near = sorted({sp.slot_key(k, j) for k in keys for j in range(1, 7)} - {None} - set(keys))
    return np.concatenate([centres(keys, size), centres(near, size), rng.uniform(-spread, spread, (extra, 3)).astype(F32)])


# ---- the maps ----
def one_hit(occupied_thresh, prior=0.5):
    """One hit on a voxel corner, seen along the diagonal: its 8 voxels, the origin's and the beam's.  The voxel nearest the origin
    also holds beam samples and is FREE; the other seven hold the hit alone: (prior + 1) / (2 prior + 1) = 0.75 is OCCUPIED
    above 0.7 and UNKNOWN under 0.8."""
    cfg = np_bki.Config(resolution=0.5, num_classes=0, prior=prior, free_thresh=0.3, occupied_thresh=occupied_thresh, free_resolution=0.3)
    rng = np.random.default_rng(3)
    frames = [bc.frame(rng, [[1.25, 1.25, 1.25]], 0, origin=(0.0, 0.0, 0.0))]
    c = Case(cfg, frames)
    m = c.statement_map()
    c.points = around(m, rng, 20, 2.0)
    o = (0.0, 0.0, 0.0)
    pairs = [ray(o, (1.25, 1.25, 1.25)), ray(o, (2.0, 2.0, 2.0)), ray((2.0, 2.0, 2.0), o), ray((1.5, 1.5, 1.5), (1.5, 1.5, -1.0)),
             ray((1.5, 1.0, 1.0), (-1.0, 1.0, 1.0)), ray((3.0, 3.0, 3.0), (1.0, 1.0, 1.0))]
    c.rays = [rays_of(pairs, mask) for mask in (0, 1, 2, 4, 6, 8, 15)]
    return c


def faces():
    """hits exactly on a voxel face on each axis, both signs: stored in two voxels, found in one"""
    cfg = np_bki.Config(resolution=0.5, num_classes=3, free_resolution=100.0)
    pts = []
    for a in range(3):
        for s in (1.0, -1.0):
            p = [s * 1.0, s * 2.0, s * 3.0]
            p[a] = s * (abs(p[a]) + 0.25)
            pts.append(p)
    rng = np.random.default_rng(4)
    frames = [bc.frame(rng, pts, 3, origin=(0.0, 0.0, 0.0))]
    q = list(pts)
    for p in pts:  # ... and the floats on either side of the face
        for a in range(3):
            for d in (-np.inf, np.inf):
                r = f32(*p)
                r[a] = np.nextafter(r[a], F32(d))
                q.append(r)
    return Case(cfg, frames, points=q)


def key_range():
    """voxels at k0 = 1 and 2^20 - 2, one step beyond on each side, NaN and infinity"""
    cfg = np_bki.Config(resolution=0.5, num_classes=1, prior=0.25, free_resolution=100.0)
    lo, hi = F32((1 - np_bki.KOFF) * 0.5), F32((2**20 - 2 - np_bki.KOFF) * 0.5)
    rng = np.random.default_rng(5)
    frames = [bc.frame(rng, [[lo, lo, lo]], 1, origin=(lo, lo, lo)), bc.frame(rng, [[hi, hi, hi]], 1, origin=(hi, hi, hi))]
    below, above = F32(lo - F32(0.5)), F32(hi + F32(0.5))
    pts = [[lo, lo, lo], [hi, hi, hi], [lo, hi, lo], [below, lo, lo], [lo, below, lo], [lo, lo, below], [above, hi, hi], [hi, above, hi],
           [hi, hi, above], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [1e30, 0, 0], [0.0, 0.0, 0.0]]
    far = [ray((lo, lo, lo), (lo + 1.0, lo, lo)), ray((hi, hi, hi), (hi, hi - 1.0, hi)), ray((below, lo, lo), (lo, lo, lo)), ray((hi, hi, hi), (hi, hi, above)),
           ray((np.nan, 0, 0), (1, 0, 0)), ray((0, 0, 0), (0, np.inf, 0)), ray((0, 0, 0), (3e38, 0, 0))]
    return Case(cfg, frames, points=pts, rays=[rays_of(far, nq.BIT_OCCUPIED), rays_of(far, 0)])


def scattered(C, prior, kernel=sp.CSM, n=60, seed=11):
    cfg, frames = bc.scattered(seed + C, n, C=C, prior=prior, sf2=1.0, ell=0.4, free_resolution=0.7)
    c = Case(cfg, frames, kernel=kernel)
    rng = np.random.default_rng(seed)
    m = c.statement_map()
    keys = sorted(m.voxels)
    pick = [keys[i] for i in rng.permutation(len(keys))[:150]]
    near = sorted({sp.slot_key(k, j) for k in pick[:40] for j in range(1, 7)} - {None})
    c.points = np.concatenate([frames[0][0], centres(pick, cfg.resolution), centres(near, cfg.resolution), rng.uniform(-7, 7, (40, 3)).astype(F32)])
    o = np.broadcast_to(frames[0][3], (32, 3))
    e = rng.uniform(-7, 7, (32, 3)).astype(F32)
    c.rays = [(o, e, mask, nq.MAX_STEPS) for mask in (nq.BIT_OCCUPIED, nq.BIT_OCCUPIED | nq.BIT_UNKNOWN, nq.BIT_ABSENT)]
    return c


def long_chains():
    """A table of 32 slots (the smallest) that one insert of 13 memberships does not grow, with five voxels whose home slot is
    the LAST one: whichever arrives first takes it, the others wrap to slots 0, 1 ... - a probe chain past the table's end
    whatever the arrival order.  Queried for every present key and for absent keys with the same home slot and the slots behind."""
    cfg = np_bki.Config(resolution=0.5, num_classes=2, prior=0.1, free_resolution=100.0)
    slots, last, present, absent, other = 32, 31, [], [], []
    for kx in range(-12, 12):
        for ky in range(-12, 12):
            for kz in range(-3, 3):
                h = key_mix(key_of(kx, ky, kz)) & (slots - 1)
                if h == last and len(present) < 5:
                    present.append((kx, ky, kz))
                elif h in (last, 0, 1, 2) and len(absent) < 24:
                    absent.append((kx, ky, kz))
                elif h in (7, 8) and len(other) < 7:
                    other.append((kx, ky, kz))
    assert len(present) == 5 and len(absent) == 24 and len(other) == 7
    hits = np.array(present + other, F32) * F32(0.5)  # (12 hits on voxel centres + the origin: 13 memberships, 26 <= 32)
    rng = np.random.default_rng(6)
    origin = np.array(other[0], F32) * F32(0.5)
    frames = [bc.frame(rng, hits, 2, origin=tuple(origin))]
    pts = np.concatenate([hits, np.array(absent, F32) * F32(0.5)])
    e = np.concatenate([hits, np.array(absent[:8], F32) * F32(0.5)])
    return Case(cfg, frames, initial_voxels=0, points=pts, rays=[(np.broadcast_to(origin, e.shape), e, nq.BIT_OCCUPIED, nq.MAX_STEPS)])


def growth(n_frames):
    cfg, frames = bc.growth()
    c = Case(cfg, frames[:n_frames], initial_voxels=0)
    rng = np.random.default_rng(8)
    m = Case(cfg, frames).statement_map()  # (the keys of BOTH frames are queried before the second one is in)
    keys = sorted(m.voxels)
    pick = [keys[i] for i in rng.permutation(len(keys))[:200]]
    c.points = np.concatenate([centres(pick, cfg.resolution), rng.uniform(-5, 13, (56, 3)).astype(F32)])
    return c


def sized(n, seed=21):
    """n points and n rays on the map of three_inserts (19 classes, prior 0.3)"""
    cfg, frames = bc.three_inserts()
    rng = np.random.default_rng(seed + n)
    pts = rng.uniform(-3.5, 3.5, (n, 3)).astype(F32)
    pts[::3] = np.round(pts[::3])
    o = rng.uniform(-1, 1, (n, 3)).astype(F32)
    e = rng.uniform(-4, 4, (n, 3)).astype(F32)
    return Case(cfg, frames, points=pts, rays=[(o, e, nq.BIT_OCCUPIED, nq.MAX_STEPS)])


def wall():
    """A wall of OCCUPIED voxels at x = 2 seen from 0: every hit twice, FREE voxels under the beams, and one wall voxel that a
    second frame's origin turns UNKNOWN: ms = (1, 2), 2 / 3 between the thresholds 0.3 and 0.9."""
    cfg = np_bki.Config(resolution=0.5, num_classes=0, prior=0.0, free_thresh=0.3, occupied_thresh=0.9, free_resolution=0.5)
    g = np.arange(-1.0, 1.01, 0.5)
    hits = np.array([[2.0, y, z] for y in g for z in g] * 2, F32)
    rng = np.random.default_rng(9)
    frames = [bc.frame(rng, hits, 0, origin=(0.0, 0.0, 0.0)), bc.frame(rng, np.zeros((0, 3), F32), 0, origin=(2.0, 0.0, 0.0))]
    c = Case(cfg, frames)
    m = c.statement_map()
    assert np_bki.state_of(cfg, m.voxels[key_of(4, 0, 0)][0]) == np_bki.UNKNOWN and np_bki.state_of(cfg, m.voxels[key_of(4, 2, 2)][0]) == np_bki.OCCUPIED
    c.points = around(m, rng, 10, 3.0)
    o = (0.0, 0.0, 0.0)
    pairs = [
        ray(o, o), ray((0.1, 0.2, -0.1), (0.1, 0.2, -0.1)),                      # zero length
        ray((0.05, 0.1, -0.2), (-0.2, 0.24, 0.2)),                               # inside one voxel
        ray(o, (3.0, 0.0, 0.0)), ray(o, (-3.0, 0.0, 0.0)), ray(o, (0.0, 3.0, 0.0)), ray(o, (0.0, -3.0, 0.0)),
        ray(o, (0.0, 0.0, 3.0)), ray(o, (0.0, 0.0, -3.0)),                       # axis-parallel
        ray(o, (3.0, 3.0, 3.0)), ray(o, (-3.0, -3.0, -3.0)), ray(o, (3.0, -3.0, 3.0)),  # through voxel corners: three-way ties
        ray(o, (3.0, 3.0, 0.0)), ray(o, (0.0, -3.0, 3.0)), ray((0.0, 0.0, 0.1), (3.0, 3.0, 0.1)),  # through edges: two-way ties
        ray((0.25, 0.25, 0.0), (2.25, 1.25, 0.0)),                               # from a corner, along faces
        ray((0.0, 5.0, 0.0), (2.0, 0.5, 0.0)), ray((-4.0, -4.0, 3.0), (2.0, 0.5, 0.5)),  # starting in a voxel that is not stored
        ray(o, (1.5, 0.75, 0.75)), ray(o, (2.0, 1.0, 1.0)), ray(o, (3.0, 1.5, 1.5)),  # ending before, in and behind an OCCUPIED voxel
        ray(o, (3.0, 0.0, 0.0)), ray((1.0, 0.1, 0.0), (2.6, -0.1, 0.1)),         # through the UNKNOWN voxel
        ray((3.0, 0.5, 0.5), (0.0, 0.5, 0.5)), ray((2.0, 1.0, 1.0), (2.0, -1.0, -1.0)),  # from behind the wall; inside the wall
    ]
    c.rays = [rays_of(pairs, mask) for mask in (nq.BIT_OCCUPIED, nq.BIT_OCCUPIED | nq.BIT_UNKNOWN, nq.BIT_UNKNOWN, 0, nq.BIT_FREE, nq.BIT_ABSENT, 15)]
    # a ray of exactly max_steps voxels and one of max_steps + 1: 1 + 6 + 2 + 1 = 10 voxels
    exact = [ray(o, (3.0, 1.0, 0.5))]
    c.rays += [rays_of(exact, 0, 10), rays_of(exact, 0, 9), rays_of(exact, 0, 11), rays_of(exact, nq.BIT_OCCUPIED, 10), rays_of(exact, nq.BIT_OCCUPIED, 9),
               rays_of([ray(o, o)], 0, 1)]
    return c


def look_along_x(yaw=0.0, t=(-1.5, 0.0, 0.0)):
    """camera z (forward) -> map x, camera x (right) -> map -y, camera y (down) -> map -z, then a turn about the map's z"""
    R0 = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ R0
    return np.concatenate([R, np.array(t, np.float64).reshape(3, 1)], axis=1).astype(F32)


def view(pose, rows, cols, z_far, stop_mask=nq.BIT_OCCUPIED):
    return dict(pose=pose, fx=0.8 * cols, fy=0.8 * cols, cx=(cols - 1) / 2.0, cy=(rows - 1) / 2.0, rows=rows, cols=cols, z_far=z_far, stop_mask=stop_mask)


def room():
    """a small room: a floor plane at z = -1, a box on it, a wall at x = 2; 469 hits on voxel centres, no beam samples"""
    cfg = np_bki.Config(resolution=0.25, num_classes=3, prior=0.0, free_resolution=1e4)
    g = np.arange(-2.0, 2.01, 0.25)
    floor = [[x, y, -1.0] for x in g for y in g]
    box = [[x, y, z] for x in (0.5, 0.75, 1.0) for y in (-0.25, 0.0, 0.25) for z in (-0.75, -0.5, -0.25)]
    back = [[2.0, y, z] for y in g for z in np.arange(-0.75, 1.01, 0.25)]
    rng = np.random.default_rng(10)
    xyz = np.array(floor + box + back, F32)
    feat, _ = bc.rows(rng, len(xyz), 0)
    label = np.zeros((len(xyz), 3), F32)
    label[:len(floor), 0], label[len(floor):len(floor) + len(box), 1], label[len(floor) + len(box):, 2] = 1, 1, 1
    label += rng.uniform(0, 0.2, label.shape).astype(F32)
    frames = [(xyz, feat, label, f32(-1.5, 0.0, 0.0))]
    turned = look_along_x(0.2, (-1.5, 0.125, 0.1))
    views = [view(look_along_x(), 1, 1, 6.0), view(look_along_x(), 8, 8, 6.0), view(turned, 7, 9, 6.0), view(turned, 48, 64, 6.0),
             view(turned, 48, 64, 2.0),                                      # z_far short of the wall: only floor and box stop a ray
             view(look_along_x(), 7, 9, 6.0, nq.BIT_OCCUPIED | nq.BIT_ABSENT),  # every ray stops where the stored voxels end
             view(look_along_x(3.0), 8, 8, 6.0)]                             # turned away from box and wall
    rng = np.random.default_rng(12)
    return Case(cfg, frames, points=np.concatenate([xyz[::5], rng.uniform(-2, 2, (30, 3)).astype(F32)]), views=views)


def all_cases():
    out = {
        "empty": Case(np_bki.Config(resolution=0.5, num_classes=3), points=[[0, 0, 0], [1.25, -1.0, 3.0], [np.nan, 0, 0]],
                      rays=[rays_of([ray((0, 0, 0), (2, 1, 0)), ray((0, 0, 0), (0, 0, 0))], m) for m in (nq.BIT_OCCUPIED, nq.BIT_ABSENT)],
                      views=[view(look_along_x(), 8, 8, 3.0)]),
        "empty_prior": Case(np_bki.Config(resolution=0.5, num_classes=0, prior=0.5), points=[[0, 0, 0], [1.25, -1.0, 3.0], [0, -np.inf, 0]],
                            rays=[rays_of([ray((0, 0, 0), (2, 1, 0))], nq.BIT_ABSENT)], views=[view(look_along_x(), 7, 9, 3.0, nq.BIT_ABSENT)]),
        "one_hit_occupied": one_hit(0.7),
        "one_hit_unknown": one_hit(0.8),
        "one_hit_prior0": one_hit(0.7, prior=0.0),
        "faces": faces(),
        "key_range": key_range(),
        "classes_0": scattered(0, 0.0),
        "classes_1": scattered(1, 0.5),
        "classes_19": scattered(19, 0.3),
        "sparse": scattered(3, 0.001, kernel=sp.SPARSE),
        "sparse_prior0": scattered(2, 0.0, kernel=sp.SPARSE, n=30),
        "long_chains": long_chains(),
        "growth_before": growth(1),
        "growth_after": growth(2),
        "wall": wall(),
        "room": room(),
    }
    for n in SIZES:
        out[f"sized_{n}"] = sized(n)
    return out


_CASES, _EXPECTED = {}, {}


def case(name):
    if not _CASES:
        _CASES.update(all_cases())
    return _CASES[name]


def names():
    case("empty")
    return list(_CASES)


def expected(name):
    """dict(map, query, rays [..], views [..]) of the statement: computed once per test session, shared and left unchanged"""
    if name not in _EXPECTED:
        c = case(name)
        m = c.statement_map()
        look = nq.Looker(m)
        _EXPECTED[name] = dict(map=m, query=nq.query(m, c.points), rays=[nq.raycast(m, o, e, mask, steps, look) for o, e, mask, steps in c.rays],
                               views=[nq.render(m, **v) for v in c.views])
    return _EXPECTED[name]


QUERY_FIELDS = ("found", "state", "semantics", "probs", "vars", "feat", "centre")
RAY_FIELDS = ("status", "key", "centre", "t", "steps", "state", "semantics")
VIEW_FIELDS = ("depth", "semantics", "feat", "label")


def raw(a):
    """the bytes of an array: NaN equals NaN, -0.0 differs from 0.0"""
    return np.ascontiguousarray(a).view(np.uint8)


def first_difference(got, want, fields):
    """Names the first element of a result record (or dict) that differs from the statement's, bit for bit; None: equal."""
    for f in fields:
        g = getattr(got, f) if hasattr(got, f) else got[f]
        w = want[f]
        if g is None:
            continue
        g = np.asarray(g)
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{f}: shape / type {g.shape} {g.dtype} against {w.shape} {w.dtype}"
        if g.size and not np.array_equal(raw(g), raw(w)):
            bad = np.flatnonzero((raw(g).reshape(g.size, -1) != raw(w).reshape(w.size, -1)).any(axis=1))[0]
            idx = np.unravel_index(bad, g.shape)
            return f"{f}{list(map(int, idx))}: {g[idx]!r} against the statement's {w[idx]!r}"
    return None


# ---- a library map (unified_cvo_amd.SemanticMap, of either side or of the twin) against the statement ----
def config_kwargs(cfg):
    return dict(cfg.kwargs(), sf2=float(cfg.sf2), ell=float(cfg.ell))


def fill(m, c):
    """the case's frames into the library map m, under the case's kernel"""
    if c.kernel == sp.SPARSE:
        m.set_kernel("sparse")
    for xyz, feat, label, origin in c.frames:
        m.insert((xyz, feat, label), origin=origin)
    return m


def differences(m, name):
    """every query, ray batch and view of the case on the library map m -> [text] of what differs from the statement"""
    c, want, out = case(name), expected(name), []
    d = first_difference(m.query(c.points), want["query"], QUERY_FIELDS)
    if d:
        out.append(f"{name}: query: {d}")
    for j, (o, e, mask, steps) in enumerate(c.rays):
        d = first_difference(m.raycast(o, e, stop=mask, max_steps=steps), want["rays"][j], RAY_FIELDS)
        if d:
            out.append(f"{name}: rays {j} (mask {mask}, max_steps {steps}): {d}")
    for j, v in enumerate(c.views):
        kw = dict(v)
        mask = kw.pop("stop_mask")
        d = first_difference(m.render(stop=mask, **kw), want["views"][j], VIEW_FIELDS)
        if d:
            out.append(f"{name}: view {j} ({v['rows']} x {v['cols']}, z_far {v['z_far']}, mask {mask}): {d}")
    return out
