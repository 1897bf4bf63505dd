"""The statement of the read side of the semantic voxel map (cvo_map_query / _raycast / _render) in numpy, on the tables of
np_bki.Map and np_bki_sparse.Map.  The CPU twin and the kernels of cvo_k_bki_query.h equal it bit for bit.

query is upstream's SemanticBKIOctoMap::search(x, y, z) (block_to_hash_key, bkiblock.cpp:70-84: the key of np_bki.k0_of per
axis - ONE voxel, not the up to 8 closed boxes np_bki.blocks_of gives an inserted hit) with the node's getters restated from
Semantics::get_probs / get_vars / get_features / get_occupied_probs (bkioctree_node.cpp:19-52), get_state and get_semantics
(the max_element of Semantics::update, bkioctree_node.cpp:68) and the default node Semantics() (bkioctree_node.h:27).

Choices where upstream's text pins nothing:
  * semantics of a point without a stored voxel is -1.  Upstream's default node leaves the member uninitialised.
  * "outside": a coordinate that is not finite, or whose k0 leaves [1, 2^20 - 2], is answered by the default node with found = 2
    and a NaN centre.  The inserts refuse such a coordinate; a query only reads, and one bad pixel must not fail a frame.
  * state and semantics of a stored voxel are functions of its ms alone (np_bki.state_of; the first maximum of ms / sum), as
    the read-out's.  Upstream caches both at the node's last update, from the same ms.
  * the ray walk's tie rule: of crossings with equal t the lowest axis goes first.
Departure: raycast is this library's own walk, written for this library; it is NOT upstream's RayCaster and is not compared with
it.  RayCaster (bkioctomap.h:103-226) has no caller upstream, and its text stands against restating it: the diagonal branch
takes three from the step count for two steps (n -= 2, then n--); a ray whose start block is not stored gets n = 0 and sees
nothing; and with xy_error > 0 and xz_error == 0 (or xy_error < 0 and yz_error == 0) none of its four branches applies, the
errors never change, and next() returns the same voxel until n runs out.
Unpinned against upstream's binary: nothing new.  get_probs / get_vars / get_features are the expressions of the translation
unit oracle/bki_upstream_driver.cpp already compiles (bkioctree_node.cpp), read_out and state_of are pinned by test_bki_upstream.py;
what np_bki lists as unpinned stays so.

Every operation below is a single float32 or, where said, float64 operation: no fused multiply-add but the one the pose
applies (transform_point_pose_vec: fma(T0, x, T1 y) + fma(T2, z, T3)), which fma32 computes exactly rounded.
"""
import numpy as np

import np_bki

F32 = np.float32
KOFF = np_bki.KOFF
ABSENT, FOUND, OUTSIDE = 0, 1, 2
BIT_FREE, BIT_OCCUPIED, BIT_UNKNOWN, BIT_ABSENT = 1, 2, 4, 8
RAY_END, RAY_STOPPED, RAY_TOO_LONG, RAY_OUTSIDE = 0, 1, 2, 3
MAX_STEPS = 1 << 20
MAX_PIXELS = 1 << 24
NO_KEY = np.uint64(2**64 - 1)
NAN = np.uint32(0x7FC00000).view(F32)  # the one NaN the read side writes


def fma32(a, x, c):
    """float32(a * x + c) with ONE rounding, elementwise: the double product is exact, the double sum's error is recovered
    (two-sum), and a sum that sits on a float32 tie is moved off it in the error's direction before the cast."""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(x, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def move(T, xyz):
    """transform_point_pose_vec per row: fma(T0, x, T1 * y) + fma(T2, z, T3), float32"""
    T = np.asarray(T, F32)[:3, :4]
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out = np.empty_like(xyz)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            out[:, r] = fma32(T[r, 0], xyz[:, 0], T[r, 1] * xyz[:, 1]) + fma32(T[r, 2], xyz[:, 2], T[r, 3])
    return out


def key_of(p, size):
    """the key of a point's voxel, or None ("outside")"""
    ks = []
    for a in range(3):
        with np.errstate(all="ignore"):
            k = np_bki.k0_of(p[a], size)  # (NaN and infinity fail both comparisons)
        if k is None:
            return None
        ks.append(k)
    return (ks[0] << 40) | (ks[1] << 20) | ks[2]


def centre_of(key, size):
    if key is None:
        return np.array([NAN, NAN, NAN], F32)
    return np.array([F32((key >> 40) - KOFF) * size, F32(((key >> 20) & 0xFFFFF) - KOFF) * size, F32((key & 0xFFFFF) - KOFF) * size], F32)


def fsum(ms):
    s = F32(0)
    for m in ms:
        s = F32(s + m)
    return s


def node(m, key):
    """(stored, state, semantics, probs, vars, feat, occupied_probs) of the voxel `key` (None: outside) of the statement map m"""
    cfg = m.cfg
    v = m.voxels.get(key) if key is not None else None
    if v is None:
        ms, fs = np.full(m.nclass, cfg.prior, F32), np.zeros(5, F32)
    else:
        ms, fs = v
    tot, occ = fsum(ms), fsum(ms[1:])
    with np.errstate(all="ignore"):
        probs = ms / tot
        vars_ = (probs - probs * probs) / F32(tot + F32(1))
        feat = fs / occ
    if v is None:
        return False, np_bki.UNKNOWN, -1, probs, vars_, feat, probs[1:]
    best = 0
    for c in range(1, m.nclass):  # max_element: the first maximum; a NaN never wins
        if probs[c] > probs[best]:
            best = c
    return True, np_bki.state_of(cfg, ms), best, probs, vars_, feat, probs[1:]


def query(m, xyz):
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    out = dict(found=np.zeros(n, np.uint8), state=np.zeros(n, np.uint8), semantics=np.zeros(n, np.int32), probs=np.zeros((n, m.nclass), F32),
               vars=np.zeros((n, m.nclass), F32), feat=np.zeros((n, 5), F32), centre=np.zeros((n, 3), F32))
    for i in range(n):
        key = key_of(xyz[i], m.cfg.resolution)
        stored, state, sem, probs, vars_, feat, _ = node(m, key)
        out["found"][i] = OUTSIDE if key is None else (FOUND if stored else ABSENT)
        out["state"][i], out["semantics"][i] = state, sem
        out["probs"][i], out["vars"][i], out["feat"][i], out["centre"][i] = probs, vars_, feat, centre_of(key, m.cfg.resolution)
    return out


class Looker:
    """the stop-mask bit of a voxel, each computed once"""

    def __init__(self, m):
        self.m, self.bits = m, {}

    def __call__(self, key):
        b = self.bits.get(key)
        if b is None:
            v = self.m.voxels.get(key)
            b = BIT_ABSENT if v is None else 1 << np_bki.state_of(self.m.cfg, v[0])
            self.bits[key] = b
        return b


def crossing_t(k0, s, i, res, o, e):
    """t of the i-th crossing on one axis, in double (Python floats), one rounding per operation"""
    b = (float(k0 - KOFF) + float(s) * (float(i) - 0.5)) * res
    return (b - o) / (e - o)


def walk(size, o, e, stop_mask, max_steps, look):
    """The voxels of the segment o -> e, face by face -> (status, steps, key or None, t as a double).  Exactly
    1 + N[x] + N[y] + N[z] voxels; each step crosses the axis with crossings left whose next t is smallest, ties to the lowest axis."""
    k0, k1 = [], []
    for a in range(3):
        with np.errstate(all="ignore"):
            ka, kb = np_bki.k0_of(o[a], size), np_bki.k0_of(e[a], size)
        if ka is None or kb is None:
            return RAY_OUTSIDE, 0, None, 0.0
        k0.append(ka)
        k1.append(kb)
    N = [abs(k1[a] - k0[a]) for a in range(3)]
    s = [(k1[a] > k0[a]) - (k1[a] < k0[a]) for a in range(3)]
    total = 1 + sum(N)
    if total > max_steps:
        return RAY_TOO_LONG, 0, None, 0.0
    res, od, ed = float(size), [float(v) for v in o], [float(v) for v in e]
    i, k = [1, 1, 1], list(k0)
    tn = [crossing_t(k0[a], s[a], 1, res, od[a], ed[a]) if N[a] else 0.0 for a in range(3)]
    t = 0.0
    for step in range(1, total + 1):
        key = (k[0] << 40) | (k[1] << 20) | k[2]
        if look(key) & stop_mask:
            return RAY_STOPPED, step, key, t
        if step == total:
            break
        a = -1
        for q in range(3):
            if i[q] <= N[q] and (a < 0 or tn[q] < tn[a]):
                a = q
        k[a] += s[a]
        t = tn[a]
        i[a] += 1
        if i[a] <= N[a]:
            tn[a] = crossing_t(k0[a], s[a], i[a], res, od[a], ed[a])
    return RAY_END, total, key, t


def visited(size, o, e):
    """the keys the walk visits, in order (no map, no stop): what the property test examines"""
    keys = []
    walk(size, o, e, 1, MAX_STEPS, lambda key: keys.append(key) or 0)
    return keys


def raycast(m, origin, end, stop_mask, max_steps, look=None):
    origin, end = np.asarray(origin, F32).reshape(-1, 3), np.asarray(end, F32).reshape(-1, 3)
    n = origin.shape[0]
    look = look or Looker(m)
    out = dict(status=np.zeros(n, np.uint8), key=np.full(n, NO_KEY, np.uint64), centre=np.zeros((n, 3), F32), t=np.zeros(n, F32),
               steps=np.zeros(n, np.int32), state=np.zeros(n, np.uint8), semantics=np.zeros(n, np.int32), td=np.zeros(n, np.float64))
    for i in range(n):
        status, steps, key, t = walk(m.cfg.resolution, origin[i], end[i], stop_mask, max_steps, look)
        _, state, sem, _, _, _, _ = node(m, key)
        out["status"][i], out["steps"][i], out["t"][i], out["td"][i] = status, steps, F32(t), t
        out["key"][i] = NO_KEY if key is None else np.uint64(key)
        out["centre"][i], out["state"][i], out["semantics"][i] = centre_of(key, m.cfg.resolution), state, sem
    return out


def pixel_rays(pose, fx, fy, cx, cy, rows, cols, z_far):
    """(origin, end) rows x cols x 3 of a rendered view: the camera-frame end point (((u - cx) / fx) z_far, ((v - cy) / fy) z_far,
    z_far) in float32, each operation on its own, moved by the pose; the origin is the pose's translation"""
    T = np.asarray(pose, F32)[:3, :4]
    fx, fy, cx, cy, z_far = F32(fx), F32(fy), F32(cx), F32(cy), F32(z_far)
    v, u = np.meshgrid(np.arange(rows, dtype=F32), np.arange(cols, dtype=F32), indexing="ij")
    cam = np.stack([((u - cx) / fx) * z_far, ((v - cy) / fy) * z_far, np.full((rows, cols), z_far, F32)], axis=-1).astype(F32)
    end = move(T, cam.reshape(-1, 3)).reshape(rows, cols, 3)
    origin = np.broadcast_to(T[:, 3], (rows, cols, 3)).astype(F32)
    return origin, end


def render(m, pose, fx, fy, cx, cy, rows, cols, z_far, stop_mask):
    C = m.cfg.num_classes
    origin, end = pixel_rays(pose, fx, fy, cx, cy, rows, cols, z_far)
    look = Looker(m)
    out = dict(depth=np.zeros((rows, cols), F32), semantics=np.full((rows, cols), -1, np.int32), feat=np.zeros((rows, cols, 5), F32),
               label=np.zeros((rows, cols, C), F32))
    zf = float(F32(z_far))
    for v in range(rows):
        for u in range(cols):
            status, _, key, t = walk(m.cfg.resolution, origin[v, u], end[v, u], stop_mask, MAX_STEPS, look)
            if status != RAY_STOPPED:
                continue
            _, _, sem, _, _, feat, occupied = node(m, key)
            out["depth"][v, u] = F32(t * zf)  # (one double product, one cast)
            out["semantics"][v, u], out["feat"][v, u], out["label"][v, u] = sem, feat, occupied[:C]
    return out
