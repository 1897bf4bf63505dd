"""The statement of the semantic voxel map (cvo_map_*): upstream's bki_mapping_lib as its driver main_local_mapping.cpp uses
it, in numpy.  Restated from semantic_bki::SemanticBKIOctoMap::insert_pointcloud_csm, get_training_data, beam_sample,
get_blocks_in_bbox, get_gp_points_in_bbox (bkioctomap.cpp:153-314, 331-389, 418-456), SemanticBKInference::predict_csm and
covCountingSensorModel (bki.h:80-118, 168-170), block_to_hash_key / hash_key_to_block (bkiblock.cpp:70-84),
Semantics::get_occupied_probs / get_features / update (bkioctree_node.cpp:28-79), the State enum (bkioctree_node.h:27) and
CvoPointCloud(const SemanticBKIOctoMap*, num_classes) (bkioctomap.cpp:22-78).  The CPU twin and the kernels equal it bit for bit.

Covered: block_depth = 1, the driver's value - one block is one cell, Block::size = resolution.  The counting-sensor kernel is
all ones, so a block's update is the histogram of the training points inside its box.

Choices where upstream's text pins nothing:
  * fbar of a block is the float sum of its hits' feature rows in ASCENDING HIT INDEX, starting from 0.  Upstream's order is
    its R-tree's traversal order under an Eigen product.
  * The cloud lists the OCCUPIED voxels in ASCENDING KEY order.  Upstream walks an unordered_map.
  * max_range compares the DOUBLE square root of the float sum of squares (upstream's unqualified sqrt may resolve to the float
    or the double overload; only a hit within one float ulp of the bound can tell them apart).
Departures:
  * Every block that holds a training point is updated exactly once per insert.  Upstream enumerates blocks by stepping a
    float across the bounding box, which can in principle skip or repeat a key.
  * Blocks upstream allocates only because a face neighbour has points are not stored: never-updated UNKNOWN leaves, never in
    the cloud.
Extension: num_classes = 0 (upstream's driver is broken for clouds without labels): every hit is class 1 of a two-class map
and the cloud read out has no labels.
Pinned against upstream's own compiled bkiblock.cpp, bkioctree.cpp, bkioctree_node.cpp, point3f.cpp and rtree.h
(oracle/bki_upstream_driver.cpp, tests/golden/bki_upstream.npz, test_bki_upstream.py): k0_of, the centre expression, holds /
blocks_of, state_of, read_out and Map on frames without beam samples - bit for bit, no difference found.  Unpinned, because
their translation unit needs PCL and Eigen: training_data's order and max_range comparison, beam, upstream's enumeration of
blocks (get_blocks_in_bbox), the Eigen products of predict_csm and maxCoeff's choice among equal label maxima.

Every operation below is a single float32 (or, where said, float64) numpy operation: no fused multiply-add.
"""
import numpy as np

F32 = np.float32
KOFF = 524288
FREE, OCCUPIED, UNKNOWN = 0, 1, 2
MAX_TRAINING = 1 << 24
MAX_RAY = 65536


class Refused(Exception):
    """code: "invalid" or "unsupported"."""

    def __init__(self, code, text):
        super().__init__(text)
        self.code = code


class Config:
    def __init__(self, resolution=0.05, block_depth=1, num_classes=0, sf2=1.0, ell=1.0, prior=0.0, var_thresh=1.0, free_thresh=0.65,
                 occupied_thresh=0.9, ds_resolution=-1.0, free_resolution=1.0, max_range=-1.0):
        self.resolution, self.block_depth, self.num_classes = F32(resolution), int(block_depth), int(num_classes)
        self.prior, self.free_thresh, self.occupied_thresh = F32(prior), F32(free_thresh), F32(occupied_thresh)
        self.free_resolution, self.max_range = F32(free_resolution), F32(max_range)
        self.sf2, self.ell, self.var_thresh, self.ds_resolution = sf2, ell, var_thresh, ds_resolution  # change nothing

    def kwargs(self):
        return dict(resolution=float(self.resolution), block_depth=self.block_depth, num_classes=self.num_classes, prior=float(self.prior),
                    free_thresh=float(self.free_thresh), occupied_thresh=float(self.occupied_thresh),
                    free_resolution=float(self.free_resolution), max_range=float(self.max_range))


def check_config(c):
    for v, name in ((c.resolution, "resolution"), (c.free_resolution, "free_resolution")):
        if not np.isfinite(v) or not v > 0:
            raise Refused("invalid", name)
    for v in (c.free_thresh, c.occupied_thresh):
        if not (0 <= v <= 1):
            raise Refused("invalid", "threshold")
    if not np.isfinite(c.prior) or c.prior < 0 or not (0 <= c.num_classes <= 19) or not np.isfinite(c.max_range):
        raise Refused("invalid", "prior / num_classes / max_range")
    if c.block_depth != 1:
        raise Refused("unsupported", "block_depth")


def k0_of(p, size):
    """int64(p / (double)size + 524288.5), or None outside [1, 2^20 - 2]."""
    q = np.float64(p) / np.float64(size) + np.float64(524288.5)
    if not (q >= 1.0 and q < 1048575.0):
        return None
    return int(q)  # (truncation)


def holds(k, p, size):
    c = F32(k - KOFF) * size
    h = size / F32(2.0)
    return bool(F32(c - h) <= p) and bool(p <= F32(c + h))


def axis_blocks(p, size):
    k0 = k0_of(p, size)
    if k0 is None:
        return None
    return [k for k in (k0 - 1, k0, k0 + 1) if holds(k, p, size)]


def blocks_of(x, y, z, size):
    """Keys of the blocks whose closed float box holds the point (0, 1, 2, 4 or 8 of them), or None when a k0 leaves its range."""
    ax, ay, az = axis_blocks(x, size), axis_blocks(y, size), axis_blocks(z, size)
    if ax is None or ay is None or az is None:
        return None
    return [(kx << 40) | (ky << 20) | kz for kx in ax for ky in ay for kz in az]


def dist2(p, o):
    d = p - o  # float32
    return F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))


def beam(p, o, fr):
    """The beam samples of hit p seen from o; Refused when the ray would need MAX_RAY samples or more."""
    l = F32(np.sqrt(dist2(p, o)))
    with np.errstate(all="ignore"):
        if not F32(l / fr) < F32(MAX_RAY):
            raise Refused("unsupported", "ray")
        n = (p - o) / l
    out = []
    d = fr
    while d < l:
        out.append(o + F32(n * d))
        d = F32(d + fr)
    if l > fr:
        out.append(o + F32(n * F32(l - fr)))
    return out


def training_data(cfg, xyz, label, origin):
    """[(point (3,) float32, class, hit index or -1)] in upstream's order; Refused as the library refuses."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    o = np.asarray(origin, F32).reshape(3)
    if not np.all(np.isfinite(xyz)) or not np.all(np.isfinite(o)):
        raise Refused("invalid", "not finite")
    C = cfg.num_classes
    out = []
    for i in range(xyz.shape[0]):
        p = xyz[i]
        if cfg.max_range > 0 and np.sqrt(np.float64(dist2(p, o))) > np.float64(cfg.max_range):
            continue
        cls = 1 + int(np.argmax(label[i])) if C > 0 else 1  # (argmax: the first maximum)
        out.append((p, cls, i))
        out += [(s.astype(F32), 0, -1) for s in beam(p, o, cfg.free_resolution)]
        if len(out) >= MAX_TRAINING:
            raise Refused("unsupported", "training points")
    out.append((o, 0, -1))
    if len(out) >= MAX_TRAINING:
        raise Refused("unsupported", "training points")
    return out


def state_of(cfg, ms):
    s = F32(0)
    for m in ms:
        s = F32(s + m)
    with np.errstate(all="ignore"):
        probs = ms / s
    if int(np.argmax(probs)) == 0:
        return FREE
    p = F32(F32(1) - probs[0])
    return OCCUPIED if p > cfg.occupied_thresh else (FREE if p < cfg.free_thresh else UNKNOWN)


def read_out(ms, fs):
    """(get_features, get_occupied_probs) of a voxel: fs over the float sum of ms[1:], ms[1:] over the float sum of ms"""
    occ, tot = F32(0), F32(0)
    for m in ms[1:]:
        occ = F32(occ + m)
    for m in ms:
        tot = F32(tot + m)
    with np.errstate(all="ignore"):
        return fs / occ, ms[1:] / tot


class Map:
    """voxels: key -> [ms (nclass,) float32, fs (5,) float32]."""

    def __init__(self, cfg):
        check_config(cfg)
        self.cfg = cfg
        self.nclass = max(cfg.num_classes, 1) + 1
        self.voxels = {}
        self.last = {}

    def insert(self, xyz, feat, label, origin):
        cfg, size = self.cfg, self.cfg.resolution
        feat = None if feat is None else np.asarray(feat, F32).reshape(-1, 5)
        label = None if label is None else np.asarray(label, F32)
        if cfg.num_classes > 0 and label is None and np.asarray(xyz).size:
            raise Refused("invalid", "a map with classes needs label rows")
        pts = training_data(cfg, xyz, label, origin)
        touched = {}  # key -> [integer counts, fbar]
        members = 0
        for p, cls, hit in pts:
            keys = blocks_of(p[0], p[1], p[2], size)
            if keys is None:
                raise Refused("invalid", "block index out of range")
            members += len(keys)
            for key in keys:
                t = touched.setdefault(key, [np.zeros(self.nclass, np.int64), np.zeros(5, F32)])
                t[0][cls] += 1
                if hit >= 0 and feat is not None:
                    t[1] = t[1] + feat[hit]  # (ascending hit index: pts is in hit order)
        for key, (counts, fbar) in touched.items():
            v = self.voxels.setdefault(key, [np.full(self.nclass, cfg.prior, F32), np.zeros(5, F32)])
            v[0] = v[0] + counts.astype(F32)
            v[1] = v[1] + fbar
        self.last = dict(training=len(pts), members=members, longest_run=max([int(t[0][1:].sum()) for t in touched.values()] + [0]))

    def table(self):
        """(keys (v,) uint64 ascending, ms (v, nclass), fs (v, 5))."""
        keys = sorted(self.voxels)
        ms = np.array([self.voxels[k][0] for k in keys], F32).reshape(len(keys), self.nclass)
        fs = np.array([self.voxels[k][1] for k in keys], F32).reshape(len(keys), 5)
        return np.array(keys, np.uint64), ms, fs

    def cloud(self):
        """(xyz (n, 3), feat (n, 5), label (n, C)) of the OCCUPIED voxels in ascending key order."""
        cfg, C = self.cfg, self.cfg.num_classes
        xyz, feat, lab = [], [], []
        for key in sorted(self.voxels):
            ms, fs = self.voxels[key]
            if state_of(cfg, ms) != OCCUPIED:
                continue
            xyz.append([F32((key >> 40) - KOFF) * cfg.resolution, F32(((key >> 20) & 0xFFFFF) - KOFF) * cfg.resolution,
                        F32((key & 0xFFFFF) - KOFF) * cfg.resolution])
            f, l = read_out(ms, fs)
            feat.append(f)
            lab.append(l[:C])
        n = len(xyz)
        return (np.array(xyz, F32).reshape(n, 3), np.array(feat, F32).reshape(n, 5), np.array(lab, F32).reshape(n, C))
