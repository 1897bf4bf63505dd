"""The statement of one insert into the semantic voxel map under the SPARSE kernel (cvo_map_set_kernel(map, CVO_MAP_KERNEL_SPARSE)),
in numpy, at block_depth 1.  Restated from semantic_bki::SemanticBKInference::predict and covSparse (bki.h:51-78, 153-166),
get_extended_block (bkiblock.cpp:86-113), Semantics::update (bkioctree_node.cpp:54-79) and the insert_pointcloud declaration
bkioctomap.h:94 keeps commented out.  Everything the two kernels share - the training data, the blocks of a point, the state and
the read-out - is np_bki's; a map may take inserts of either kernel in any order (Map.kernel).  The CPU twin and the kernels of
cvo_k_bki_sparse.h equal this bit for bit.

Training blocks: as under the counting kernel, a training point belongs to the 1 - 8 blocks whose closed float box holds it; a
block's training list is its members in training_data's order (hits, each followed by its beam samples, the origin last).
Test voxels: every touched block and every face neighbour of one (upstream's get_blocks_in_bbox pads the bounding box by a
block on each side, so all of them are enumerated).  A test voxel that was not in the map is created with ms = prior, fs = 0
and STORED, even if every weight it receives is zero - unlike the counting insert (np_bki), which does not store blocks that
only have a neighbour with points.
Per test voxel: the neighbour slots j = 0 .. 6 in get_extended_block's order (self, +x, -x, +y, -y, +z, -z); for every slot whose
block has training points ybar[c] is the float sum from 0, in ascending training order, of k(v, p) over the block's points of
class c, fbar[f] the float sum of F32(k * feat[hit][f]) over its hits in the same order (feature rows given), then ms += ybar
and fs += fbar - one float add per component per slot, in slot order: upstream's one node.update per neighbour block.  A point
on a shared face is in both blocks' lists and votes through both slots, as upstream's boxes make it.

The weight k(v, p): sparse_k below.  sin and cos are this module's own routine (sincos) - numpy's, glibc's and the device
library's would not agree bit for bit - which the twin and the kernel repeat operation for operation.

Choices where upstream's text pins nothing:
  * the order inside a block's sum: ascending training order (upstream's is an Eigen product over its R-tree's traversal);
  * squaredNorm's order: x, y, z, left to right.
Extensions:
  * fbar: predict has no feature product; predict_csm's Ks * f is carried over to the sparse weights.
  * num_classes = 0, as np_bki: every hit is class 1 of a two-class map.
  * a neighbour slot whose block index would leave the key's 20-bit field ([0, 2^20 - 1]) does not exist.  Points are confined
    to k0 in [1, 2^20 - 2]; only a point exactly on the outermost face of that range has a block with such a neighbour.
Unpinned: all of it against upstream's binary, because bki.h needs Eigen.  get_extended_block itself lives in bkiblock.cpp,
which the oracle recipe compiles, but that recipe is not extended here, so the slot order is not pinned either.
Caps: np_bki's, and MAX_RECORDS memberships in one insert (the device sorts one work record per membership); an insert with
that many or more is refused as unsupported before anything is written.

Every operation is a single float32 numpy operation: no fused multiply-add.
"""
import numpy as np

import np_bki
from np_bki import F32, KOFF, Refused

CSM, SPARSE = 0, 1
MAX_RECORDS = 1 << 24
SLOTS = 7
PI = F32(3.1415926)  # upstream's constant
FAR = F32(1.5)       # from here on the weight is 0 without being evaluated: the expression is below -0.0075 there

# the reduction a - q pi/2: pi/2 in three pieces, the first two short enough that q * piece is exact for q <= 6
TWO_OVER_PI = F32(0.63661977)
P1, P2, P3 = F32(1.5703125), F32(4.837512969970703125e-4), F32(7.54978995489188216e-8)
S1, S2, S3 = F32(-1.9515295891e-4), F32(8.3321608736e-3), F32(-1.6666654611e-1)
C1, C2, C3 = F32(2.443315711809948e-5), F32(-1.388731625493765e-3), F32(4.166664568298827e-2)


def sincos(a):
    """(sin a, cos a) of float32 a in [0, 3 pi), scalars or arrays: the quarter turn q = int(a * 2/pi + 0.5) (truncated), r = a - q pi/2
    in three subtractions, a polynomial each in z = r * r by Horner's rule, the quadrant's swap and signs."""
    a = np.asarray(a, F32)
    q = (a * TWO_OVER_PI + F32(0.5)).astype(np.int32)
    fq = q.astype(F32)
    r = a - fq * P1
    r = r - fq * P2
    r = r - fq * P3
    z = r * r
    ps = ((S1 * z + S2) * z + S3) * z * r + r
    pc = ((C1 * z + C2) * z + C3) * z * z - F32(0.5) * z + F32(1.0)
    odd = (q & 1) != 0
    s0, c0 = np.where(odd, pc, ps), np.where(odd, ps, pc)
    return np.where((q & 2) != 0, -s0, s0).astype(F32), np.where(((q + 1) & 2) != 0, -c0, c0).astype(F32)


def weight_of_distance(d, sf2=F32(1)):
    """covSparse of float32 distances d (in units of ell), scalars or arrays"""
    d = np.asarray(d, F32)
    near = d < FAR
    dn = np.where(near, d, F32(0))
    a = dn * F32(2) * PI
    s, c = sincos(a)
    k = ((F32(2) + c) * (F32(1) - dn) / F32(3) + s / (F32(2) * PI)) * F32(sf2)
    k = np.where(k < 0, F32(0), k)
    return np.where(near, k, F32(0)).astype(F32)


def distance(centre, pts, ell):
    """|centre / ell - p / ell| of the (3,) centre to the (n, 3) points: the squares summed left to right, a float sqrt"""
    e = (centre / ell)[None, :] - pts / ell
    sq = e * e
    return np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def sparse_k(centre, pts, sf2, ell):
    return weight_of_distance(distance(np.asarray(centre, F32), np.asarray(pts, F32).reshape(-1, 3), F32(ell)), F32(sf2))


def centre_of(key, size):
    return np.array([F32((key >> 40) - KOFF) * size, F32(((key >> 20) & 0xFFFFF) - KOFF) * size, F32((key & 0xFFFFF) - KOFF) * size], F32)


def slot_key(key, j):
    """the block in neighbour slot j of `key` (get_extended_block's order), or None where the index leaves its 20-bit field"""
    if j == 0:
        return key
    shift = 40 - 20 * ((j - 1) // 2)
    k = ((key >> shift) & 0xFFFFF) + (1 if j % 2 == 1 else -1)
    if k < 0 or k > 0xFFFFF:
        return None
    return (key & ~(0xFFFFF << shift)) | (k << shift)


def float_sum(values):
    """sequential float32 sum from 0"""
    if len(values) == 0:
        return F32(0)
    return np.add.accumulate(np.concatenate([np.zeros(1, F32), np.asarray(values, F32)]), dtype=F32)[-1]


def check_kernel(cfg, kernel):
    if kernel not in (CSM, SPARSE):
        raise Refused("invalid", "kernel")
    if kernel == SPARSE:
        for v in (cfg.sf2, cfg.ell):
            if not np.isfinite(F32(v)) or not F32(v) > 0:
                raise Refused("invalid", "sf2 / ell")


class Map(np_bki.Map):
    """np_bki.Map with a kernel: CSM inserts as np_bki.Map, SPARSE as this module states."""

    def __init__(self, cfg, kernel=CSM):
        super().__init__(cfg)
        self.kernel = CSM
        self.set_kernel(kernel)

    def set_kernel(self, kernel):
        check_kernel(self.cfg, kernel)
        self.kernel = kernel

    def insert(self, xyz, feat, label, origin):
        if self.kernel == CSM:
            return super().insert(xyz, feat, label, origin)
        cfg, size = self.cfg, self.cfg.resolution
        sf2, ell = F32(cfg.sf2), F32(cfg.ell)
        feat = None if feat is None else np.asarray(feat, F32).reshape(-1, 5)
        label = None if label is None else np.asarray(label, F32)
        if cfg.num_classes > 0 and label is None and np.asarray(xyz).size:
            raise Refused("invalid", "a map with classes needs label rows")
        pts = np_bki.training_data(cfg, xyz, label, origin)
        lists = {}  # key -> training indices, ascending
        members = 0
        for t, (p, cls, hit) in enumerate(pts):
            keys = np_bki.blocks_of(p[0], p[1], p[2], size)
            if keys is None:
                raise Refused("invalid", "block index out of range")
            members += len(keys)
            for key in keys:
                lists.setdefault(key, []).append(t)
        if members >= MAX_RECORDS:
            raise Refused("unsupported", "work records")
        P = np.array([p for p, _, _ in pts], F32).reshape(len(pts), 3)
        cls = np.array([c for _, c, _ in pts], np.int64)
        hit = np.array([h for _, _, h in pts], np.int64)
        tests = set()
        for key in lists:
            tests.update(k for k in (slot_key(key, j) for j in range(SLOTS)) if k is not None)
        for v in sorted(tests):
            vox = self.voxels.setdefault(v, [np.full(self.nclass, cfg.prior, F32), np.zeros(5, F32)])
            centre = centre_of(v, size)
            for j in range(SLOTS):
                b = slot_key(v, j)
                if b is None or b not in lists:
                    continue
                idx = np.array(lists[b], np.int64)
                k = sparse_k(centre, P[idx], sf2, ell)
                ybar = np.array([float_sum(k[cls[idx] == c]) for c in range(self.nclass)], F32)
                vox[0] = vox[0] + ybar
                if feat is not None:
                    hits = hit[idx] >= 0
                    prod = k[hits][:, None] * feat[hit[idx][hits]]
                    vox[1] = vox[1] + np.array([float_sum(prod[:, f]) for f in range(5)], F32)
        self.last = dict(training=len(pts), members=members, longest_run=max([len(l) for l in lists.values()] + [0]))
