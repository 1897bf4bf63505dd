"""Source / target clouds whose association is known in closed form, with every row placed on a chosen candidate count.

The association kernels change path at fixed row sizes: six ELL entries parked in LDS (k_assoc), sorting networks of 8 /
16 / 32 / 64 (k_list), the list capacities ASSOC_CAP32 / ASSOC_CAP16, 128-candidate steps (k_assoc_dense), wide rows of
257 .. 1216 candidates, the long-list limit LONG_CAP = 1024, 16- vs 32-bit candidate indices at M = 65536, and the
first-K truncation.  Random clouds seldom put a row exactly on one of those limits; these clouds do it on purpose.

Construction (geometry only; the colour variant adds features that always pass the colour cut-off):
  * source row i sits on a cubic grid of spacing 4 r_max, where r_i is its geometric cut-off radius at `ell`
    (a_ij = sigma^2 exp(-d^2 / 2 l_i^2) > sp_thres  <=>  d^2 < -2 l_i^2 ln(sp_thres / sigma^2)) with the range-scaled
    lengthscale l_i = (|x_i| / 500 + 1) ell that np_reference.kernel_matrix (and the oracle's compute_range_ell) uses;
  * row i owns a cluster of exactly c_i targets, inside a ball of radius 0.45 r_i around x_i;
  * every other target is at least 3 r_max away from every source row (other rows' clusters sit on other grid nodes;
    the padding targets far above the grid), so no skin or rounding slack of k_scan turns it into a candidate.
At iteration 0 with the identity pose a row's candidates are its hits, both exactly its cluster, and its ELL row is its
cluster's targets in ascending original index, cut to the first K.
"""
import math

import numpy as np

from unified_cvo_amd import CvoPointCloud

FD = 5            # colour channels of the FEAT_COL instantiations (config 3)
CLUSTER_FRAC = 0.45  # cluster radius / row cut-off radius (<= 0.5: far inside the cut-off, whatever the float rounding)


def cutoff_factor(P):
    """r / l: a_ij > sp_thres  <=>  d^2 < -2 l^2 ln(sp_thres / sigma^2) (geometry only)."""
    sp = float(np.float32(P.sp_thres))
    s2 = float(np.float32(P.sigma)) ** 2
    return math.sqrt(-2.0 * math.log(sp / s2))


def range_ell(x, ell):
    """(|x| / 500 + 1) ell per row, float64 (np_reference.kernel_matrix line 17)."""
    return (np.linalg.norm(np.asarray(x, np.float64), axis=1) / 500.0 + 1.0) * ell


class RowCloud:
    """A built pair: src (N, 3) / tgt (M, 3) float32, optional colour features, and members[i] = the ascending original
    target indices of row i's cluster."""

    def __init__(self, P, ell, src, tgt, members, fsrc=None, ftgt=None):
        self.P, self.ell = P, ell
        self.src, self.tgt = src, tgt
        self.fsrc, self.ftgt = fsrc, ftgt
        self.members = members
        self.counts = np.array([len(m) for m in members], np.int64)

    @property
    def N(self):
        return self.src.shape[0]

    @property
    def M(self):
        return self.tgt.shape[0]

    def clouds(self):
        """(source, target) CvoPointClouds."""
        if self.fsrc is None:
            return CvoPointCloud.from_xyz(self.src), CvoPointCloud.from_xyz(self.tgt)
        geo_s = np.tile(np.array([[0.0, 1.0]], np.float32), (self.N, 1))
        geo_t = np.tile(np.array([[0.0, 1.0]], np.float32), (self.M, 1))
        return (CvoPointCloud.from_arrays(self.src, self.fsrc, None, geo_s),
                CvoPointCloud.from_arrays(self.tgt, self.ftgt, None, geo_t))

    def radius(self):
        return range_ell(self.src, self.ell) * cutoff_factor(self.P)

    def values(self, i):
        """float64 kernel values of row i's cluster, in ascending original index."""
        P = self.P
        j = self.members[i]
        x = self.src[i].astype(np.float64)
        y = self.tgt[j].astype(np.float64)
        l = range_ell(x[None], self.ell)[0]
        a = float(np.float32(P.sigma)) ** 2 * np.exp(-((y - x) ** 2).sum(1) / (2.0 * l * l))
        if self.fsrc is not None:
            c2 = float(np.float32(P.c_ell)) ** 2
            cs2 = float(np.float32(P.c_sigma)) ** 2
            d2c = ((self.ftgt[j].astype(np.float64) - self.fsrc[i].astype(np.float64)) ** 2).sum(1)
            a = a * cs2 * np.exp(-d2c / (2.0 * c2))
        return a

    def closed_form(self, K):
        """(nonzeros, ind [N, K] -1 padded, mat [N, K] float64 0 padded) of the first-K association at identity."""
        nz = np.minimum(self.counts, K).astype(np.uint32)
        ind = np.full((self.N, K), -1, np.int64)
        mat = np.zeros((self.N, K), np.float64)
        for i, m in enumerate(self.members):
            k = min(len(m), K)
            if k:
                ind[i, :k] = m[:k]
                mat[i, :k] = self.values(i)[:k]
        return nz, ind, mat

    def inner_product(self, K):
        """Sum over rows of their first K kernel values (float64)."""
        return float(sum(self.values(i)[:K].sum() for i in range(self.N) if self.counts[i]))

    def csr(self, K):
        """(row_ptr, col) of the first-K association."""
        nz = np.minimum(self.counts, K)
        rp = np.concatenate([[0], np.cumsum(nz)]).astype(np.int64)
        col = np.concatenate([m[:K] for m in self.members] + [np.zeros(0, np.int64)]).astype(np.int64)
        return rp, col


def build(P, counts, ell=None, n_rows=None, n_targets=None, low_rows=(), seed=0, colour=False):
    """A RowCloud whose row i (in the given order; the source cloud's original order is shuffled with `seed`) owns
    counts[i] targets.

    n_rows: pad with rows that have no hits up to this N.  n_targets: pad with far-away targets up to this M.
    low_rows: rows (indices into `counts`) whose hits take the lowest original target indices, in that order; every other
    target gets a seeded shuffled index.  colour: 5-channel features within a few hundredths of one common colour (the
    colour kernel then keeps every geometric hit: see the module docstring)."""
    ell = float(P.ell_init if ell is None else ell)
    rs = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    N = max(len(counts), n_rows or 0)
    counts = counts + [0] * (N - len(counts))
    # grid of spacing 4 r_max: r_max at the grid's largest |x| (range ell grows with |x|)
    g = max(1, int(math.ceil(N ** (1.0 / 3.0))))
    r0 = ell * cutoff_factor(P)
    s = 4.0 * r0 * 1.25
    node = np.stack(np.unravel_index(np.arange(N), (g, g, g)), axis=1).astype(np.float64)
    x = (node - (g - 1) / 2.0) * s
    x[:, 2] += 2.0
    x = x.astype(np.float32)
    r = range_ell(x, ell) * cutoff_factor(P)
    assert r.max() <= 1.25 * r0, "grid too wide for its spacing"
    clusters = []
    for i, c in enumerate(counts):
        d = rs.normal(size=(c, 3))
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
        rad = CLUSTER_FRAC * r[i] * rs.random(c) ** (1.0 / 3.0)
        clusters.append((x[i].astype(np.float64) + d * rad[:, None]).astype(np.float32))
    n_hit = sum(counts)
    M = max(n_hit, n_targets or 0)
    pad = np.zeros((M - n_hit, 3), np.float32)
    if M > n_hit:  # far above the grid: a slab 1000 away
        pad = np.stack([rs.uniform(-50, 50, M - n_hit), rs.uniform(-50, 50, M - n_hit),
                        rs.uniform(1000, 1100, M - n_hit)], axis=1).astype(np.float32)
    owner = np.concatenate([np.full(c, i, np.int64) for i, c in enumerate(counts)] + [np.full(M - n_hit, -1, np.int64)])
    built = np.concatenate(clusters + [pad]) if M else np.zeros((0, 3), np.float32)
    # original target indices: low_rows first, the rest shuffled
    first = np.concatenate([np.flatnonzero(owner == i) for i in low_rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    rest = np.setdiff1d(np.arange(M), first)
    order = np.concatenate([first, rest[rs.permutation(len(rest))]])  # order[new] = built index
    tgt = built[order]
    owner_new = owner[order]
    members = [np.zeros(0, np.int64)] * N
    idx = np.argsort(owner_new, kind="stable")
    bounds = np.searchsorted(owner_new[idx], np.arange(-1, N + 1))
    for i in range(N):
        members[i] = np.sort(idx[bounds[i + 1]:bounds[i + 2]])
    # the source's original order: shuffled (the device orders rows spatially; count blocks stay spatially contiguous)
    sperm = rs.permutation(N)
    src = x[sperm]
    members = [members[k] for k in sperm]
    fsrc = ftgt = None
    if colour:
        base = np.array([0.5, 0.4, 0.6, 0.45, 0.55], np.float32)
        fsrc = (base + rs.uniform(-0.02, 0.02, (N, FD))).astype(np.float32)
        ftgt = (base + rs.uniform(-0.02, 0.02, (M, FD))).astype(np.float32)
    return RowCloud(P, ell, src, tgt, members, fsrc, ftgt)


def foreign_distance(rc):
    """min over rows i of (distance from x_i to the nearest target NOT in its cluster) / r_i, evaluated in row chunks."""
    own = np.full(rc.M, -1, np.int64)
    for i, m in enumerate(rc.members):
        own[m] = i
    y = rc.tgt.astype(np.float64)
    r = rc.radius()
    best = np.inf
    for a in range(0, rc.N, 256):
        x = rc.src[a:a + 256].astype(np.float64)
        d2 = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T
        d2[own[None, :] == np.arange(a, a + x.shape[0])[:, None]] = np.inf
        d = np.sqrt(np.maximum(d2.min(axis=1), 0.0)) if rc.M else np.full(x.shape[0], np.inf)
        best = min(best, float((d / r[a:a + 256]).min()))
    return best


# --- the families --------------------------------------------------------------------------------------------------
LIST_VALUES = (0, 1, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
OVERFLOW_VALUES = (127, 128, 129, 255, 256, 257, 304, 305, 384, 385, 1023, 1024, 1025, 1215, 1216, 1217, 2000)
WIDE_M = (1024, 1025, 1100, 1216, 1217)


def list_family(P, seed=1, colour=False, ell=None):
    """64 rows on each list class (a whole wave, and with the spatial sort a 256-row window, on one value): 6 entries in
    LDS, sorting networks 8 / 16 / 32 / 64, ASSOC_CAP32 = 32 and ASSOC_CAP16 = 64 (rows of 65 overflow)."""
    return build(P, [c for c in LIST_VALUES for _ in range(64)], ell=ell, seed=seed, colour=colour)


def overflow_family(P, seed=2, colour=False, ell=None):
    """Two rows on each overflow class: 128-candidate steps of k_assoc_dense, WIDE_MIN = 256, WIDE_CAP = 304 per quarter,
    LONG_CAP = 1024 (rows beyond it are scanned literally), 1216 = 4 x WIDE_CAP, and one row well above; 64 empty rows."""
    return build(P, [c for c in OVERFLOW_VALUES for _ in range(2)], ell=ell, n_rows=98, seed=seed, colour=colour)


def wide_family(P, M, low=True, seed=3):
    """A lone small pair (N = 16) with M targets, M around LONG_CAP / 4 x WIDE_CAP: one big row (all targets but 24, or
    all of them when that leaves it within LONG_CAP), its hits either on the lowest original indices (a full first
    quarter of the wide phase) or shuffled, plus a row of the rest."""
    big = M - 24 if M - 24 > 1024 else (1000 if M <= 1024 else M)
    counts = [big, M - big] + [0] * 14
    return build(P, counts, n_targets=M, low_rows=(0,) if low else (), seed=seed)


def dense_family(P, M=1100, seed=4):
    """More than half of 16 rows overflow and M <= 2048: the pair enters the dense regime (cvo_update.h: 2 c_ovf > N and
    M <= 2048), where every row is evaluated over all M targets (the wide phase at 1025 <= M <= 1216).  Row 0 has 400
    hits on the lowest original indices."""
    return build(P, [400] + [70] * 8 + [0] * 7, n_targets=M, low_rows=(0,), seed=seed)


def bits_family(P, M, seed=5):
    """Rows of 20 .. 100 candidates (and two beyond LONG_CAP) padded to M targets: M = 65535 keeps 16-bit candidate lists
    (capacity ASSOC_CAP16 = 64, long lists on), M = 65536 switches to 32-bit lists (ASSOC_CAP32 = 32, no long lists)."""
    return build(P, [c for c in (20, 32, 33, 48, 64, 65, 100) for _ in range(8)] + [1100, 1100], n_rows=96,
                 n_targets=M, seed=seed)


def score_family(P, seed=6):
    """Clusters of 3 .. 200 targets (several 64-target tiles each) for the inner-product limits around c_max = 200."""
    return build(P, [c for c in (3, 70, 150, 200) for _ in range(4)], n_rows=40, seed=seed)
