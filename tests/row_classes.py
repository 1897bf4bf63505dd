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

With build(feature=...) (FEATURE_KINDS below) the cluster is only the row's geometric CANDIDATES: colour, one-hot or soft
class rows or geometric types make a chosen number of them hits and reject the others, interleaved in original-index order,
every member at least 1e-3 (relative, float64) away from every gate it meets.  Then candidates != hits, and the code that
exists because they differ - slots from ballots and prefix counts, per-quarter compaction, first-K and the void rule counted
on hits, row classes counted on candidates - sees rows where the two sit on different limits.
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


NC = 19           # semantic classes (label rows of 19 floats)
# Feature kinds whose gates REJECT members of a row's cluster (build(feature=...)): the switches and parameters each kind
# sets on a copy of the caller's parameters (the shipped geometry configuration: sp_thres = 6e-4).
#
# Each of the colour / semantic cut-offs is `that kernel > sp_thres` in disguise, so while every other factor is <= 1 a
# kernel that SKIPPED the gate would still drop the pair at `a > sp_thres` and nobody could tell.  The kinds that test a
# gate therefore set sigma = 3: a cluster member's geometric kernel is sigma^2 (sp / sigma^2)^(d / r)^2 with d <= 0.45 r,
# i.e. in [1.28, 9], and a member just beyond a cut-off ('near': its kernel in [sp / 1.2, sp / 1.05]) has a product ABOVE
# sp_thres - only the gate rejects it.  Half of the rejected members are near, half far beyond.
#   colour    c_ell = 0.15, c_sigma = 0.6: d2_c_thres = -2 c_ell^2 ln(sp / c_sigma^2) = 0.288.  Hits at d2_c in
#             [0.002, 0.03]; rejected near at d2_c_thres (1.008 .. 1.02), far at [1, 2];
#   product   sigma = 0.1 (geometric kernel in [5.66e-3, 0.01]), the same colour kernel; rejected members at d2_c in
#             [0.10, 0.25]: inside the colour cut-off, but ck <= 0.039 and the product <= 3.9e-4 < sp_thres: every single
#             gate passes and the product drops them;
#   hot       one-hot classes, s_sigma = 0.8, s_ell = 0.376: d2_s_thres = -2 s_ell^2 ln(sp / s_sigma^2) = 1.971 < 2, another
#             class is rejected (FEAT_HOT: diff_ok is false) although sk_diff = 5.4e-4 times the geometric kernel is above
#             sp_thres;
#   hot_pass  one-hot classes, s_ell = 1: d2_s_thres = 13.9, another class passes with sk = 0.64 e^-1: nothing is rejected
#             and a row carries two distinct semantic kernel values;
#   soft      s_ell = 0.3 (d2_s_thres = 1.255); soft source rows 0.9 e_a + 0.1 e_b, targets (1 - t) p + t e_c: d2_s =
#             1.82 t^2; hits t in [0.08, 0.36], rejected near at d2_s_thres (1.008 .. 1.02), far t in [0.88, 0.98];
#   hot_soft  one-hot source rows e_a, soft targets (1 - t) e_a + t e_c: d2_s = 2 t^2, the same three bands of d2_s; the target
#             cloud is not one-hot, so the call must take FEAT_ALL;
#   geotype   sigma = 1 (geometric kernel >= 0.22); source types s (cos th, sin th); hits parallel or at 15 .. 55 degrees
#             (geo_sim = cos^2 in [0.33, 1], arbitrary lengths); rejected members exactly orthogonal (geo_sim = 0), nearly so
#             (geo_sim in [0.004, 0.008]: a = 0.22 x 0.004 > sp_thres, only `geo_sim < 0.01` rejects them) or, every
#             seventh, of type (0, 0) (0 / 0 = NaN passes `geo_sim < 0.01` and is dropped by `a > sp_thres`).
FEATURE_KINDS = ("colour", "product", "hot", "hot_pass", "soft", "hot_soft", "geotype")
FEATURE_SETTINGS = {
    "colour": dict(sigma=3.0, is_using_intensity=1, c_ell=0.15, c_sigma=0.6),
    "product": dict(sigma=0.1, is_using_intensity=1, c_ell=0.15, c_sigma=0.6),
    "hot": dict(sigma=3.0, is_using_semantics=1, s_ell=0.376, s_sigma=0.8),
    "hot_pass": dict(sigma=3.0, is_using_semantics=1, s_ell=1.0, s_sigma=0.8),
    "soft": dict(sigma=3.0, is_using_semantics=1, s_ell=0.3, s_sigma=0.8),
    "hot_soft": dict(sigma=3.0, is_using_semantics=1, s_ell=0.3, s_sigma=0.8),
    "geotype": dict(sigma=1.0, is_using_geometric_type=1),
}
GATE_ONLY_KINDS = ("colour", "hot", "soft", "hot_soft", "geotype")  # kinds with members that ONLY their gate rejects


def feature_params(P, kind):
    """A copy of P with the switches and cut-off parameters of a rejecting feature kind."""
    import copy
    Q = copy.copy(P)
    Q.is_using_intensity = Q.is_using_semantics = Q.is_using_geometric_type = 0
    for k, v in FEATURE_SETTINGS[kind].items():
        setattr(Q, k, v)
    return Q


def interleaved(c, h):
    """h of c positions, evenly spread (the centres of h equal parts of 0 .. c): for 0 < h < c neither a prefix nor a
    suffix, rejected positions in between."""
    return ((2 * np.arange(h, dtype=np.int64) + 1) * c) // (2 * max(h, 1))


class RowCloud:
    """A built pair: src (N, 3) / tgt (M, 3) float32, optional features, members[i] = the ascending original target
    indices of row i's HITS and cands[i] those of its cluster (its geometric candidates).  Without a rejecting feature
    kind (kind is None) the two are the same."""

    def __init__(self, P, ell, src, tgt, members, fsrc=None, ftgt=None, kind=None, cands=None, lsrc=None, ltgt=None,
                 gsrc=None, gtgt=None):
        self.P, self.ell = P, ell
        self.src, self.tgt = src, tgt
        self.fsrc, self.ftgt = fsrc, ftgt
        self.lsrc, self.ltgt = lsrc, ltgt
        self.gsrc, self.gtgt = gsrc, gtgt
        self.kind = kind
        self.members = members
        self.cands = members if cands is None else cands
        self.counts = np.array([len(m) for m in members], np.int64)
        self.cand_counts = np.array([len(m) for m in self.cands], np.int64)

    @property
    def N(self):
        return self.src.shape[0]

    @property
    def M(self):
        return self.tgt.shape[0]

    def params(self, K=None):
        """A copy of the cloud's parameters (its feature switches and cut-offs included) with nearest_neighbors_max = K."""
        import copy
        Q = copy.copy(self.P)
        if K is not None:
            Q.nearest_neighbors_max = int(K)
        return Q

    def clouds(self):
        """(source, target) CvoPointClouds."""
        if self.fsrc is None and self.lsrc is None and self.gsrc is None:
            return CvoPointCloud.from_xyz(self.src), CvoPointCloud.from_xyz(self.tgt)
        geo_s = np.tile(np.array([[0.0, 1.0]], np.float32), (self.N, 1)) if self.gsrc is None else self.gsrc
        geo_t = np.tile(np.array([[0.0, 1.0]], np.float32), (self.M, 1)) if self.gtgt is None else self.gtgt
        return (CvoPointCloud.from_arrays(self.src, self.fsrc, self.lsrc, geo_s),
                CvoPointCloud.from_arrays(self.tgt, self.ftgt, self.ltgt, geo_t))

    def radius(self):
        return range_ell(self.src, self.ell) * cutoff_factor(self.P)

    def factors(self, i, j=None):
        """float64 arithmetic of row i against the targets j (default: its cluster): dict(a = product of the switched-on
        kernels, hit = every gate passed and a > sp_thres, margin = the smallest relative distance of each target from a
        gate it meets: the geometric / colour / semantic cut-offs, 0.01 on geo_sim, and - for a target that passes all of
        them - sp_thres on the product; a NaN geo_sim is at no finite distance from anything)."""
        P = self.P
        j = self.cands[i] if j is None else j
        sp = float(np.float32(P.sp_thres))
        a = np.ones(len(j))
        ok = np.ones(len(j), bool)
        margin = np.full(len(j), np.inf)

        def cut(d2, thr):
            nonlocal ok, margin
            ok &= d2 < thr
            margin = np.minimum(margin, np.abs(d2 - thr) / thr)

        if P.is_using_geometric_type:
            ga, gb = self.gsrc[i].astype(np.float64), self.gtgt[j].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                gs = (gb @ ga) ** 2 / ((ga * ga).sum() * (gb * gb).sum(1))
            ok &= ~(gs < 0.01)
            margin = np.minimum(margin, np.where(np.isnan(gs), np.inf, np.abs(gs - 0.01) / 0.01))
            a = a * gs
        if P.is_using_geometry:
            x = self.src[i].astype(np.float64)
            l = range_ell(x[None], self.ell)[0]
            s2 = float(np.float32(P.sigma)) ** 2
            d2 = ((self.tgt[j].astype(np.float64) - x) ** 2).sum(1)
            cut(d2, -2.0 * l * l * math.log(sp / s2))
            a = a * s2 * np.exp(-d2 / (2.0 * l * l))
        if P.is_using_intensity:
            c2 = float(np.float32(P.c_ell)) ** 2
            cs2 = float(np.float32(P.c_sigma)) ** 2
            d2c = ((self.ftgt[j].astype(np.float64) - self.fsrc[i].astype(np.float64)) ** 2).sum(1)
            cut(d2c, -2.0 * c2 * math.log(sp / cs2))
            a = a * cs2 * np.exp(-d2c / (2.0 * c2))
        if P.is_using_semantics:
            se2 = float(np.float32(P.s_ell)) ** 2
            ss2 = float(np.float32(P.s_sigma)) ** 2
            d2s = ((self.ltgt[j].astype(np.float64) - self.lsrc[i].astype(np.float64)) ** 2).sum(1)
            cut(d2s, -2.0 * se2 * math.log(sp / ss2))
            a = a * ss2 * np.exp(-d2s / (2.0 * se2))
        with np.errstate(invalid="ignore"):
            hit = ok & (a > sp)
            margin = np.where(ok & ~np.isnan(a), np.minimum(margin, np.abs(a - sp) / sp), margin)
        return dict(a=a, hit=hit, margin=margin)

    def values(self, i):
        """float64 kernel values of row i's hits, in ascending original index."""
        P = self.P
        j = self.members[i]
        if self.kind is not None:
            return self.factors(i, j)["a"]
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
        """(nonzeros, ind [N, K] -1 padded, mat [N, K] float64 0 padded) of the first-K association at identity: the
        first K of every row's hits."""
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


def _unit(rs, n, d):
    u = rs.normal(size=(n, d))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _featured(P, ell, src, tgt, cands, kind, hits, seed):
    """The RowCloud of a rejecting feature kind: row i's cluster cands[i] (ascending original index) gets features that
    make the positions hits[i] of it (an int h: interleaved(c, h); or explicit positions) hits and rejects the others, as
    FEATURE_KINDS describes.  Feature values come from a generator of their own, (seed, kind)."""
    Q = P  # (build() has applied feature_params: the geometry was laid out for the kind's sigma)
    N, M = src.shape[0], tgt.shape[0]
    sp = float(np.float32(Q.sp_thres))

    def thres(ell, sig):  # -2 ell^2 ln(sp / sig^2) of the float parameters, as the kernels compute their cut-offs
        return -2.0 * float(np.float32(ell)) ** 2 * math.log(sp / float(np.float32(sig)) ** 2)

    rf = np.random.default_rng([int(seed), FEATURE_KINDS.index(kind), 77])
    pos = []
    for i, m in enumerate(cands):
        h = len(m) if hits is None or i >= len(hits) else hits[i]
        p = interleaved(len(m), int(h)) if np.ndim(h) == 0 else np.asarray(h, np.int64)
        assert len(p) <= len(m) and (len(p) == 0 or (p.min() >= 0 and p.max() < len(m) and np.all(np.diff(p) > 0))), i
        pos.append(p)
    marked = [np.isin(np.arange(len(m)), p) for m, p in zip(cands, pos)]
    fsrc = ftgt = lsrc = ltgt = gsrc = gtgt = None
    if kind in ("colour", "product"):
        fsrc = rf.uniform(0.3, 0.7, (N, FD))
        ftgt = rf.uniform(0.0, 1.0, (M, FD))
        lo, hi = (1.0, 2.0) if kind == "colour" else (0.10, 0.25)
        thr = thres(Q.c_ell, Q.c_sigma)
        for i, m in enumerate(cands):
            d2 = np.where(marked[i], rf.uniform(0.002, 0.03, len(m)), rf.uniform(lo, hi, len(m)))
            if kind == "colour":
                d2 = np.where(~marked[i] & (rf.random(len(m)) < 0.5), thr * rf.uniform(1.008, 1.02, len(m)), d2)
            ftgt[m] = fsrc[i] + _unit(rf, len(m), FD) * np.sqrt(d2)[:, None]
        fsrc, ftgt = fsrc.astype(np.float32), ftgt.astype(np.float32)
    elif kind in ("hot", "hot_pass", "soft", "hot_soft"):
        cls_s = rf.integers(0, NC, N)
        other_s = (cls_s + rf.integers(1, NC, N)) % NC
        lsrc = np.zeros((N, NC))
        lsrc[np.arange(N), cls_s] = 1.0
        if kind == "soft":
            lsrc[np.arange(N), cls_s] = 0.9
            lsrc[np.arange(N), other_s] = 0.1
        ltgt = np.zeros((M, NC))
        ltgt[np.arange(M), rf.integers(0, NC, M)] = 1.0
        if kind in ("soft", "hot_soft"):  # targets outside every cluster: soft rows too
            ltgt = 0.8 * ltgt + 0.2 * rf.dirichlet(np.ones(NC), M)
        for i, m in enumerate(cands):
            c = len(m)
            e = np.zeros((c, NC))
            if kind in ("hot", "hot_pass"):
                e[np.arange(c), np.where(marked[i], cls_s[i], (cls_s[i] + rf.integers(1, NC, c)) % NC)] = 1.0
                ltgt[m] = e
                continue
            # a third class per member, neither of the source row's two
            third = np.array([k for k in range(NC) if k != cls_s[i] and k != other_s[i]])[rf.integers(0, NC - 2, c)]
            e[np.arange(c), third] = 1.0
            # d2_s = t^2 |p - e_c|^2 = t^2 (|p|^2 + 1)
            scale = float((lsrc[i] ** 2).sum()) + 1.0
            t = np.where(marked[i], rf.uniform(0.08, 0.36, c), rf.uniform(0.88, 0.98, c))
            near = np.sqrt(thres(Q.s_ell, Q.s_sigma) * rf.uniform(1.008, 1.02, c) / scale)
            t = np.where(~marked[i] & (rf.random(c) < 0.5), near, t)
            ltgt[m] = (1.0 - t)[:, None] * lsrc[i] + t[:, None] * e
        lsrc, ltgt = lsrc.astype(np.float32), ltgt.astype(np.float32)
    elif kind == "geotype":
        th = rf.uniform(0.0, np.pi, N)
        gsrc = np.stack([np.cos(th), np.sin(th)], 1) * rf.uniform(0.5, 2.0, (N, 1))
        tt = rf.uniform(0.0, np.pi, M)
        gtgt = np.stack([np.cos(tt), np.sin(tt)], 1) * rf.uniform(0.5, 2.0, (M, 1))
        for i, m in enumerate(cands):
            c = len(m)
            dev = np.where(rf.random(c) < 0.3, 0.0, np.radians(rf.uniform(15.0, 55.0, c)) * rf.choice([-1.0, 1.0], c))
            ang = th[i] + np.where(marked[i], dev, np.pi / 2)
            g = np.stack([np.cos(ang), np.sin(ang)], 1) * rf.uniform(0.5, 2.0, (c, 1))
            rej = np.flatnonzero(~marked[i])
            g[rej] = np.stack([-gsrc[i, 1], gsrc[i, 0]], 0) * rf.uniform(0.5, 2.0, (len(rej), 1))  # exactly orthogonal
            nearly = rej[1::2]  # geo_sim = cos^2 in [0.004, 0.008]
            an = th[i] + np.arccos(np.sqrt(rf.uniform(0.004, 0.008, len(nearly)))) * rf.choice([-1.0, 1.0], len(nearly))
            g[nearly] = np.stack([np.cos(an), np.sin(an)], 1) * rf.uniform(0.5, 2.0, (len(nearly), 1))
            g[rej[::7]] = 0.0
            gtgt[m] = g
        gsrc, gtgt = gsrc.astype(np.float32), gtgt.astype(np.float32)
    else:
        raise KeyError(kind)
    rc = RowCloud(Q, ell, src, tgt, [m[p] for m, p in zip(cands, pos)], fsrc, ftgt, kind, cands, lsrc, ltgt,
                  gsrc, gtgt)
    # the float64 gates of the built arrays decide what a hit is; the construction must have produced what was asked
    for i, m in enumerate(cands):
        hit = rc.factors(i)["hit"]
        assert np.array_equal(hit, np.ones(len(m), bool) if kind == "hot_pass" else marked[i]), (kind, i)
    if kind == "hot_pass":
        rc = RowCloud(Q, ell, src, tgt, cands, fsrc, ftgt, kind, cands, lsrc, ltgt, gsrc, gtgt)
    rc.marked = marked
    return rc


def build(P, counts, ell=None, n_rows=None, n_targets=None, low_rows=(), seed=0, colour=False, feature=None, hits=None):
    """A RowCloud whose row i (in the given order; the source cloud's original order is shuffled with `seed`) owns
    counts[i] targets.

    n_rows: pad with rows that have no hits up to this N.  n_targets: pad with far-away targets up to this M.
    low_rows: rows (indices into `counts`) whose hits take the lowest original target indices, in that order; every other
    target gets a seeded shuffled index.  colour: 5-channel features within a few hundredths of one common colour (the
    colour kernel then keeps every geometric hit: see the module docstring).
    feature: one of FEATURE_KINDS - the cluster of counts[i] targets are row i's geometric CANDIDATES and features make
    hits[i] of them hits (an int: that many, interleaved with the rejected ones in original-index order; an array: those
    positions of the cluster in ascending original index; missing: all).  The kind's parameters (feature_params) apply to
    the layout too: the cluster radii follow its sigma."""
    assert not (colour and feature), "colour=True is the always-passing variant; feature='colour' the rejecting one"
    if feature is not None:
        P = feature_params(P, feature)
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
    if feature is not None:
        hits = None if hits is None else [(list(hits) + [None] * N)[k] for k in sperm]
        hits = None if hits is None else [len(members[q]) if h is None else h for q, h in enumerate(hits)]
        return _featured(P, ell, src, tgt, members, feature, hits, seed)
    fsrc = ftgt = None
    if colour:
        base = np.array([0.5, 0.4, 0.6, 0.45, 0.55], np.float32)
        fsrc = (base + rs.uniform(-0.02, 0.02, (N, FD))).astype(np.float32)
        ftgt = (base + rs.uniform(-0.02, 0.02, (M, FD))).astype(np.float32)
    return RowCloud(P, ell, src, tgt, members, fsrc, ftgt)


def foreign_distance(rc):
    """min over rows i of (distance from x_i to the nearest target NOT in its cluster) / r_i, evaluated in row chunks."""
    own = np.full(rc.M, -1, np.int64)
    for i, m in enumerate(rc.cands):
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


# (candidates, hits) of the families with a rejecting feature kind: the hit counts sit on the limits the candidate counts
# of LIST_VALUES / OVERFLOW_VALUES sit on, the candidate counts on the next limit up (so a row's class, which follows its
# candidates, and its slot / first-K / compaction arithmetic, which follows its hits, meet different limits), plus rows far
# beyond a limit with hits far below it.
LIST_CH = ((2, 0), (3, 1), (12, 5), (13, 6), (16, 7), (17, 8), (20, 9), (32, 15), (33, 16), (40, 17), (64, 31), (64, 32),
           (64, 33), (64, 63), (63, 6), (64, 1))
OVERFLOW_CH = ((65, 6), (70, 6), (65, 64), (127, 64), (128, 65), (129, 127), (255, 128), (256, 129), (257, 255), (300, 40),
               (304, 256), (305, 257), (384, 304), (385, 305), (1023, 384), (1024, 385), (1025, 1023), (1100, 70),
               (1215, 1024), (1216, "quarters"), (1217, 1216), (2000, 1025))


def quarter_hits(c=1216):
    """Hit positions of a row of c = 4 x 304 candidates whose quarters differ: all but one of the first 304 (303 hits), none
    of the second, every other one of the third (152), five of the fourth - 460 hits."""
    q = c // 4
    return np.concatenate([np.delete(np.arange(q), q // 2), 2 * q + np.arange(0, q, 2), 3 * q + interleaved(q, 5)])


def _hits_of(ch):
    return [quarter_hits(c) if isinstance(h, str) else h for c, h in ch]


def list_family(P, seed=1, colour=False, ell=None, feature=None):
    """64 rows on each list class (a whole wave, and with the spatial sort a 256-row window, on one value): 6 entries in
    LDS, sorting networks 8 / 16 / 32 / 64, ASSOC_CAP32 = 32 and ASSOC_CAP16 = 64 (rows of 65 overflow).
    feature: rows of LIST_CH (candidates, hits) instead, all within the list capacity."""
    if feature:
        return build(P, [c for c, _ in LIST_CH for _ in range(64)], ell=ell, seed=seed, feature=feature,
                     hits=[h for h in _hits_of(LIST_CH) for _ in range(64)])
    return build(P, [c for c in LIST_VALUES for _ in range(64)], ell=ell, seed=seed, colour=colour)


def overflow_family(P, seed=2, colour=False, ell=None, feature=None):
    """Two rows on each overflow class: 128-candidate steps of k_assoc_dense, WIDE_MIN = 256, WIDE_CAP = 304 per quarter,
    LONG_CAP = 1024 (rows beyond it are scanned literally), 1216 = 4 x WIDE_CAP, and one row well above; 64 empty rows.
    feature: rows of OVERFLOW_CH (candidates, hits) instead."""
    if feature:
        return build(P, [c for c, _ in OVERFLOW_CH for _ in range(2)], ell=ell, n_rows=2 * len(OVERFLOW_CH) + 64,
                     seed=seed, feature=feature, hits=[h for h in _hits_of(OVERFLOW_CH) for _ in range(2)])
    return build(P, [c for c in OVERFLOW_VALUES for _ in range(2)], ell=ell, n_rows=98, seed=seed, colour=colour)


def wide_family(P, M, low=True, seed=3, feature=None):
    """A lone small pair (N = 16) with M targets, M around LONG_CAP / 4 x WIDE_CAP: one big row (all targets but 24, or
    all of them when that leaves it within LONG_CAP), its hits either on the lowest original indices (a full first
    quarter of the wide phase) or shuffled, plus a row of the rest.
    feature: the big row keeps 3 of 4 of its candidates as hits when M <= 1100, else quarter_hits' pattern stretched to
    its length (a nearly full quarter, an empty one, a half and a handful); the small row half of its candidates."""
    big = M - 24 if M - 24 > 1024 else (1000 if M <= 1024 else M)
    counts = [big, M - big] + [0] * 14
    if feature:
        q = big // 4
        bh = (3 * big) // 4 if M <= 1100 else np.concatenate(
            [np.delete(np.arange(q), q // 2), 2 * q + np.arange(0, q, 2), 3 * q + interleaved(big - 3 * q, 5)])
        return build(P, counts, n_targets=M, low_rows=(0,) if low else (), seed=seed, feature=feature,
                     hits=[bh, (M - big) // 2])
    return build(P, counts, n_targets=M, low_rows=(0,) if low else (), seed=seed)


def dense_family(P, M=1100, seed=4, feature=None):
    """More than half of 16 rows overflow and M <= 2048: the pair enters the dense regime (cvo_update.h: 2 c_ovf > N and
    M <= 2048), where every row is evaluated over all M targets (the wide phase at 1025 <= M <= 1216).  Row 0 has 400
    hits on the lowest original indices.
    feature: row 0 keeps 40 of its 400 candidates, the rows of 70 keep 6, 64 or all 70 of theirs."""
    if feature:
        return build(P, [400] + [70] * 8 + [0] * 7, n_targets=M, low_rows=(0,), seed=seed, feature=feature,
                     hits=[40, 6, 6, 6, 64, 64, 70, 70, 33])
    return build(P, [400] + [70] * 8 + [0] * 7, n_targets=M, low_rows=(0,), seed=seed)


def bits_family(P, M, seed=5, feature=None):
    """Rows of 20 .. 100 candidates (and two beyond LONG_CAP) padded to M targets: M = 65535 keeps 16-bit candidate lists
    (capacity ASSOC_CAP16 = 64, long lists on), M = 65536 switches to 32-bit lists (ASSOC_CAP32 = 32, no long lists).
    feature: every row keeps a third of its candidates, rounded up (7 .. 34 hits; the rows of 1100 keep 70)."""
    counts = [c for c in (20, 32, 33, 48, 64, 65, 100) for _ in range(8)] + [1100, 1100]
    if feature:
        return build(P, counts, n_rows=96, n_targets=M, seed=seed, feature=feature,
                     hits=[70 if c == 1100 else (c + 2) // 3 for c in counts])
    return build(P, counts, n_rows=96, n_targets=M, seed=seed)


def score_family(P, seed=6):
    """Clusters of 3 .. 200 targets (several 64-target tiles each) for the inner-product limits around c_max = 200."""
    return build(P, [c for c in (3, 70, 150, 200) for _ in range(4)], n_rows=40, seed=seed)


def score_rows(P, K, h_max, feature, seed=7):
    """Rows of 3 K candidates for the scores: four with h_max hits (K - 1, K or K + 1: k_overlap's void rule counts hits,
    not candidates), four with K // 2, and rows of 3 / 70 candidates with 2 / 6 hits; 24 empty rows."""
    counts = [3 * K] * 8 + [3] * 4 + [70] * 4
    hits = [h_max] * 4 + [K // 2] * 4 + [2] * 4 + [6] * 4
    return build(P, counts, n_rows=40, seed=seed, feature=feature, hits=hits)
