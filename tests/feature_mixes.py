"""Clouds and parameters for the 16 settings of (geometry, intensity, semantics, geometric_type) with cut-offs moved so
that every gate of the pair arithmetic rejects a real share of the pairs that reach it (test_oracle_numpy.py on the CPU,
test_gpu_feature_gates.py on the GPU).

The shipped configurations never let the semantic gate reject (semantic_img_gpu0.yaml: s_ell = 1, sp_thres = 0.006 give
d2_s_thres = 10.2, two class distributions are at most 2 apart) and use one geometric type.  MOVED sets sigma, sp_thres,
c_ell and s_ell so that, on the config-4 synthetic clouds below, each of the five gates (geometric type, distance, colour,
semantics, a > sp_thres on the product) rejects between a tenth and nine tenths of what reaches it; the tests assert those
shares with np_reference.gate_shares, so a later change cannot quietly return to a gate that never fires.
"""
import itertools

import numpy as np

import cases
from unified_cvo_amd import CvoPointCloud, synth

MIXES = list(itertools.product((1, 0), repeat=4))  # (geometry, intensity, semantics, geometric_type)
MIX_IDS = ["g%di%ds%dt%d" % m for m in MIXES]
# sp_thres = 0.006 as shipped; on the 300-point config-4 clouds at ell = 0.9 / 1.2 (MOVED_STATES):
#   sigma = 2: the geometric cut-off radius is l sqrt(-2 ln(sp / sigma^2)) = 3.6 l (rejects 0.69 / 0.44 of all pairs), and
#   the geometric kernel of a close pair is above 1 - so a colour or semantic kernel at or below sp_thres does NOT imply a
#   product at or below it, and a kernel that skipped that gate would keep pairs the reference rejects;
#   c_ell = 0.12, c_sigma = 0.8: d2_c_thres = -2 c_ell^2 ln(sp / c_sigma^2) = 0.134 on colours spread over [0, 1]^3 x [0, 0.3]^2;
#   s_ell = 0.46, s_sigma = 0.5: d2_s_thres = -2 s_ell^2 ln(sp / s_sigma^2) = 1.58 - below 2, so another one-hot class is
#   rejected (FEAT_HOT's diff_ok is false) while sk_diff = 2.2e-3 times a geometric kernel above 2.7 would pass the
#   product; soft rows of different classes lie on both sides of it.
# A mix with a single factor has no product gate to speak of: its cut-off IS a > sp_thres, so the product rejects nothing.
MOVED = dict(sigma=2.0, sp_thres=0.006, c_ell=0.12, c_sigma=0.8, s_ell=0.46, s_sigma=0.5)
SHIPPED_STATES = ((0.5, 512), (0.8, 7))   # (ell, K)
# (ell = 0.9, not 0.8: at 0.8 one mix has its coefficient D pass through zero - |D| = 0.97 where it is ~1e3 elsewhere - and a
# relative comparison of a float sum with a double one says nothing there)
MOVED_STATES = ((0.9, 512), (1.2, 7))
LABEL_KINDS = ("soft", "hot", "hot_soft", "absent")
TYPES = np.array([[1.0, 0.0], [0.0, 1.0], [0.3, 0.9], [0.8, -0.5]], np.float32)


def params(mix, moved=True, K=None):
    """semantic_img_gpu0.yaml with the four switches of `mix` and, if asked, the MOVED cut-offs."""
    P = cases.load_params("semantic_img_gpu0")
    P.is_using_geometry, P.is_using_intensity, P.is_using_semantics, P.is_using_geometric_type = mix
    if moved:
        for k, v in MOVED.items():
            setattr(P, k, v)
    if K is not None:
        P.nearest_neighbors_max = K
    return P


def soften(onehot, rs):
    """Class distributions 0.8 .. 0.98 on the row's class, the rest spread over the others (rows sum to 1)."""
    w = rs.uniform(0.8, 0.98, (onehot.shape[0], 1))
    rest = rs.dirichlet(np.ones(onehot.shape[1]) * 0.3, onehot.shape[0]) * (1.0 - onehot)
    rest /= np.maximum(rest.sum(1, keepdims=True), 1e-30)
    return (w * onehot + (1.0 - w) * rest).astype(np.float32)


def arrays(n, labels="soft", seed=0, builder="slab"):
    """dict of float32 arrays (x, y, fx, fy, lx, ly, gx, gy) and the warm-start pose: config-4 positions, colours and
    checkerboard classes ('slab') or the clustered street scene with classes from the same checkerboard ('scene'); labels
    soft on both sides, one-hot on both, one-hot source against soft target, or 'absent' (as 'hot' for the reference: the
    caller uploads no label / colour / type arrays and the reference sees the zeros the device then creates); geometric
    types drawn from TYPES."""
    rs = np.random.default_rng([seed, 4242])
    if builder == "slab":
        x, fx, lx, y, fy, ly = synth.semantic_pair(n, seed)
        init = (synth.gt_motion() @ synth.warm_start_delta()).astype(np.float32)
    else:
        x, fx, y, fy = synth.scene_colour_pair(n, seed)
        lx, ly = synth.checkerboard_labels(x), synth.checkerboard_labels(y)
        init = np.eye(4, dtype=np.float32)
    # five classes instead of 19: about a fifth of all pairs share a class (a one-hot gate that rejects 18 of 19 pairs of a
    # mix without geometry would leave the later gates almost nothing)
    lx, ly = (np.eye(lx.shape[1], dtype=np.float32)[np.argmax(l, 1) % 5] for l in (lx, ly))
    if labels == "soft":
        lx, ly = soften(lx, rs), soften(ly, rs)
    elif labels == "hot_soft":
        ly = soften(ly, rs)
    gx = TYPES[rs.integers(0, len(TYPES), x.shape[0])]
    gy = TYPES[rs.integers(0, len(TYPES), y.shape[0])]
    d = dict(x=x, y=y, fx=fx, fy=fy, lx=lx, ly=ly, gx=gx, gy=gy)
    if labels == "absent":
        d.update(fx=np.zeros_like(fx), fy=np.zeros_like(fy), lx=np.zeros_like(lx), ly=np.zeros_like(ly),
                 gx=np.zeros_like(gx), gy=np.zeros_like(gy))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in d.items()}, init


def clouds(d):
    return (CvoPointCloud.from_arrays(d["x"], d["fx"], d["lx"], d["gx"]),
            CvoPointCloud.from_arrays(d["y"], d["fy"], d["ly"], d["gy"]))
