"""Cases of the sparse kernel's tests (test_bki_sparse_cpu.py, test_gpu_bki_sparse.py, test_cpp_bki_sparse.py): a case is
(Config with sf2 and ell, [(kernel, (xyz, feat, label, origin))]).  The shapes follow bki_cases.py's micro maps: resolution 0.5,
free_resolution 100 so that the origin is the only free point, unless said otherwise."""
import numpy as np

import bki_cases as bc
import np_bki
import np_bki_sparse as sp

F32 = np.float32
CSM, SPARSE = sp.CSM, sp.SPARSE
RES = 0.5
# segment lengths in one block: both sides of BKI_SHORT_RUN (the lane / wave split is by a voxel's records over its seven
# slots), of the wave's 64 records per trip, several trips, and the thousands a voxel next to the sensor collects
RUNS = [1, 2, bc.SHORT_RUN, bc.SHORT_RUN + 1, 63, 64, 65, 256, 257, 3000]
BELOW1, ABOVE1 = np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2))
BELOW15, ABOVE15 = np.nextafter(F32(1.5), F32(0)), np.nextafter(F32(1.5), F32(2))
D_EDGES = [BELOW1, F32(1), ABOVE1, BELOW15, F32(1.5), ABOVE15]


def config(sf2=1.0, ell=1.0, **kw):
    kw.setdefault("resolution", RES)
    kw.setdefault("free_resolution", 100.0)
    return np_bki.Config(sf2=sf2, ell=ell, **kw)


def map_kwargs(cfg):
    """np_bki.Config.kwargs() leaves sf2 and ell out: they changed nothing before this kernel"""
    return dict(cfg.kwargs(), sf2=float(F32(cfg.sf2)), ell=float(F32(cfg.ell)))


def sparse(cfg, frames):
    return cfg, [(SPARSE, f) for f in frames]


def micro(name, **kw):
    kw0, xyz, label, origin = bc.MICRO[name]
    return sparse(config(**dict(kw0, **kw)), [(bc.f32(*xyz), np.ones((len(xyz), 5), F32), None if label is None else bc.f32(*label), bc.f32(*origin))])


def d_edges():
    """hits on the x axis at ell * d from the centre of the voxel at 0, ell = resolution / 2: d below 1 lies in the voxel itself,
    d = 1 on the face it shares with its +x neighbour, the others inside that neighbour.  The origin is far away."""
    ell = F32(0.25)
    xyz = np.array([[ell * d, 0, 0] for d in D_EDGES], F32)
    rng = np.random.default_rng(3)
    feat, _ = bc.rows(rng, len(xyz), 0)
    return sparse(config(sf2=0.75, ell=float(ell)), [(xyz, feat, None, bc.f32(0.0, 0.0, -3.0))])


def run(seed, n, neighbour, C=2):
    """n hits inside ONE block, three more in its +x neighbour or none there, a few far away; no beam samples"""
    rng = np.random.default_rng(seed)
    inside = (bc.f32(2.0, 1.0, -1.0) + rng.uniform(-0.2, 0.2, (n, 3))).astype(F32)
    beside = (bc.f32(2.5, 1.0, -1.0) + rng.uniform(-0.2, 0.2, (3 if neighbour else 0, 3))).astype(F32)
    other = rng.uniform(-5, -3, (4, 3)).astype(F32)
    xyz = np.concatenate([inside, beside, other])
    xyz = xyz[rng.permutation(len(xyz))]
    return sparse(config(sf2=1.25, ell=0.75, num_classes=C), [bc.frame(rng, xyz, C)])


def rays(seed=5):
    """real beam samples (free_resolution 1): 24 rays of 5 - 60 blocks, and 150 short ones whose last sample (l - fr from the
    origin) falls into the blocks around the origin - the cluster of ray starts a sensor leaves there"""
    rng = np.random.default_rng(seed)

    def on_sphere(n, lo, hi):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))

    origin = bc.f32(0.125, 0.25, -0.125)
    xyz = (np.concatenate([on_sphere(24, 2.5, 30.0), on_sphere(150, 1.05, 1.6)]) + origin).astype(F32)
    xyz = xyz[rng.permutation(len(xyz))]
    return sparse(config(sf2=1.0, ell=1.0, num_classes=3, free_resolution=1.0), [bc.frame(rng, xyz, 3, origin=origin)])


def classes(C, with_feat, n=70):
    cfg, frames = bc.scattered(400 + C, n, C=C)
    xyz, feat, label, origin = frames[0]
    return sparse(config(sf2=0.5, ell=1.5, num_classes=C, prior=0.001), [(xyz, feat if with_feat else None, label, origin)])


def three_inserts(kernels=(SPARSE, SPARSE, SPARSE), seed=7, C=19, n=90):
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(3):
        xyz = rng.uniform(-2, 2, (n, 3)).astype(F32)
        xyz[:30] = np.round(xyz[:30])  # (voxel centres shared between the frames)
        frames.append(bc.frame(rng, xyz, C, origin=(0.1 * f, 0.2, 0.3)))
    return config(sf2=1.0, ell=1.0, num_classes=C, prior=0.3), list(zip(kernels, frames))


def growth(seed=9):
    """two frames of scattered hits whose neighbour-only voxels outnumber the touched ones several times"""
    rng = np.random.default_rng(seed)
    return sparse(config(sf2=1.0, ell=0.5, resolution=0.25, num_classes=2),
                  [bc.frame(rng, rng.uniform(-4, 4, (40, 3)).astype(F32), 2), bc.frame(rng, rng.uniform(4, 12, (90, 3)).astype(F32), 2)])


def all_cases():
    out = {"one_hit": micro("centre", sf2=0.7, ell=1.0)}
    for name in ("face", "edge", "corner"):
        out[name] = micro(name, sf2=1.0, ell=1.0)
    out["ell_is_resolution"] = micro("centre", sf2=1.0, ell=RES)
    out["ell_quarter"] = micro("centre", sf2=1.0, ell=RES / 4)
    out["ell_twenty"] = micro("centre", sf2=1.0, ell=20 * RES)
    out["d_edges"] = d_edges()
    for n in RUNS:
        for neighbour in (True, False):
            out[f"run{n}_{'beside' if neighbour else 'alone'}"] = run(500 + n, n, neighbour)
    out["rays"] = rays()
    for C in (0, 2, 19):
        for with_feat in (True, False):
            out[f"classes{C}_{'feat' if with_feat else 'nofeat'}"] = classes(C, with_feat)
    out["three_inserts"] = three_inserts()
    out["csm_sparse_csm"] = three_inserts((CSM, SPARSE, CSM))
    out["growth"] = growth()
    out["gap"] = micro("gap", sf2=1.0, ell=1.0)
    out["hit_is_origin"] = micro("hit_is_origin", sf2=1.0, ell=1.0)
    # no hit, and the origin in the rounding gap between two boxes: an insert without a single membership
    out["no_membership"] = sparse(config(resolution=float(bc.GAP_RESOLUTION)),
                                  [(np.zeros((0, 3), F32), np.zeros((0, 5), F32), None, bc.f32(float(bc.GAP_X), 0.0, 0.0))])
    return out


def statement(case):
    """[(table, cloud, last)] of the statement after every frame of the case"""
    cfg, frames = case
    m = sp.Map(cfg)
    out = []
    for kernel, (xyz, feat, label, origin) in frames:
        m.set_kernel(kernel)
        m.insert(xyz, feat, label, origin)
        out.append((m.table(), m.cloud(), dict(m.last)))
    return out


_STATEMENTS = {}


def statement_of(name):
    """... computed once per test session, shared and left unchanged"""
    if name not in _STATEMENTS:
        _STATEMENTS[name] = statement(all_cases()[name])
    return _STATEMENTS[name]


def run_map(m, case):
    """the case through a SemanticMap (of either side) -> [(stats with the read-back table, cloud, size)] after every frame"""
    out = []
    for kernel, (xyz, feat, label, origin) in case[1]:
        m.set_kernel("sparse" if kernel == SPARSE else "csm")
        m.insert((xyz, feat, label), origin=origin)
        out.append((m.debug_stats(readback=True), m.cloud(), m.size()))
    return out
