"""numpy statement of the voxel selection (cvo_voxel_select) and the clouds its tests share."""
import numpy as np

from unified_cvo_amd import synth


def voxel_keys(xyz, s):
    """k = rint(x / s) per axis: float32 quotient, correctly rounded, ties to even (VoxelMap_impl.hpp:170)."""
    return np.rint(np.asarray(xyz, np.float32).reshape(-1, 3) / np.float32(s)).astype(np.int64)


def reference(xyz, s):
    """Indices of the kept points, ascending: of every occupied voxel the point with the lowest index."""
    k = voxel_keys(xyz, s)
    if k.shape[0] == 0:
        return np.zeros(0, np.int32)
    _, first = np.unique(k, axis=0, return_index=True)  # (return_index: the first occurrence)
    return np.sort(first).astype(np.int32)


def reference_packed(xyz, s):
    """reference() for frames of millions of points: ONE np.unique over the packed key kx | ky << 21 | kz << 42 of the
    voxel indices moved to 0 .. 2^21 - 1 (needs |k| < 2^20, what the selection accepts) instead of a row-wise one.
    test_voxel_cpu.py holds the two equal."""
    k = voxel_keys(xyz, s)
    if k.shape[0] == 0:
        return np.zeros(0, np.int32)
    assert np.abs(k).max() < 2 ** 20
    k += 2 ** 20
    _, first = np.unique(k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42), return_index=True)
    return np.sort(first).astype(np.int32)


def scan_order(xyz):
    """The same points in the order a camera delivers them: sorted by image row, then column, of their pinhole
    projection (640 columns over the scene's field of view).  Neighbours in the order share voxels."""
    p = np.asarray(xyz, np.float64)
    z = np.maximum(p[:, 2], 1e-3)
    col = np.floor((p[:, 0] / z) * 320.0 / 1.8).astype(np.int64)
    row = np.floor((-p[:, 1] / z) * 320.0 / 1.8).astype(np.int64)
    return np.ascontiguousarray(np.asarray(xyz, np.float32)[np.lexsort((col, row))])


def scene(n):
    return synth.scene_pair(n)[0]


LEAVES = (0.05, 0.1, 0.25, 0.5, 1.0)


def half_boundary_cloud(s=0.25):
    """Every coordinate an odd multiple of s / 2 (s a power of two: exact), both signs - ties only.  rint must send
    0.375 / 0.25 = 1.5 and 0.625 / 0.25 = 2.5 both to 2; a multiply by 1 / s would be exact here too, the next cloud is not."""
    m = np.arange(-41, 43, 2, dtype=np.float32) * np.float32(s / 2)
    g = np.stack(np.meshgrid(m, m[:7], m[::5], indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([g, g[::-1]]), np.float32)


def division_cloud(s=0.1, n=20000, seed=5):
    """Coordinates whose quotient by s and whose product with float32(1 / s) round to different voxels: every voxel
    centre +- half a voxel computed in float64 and rounded, kept only where the two recipes disagree (plus the rest
    of the draw, so that the cloud is not made of those alone)."""
    rs = np.random.default_rng(seed)
    k = rs.integers(-700, 700, (n, 3)).astype(np.float64)
    x = ((k + 0.5) * np.float64(np.float32(s))).astype(np.float32)
    for d in (-1, 1):  # the neighbouring floats: the tie itself is rarely representable
        x = np.concatenate([x, np.nextafter(x, np.float32(d * np.inf))])
    a = np.rint(x / np.float32(s))
    b = np.rint(x * (np.float32(1.0) / np.float32(s)))
    differ = np.any(a != b, axis=1)
    assert differ.sum() > 100, differ.sum()
    return np.ascontiguousarray(np.concatenate([x[differ], x[~differ][:5000]]), np.float32)


def duplicates_cloud(n=30000, seed=11):
    """A scene with exact copies of earlier points scattered through it."""
    rs = np.random.default_rng(seed)
    x = scene(n).copy()
    dst = rs.choice(np.arange(n // 10, n), n // 3, replace=False)
    x[dst] = x[rs.integers(0, n // 10, dst.shape[0])]
    return x


def own_voxel_cloud(n=50000, s=0.5):
    """Every point alone in its voxel: distinct lattice sites, jittered by less than a quarter voxel."""
    rs = np.random.default_rng(13)
    site = rs.permutation(80 * 80 * 40)[:n]
    k = np.stack([site % 80 - 40, (site // 80) % 80 - 40, site // 6400 - 20], axis=1).astype(np.float64)
    return ((k + rs.uniform(-0.2, 0.2, k.shape)) * s).astype(np.float32)


def cpu_cases():
    """(name, xyz, leaf size) of every cloud the CPU twin and the device are held to."""
    out = []
    for n in (10000, 307200):
        x = scene(n)
        for s in LEAVES:
            out.append((f"scene{n}-{s}", x, s))
    out.append(("slab", synth.geometric_pair(10000)[0], 0.5))
    out.append(("half-boundary", half_boundary_cloud(0.25), 0.25))
    out.append(("division", division_cloud(0.1), 0.1))
    out.append(("copies", np.tile(np.array([[0.3, -1.2, 7.7]], np.float32), (100000, 1)), 0.1))
    out.append(("own-voxel", own_voxel_cloud(), 0.5))
    for n in (0, 1, 7):
        out.append((f"n{n}", scene(100)[:n], 0.25))
    out.append(("duplicates", duplicates_cloud(), 0.1))
    return out
