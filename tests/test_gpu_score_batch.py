"""Batched scores (cvo_inner_product_batch / cvo_function_angle_batch, CvoGPU.inner_product_batch /
function_angle_batch, the C++ veneer's overloads): every value equals (==) what the single call returns on the same
context - overlap launches, void jobs repeated through the list chain, chain-only calls, deduplicated <X, X> / <Y, Y>,
chunked launches of thousands of jobs.  A single call is a one-job batch (score_batch), so these comparisons show that a
job's value does not depend on its company; the values themselves are pinned by the oracle test here and by the oracle and
list-chain comparisons of test_gpu_parity.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
from unified_cvo_amd import CvoError, CvoGPU, CvoParams, CvoPointCloud, _capi, synth

pytestmark = pytest.mark.gpu


def _pose(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    T[:3, 3] = t
    return T


def _singles(gpu, src, tgt, Ts, ells):
    ip = np.array([gpu.inner_product_gpu(s, t, T, e) for s, t, T, e in zip(src, tgt, Ts, ells)], np.float32)
    fa = np.array([gpu.function_angle(s, t, T, e, True) for s, t, T, e in zip(src, tgt, Ts, ells)], np.float32)
    fe = np.array([gpu.function_angle(s, t, T, e, False) for s, t, T, e in zip(src, tgt, Ts, ells)], np.float32)
    return ip, fa, fe


def _batches(gpu, src, tgt, Ts, ells):
    return (gpu.inner_product_batch(src, tgt, Ts, ells), gpu.function_angle_batch(src, tgt, Ts, ells, True),
            gpu.function_angle_batch(src, tgt, Ts, ells, False))


def _assert_same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g, w), (np.flatnonzero(g != w)[:8], g[g != w][:4], w[g != w][:4])


def _mixed_clouds():
    """Clouds of configs 2 / 3 / 4 at 1k .. 10k points (pairs of each)."""
    out = []
    for builder, n in ((cases.config2, 1000), (cases.config2, 10000), (cases.config3, 2500), (cases.config3, 6000),
                       (cases.config4, 1500), (cases.config4, 4000)):
        _, s, t, _ = builder(n=n)
        out += [s, t]
    return out


def test_mixed_batch_is_bit_identical_to_single_calls():
    clouds = _mixed_clouds()
    rng = np.random.default_rng(11)
    poses = [np.eye(4, dtype=np.float32), synth.gt_motion().astype(np.float32)]
    for params_of in (cases.config2, cases.config3, cases.config4):
        P = params_of(n=64)[0]
        gpu = CvoGPU(params=P)
        dev = [gpu.upload(c) for c in clouds]
        src, tgt, Ts, ells = [], [], [], []
        for k in range(54):
            i = int(rng.integers(0, len(clouds)))
            j = i ^ 1 if k % 6 else i  # the cloud's own partner, or itself (source == target)
            src.append(clouds[i] if k % 2 else dev[i])  # CvoPointCloud (uploaded once per object) and DeviceCloud
            tgt.append(dev[j])
            Ts.append(poses[k % 2])
            ells.append((0.15, 0.3, P.ell_init)[k % 3])
        want = _singles(gpu, src, tgt, Ts, ells)
        got = _batches(gpu, src, tgt, Ts, ells)
        _assert_same(got, want)
        assert np.all(np.isfinite(got[2])) and np.any(got[0] > 0)
        gpu.close()


def test_void_jobs_go_through_the_chain_bit_for_bit():
    P, src, tgt, init = cases.config2(n=2000)
    P.nearest_neighbors_max = 6  # rows at ell 0.5 find more than 6 pairs (void), at 0.05 they do not
    gpu = CvoGPU(params=P)
    da, db = gpu.upload(src), gpu.upload(tgt)
    n = 12
    S, D = [da] * n, [db if k % 3 else da for k in range(n)]
    Ts = [_pose(0.01 * k, (0.01 * k, 0, 0)) for k in range(n)]
    ells = [0.5 if k % 2 else 0.05 for k in range(n)]
    want = _singles(gpu, S, D, Ts, ells)
    got = []
    for fn in (lambda: gpu.inner_product_batch(S, D, Ts, ells), lambda: gpu.function_angle_batch(S, D, Ts, ells, True),
               lambda: gpu.function_angle_batch(S, D, Ts, ells, False)):
        got.append(fn())
        ov, ch, launches = gpu.debug_last_score_batch()
        assert ch > 0 and ov > 0 and launches >= 2, (ov, ch, launches)
    _assert_same(got, want)
    assert np.all(got[0] > 0)


@pytest.mark.parametrize("how", ["no_geometry", "ip_chain"])
def test_chain_only_calls_are_bit_identical(how):
    P, src, tgt, init = cases.config2(n=1500)
    if how == "no_geometry":
        P.is_using_geometry = 0
    gpu = CvoGPU(params=P)
    if how == "ip_chain":
        gpu.set_option("IP_CHAIN", "1")
    da, db = gpu.upload(src), gpu.upload(tgt)
    n = 9
    S, D = [da, db, da] * 3, [db, da, da] * 3
    Ts = [_pose(0.02 * k, (0, 0.01 * k, 0)) for k in range(n)]
    ells = [0.3 if k < 5 else 0.2 for k in range(n)]
    want = _singles(gpu, S, D, Ts, ells)
    got = _batches(gpu, S, D, Ts, ells)
    ov, ch, _ = gpu.debug_last_score_batch()
    assert ov == 0 and ch == n + 2 * 2  # exact: every <X, Y> and <X, X>, <Y, Y> once per lengthscale
    _assert_same(got, want)


def test_pose_sweep_deduplicates_self_products():
    P, src, tgt, init = cases.config2(n=10000)
    gpu = CvoGPU(params=P)
    da, db = gpu.upload(src), gpu.upload(tgt)
    Ts = [_pose(0.004 * (k - 16), (0.01 * (k - 16), 0.005 * k, 0)) for k in range(32)]
    got = gpu.function_angle_batch([da] * 32, [db] * 32, Ts, 0.3, is_approximate=False)
    assert gpu.debug_last_score_batch() == (32 + 2, 0, 1)
    want = np.array([gpu.function_angle(da, db, T, 0.3, False) for T in Ts], np.float32)
    assert np.array_equal(got, want)
    assert len(set(got.tolist())) > 1


def test_single_calls_run_as_one_job_batches():
    P, src, tgt, init = cases.config2(n=2000)
    K = P.nearest_neighbors_max  # 512: no row finds that many pairs at ell 0.3; at 0.5 some find more than 6
    gpu = CvoGPU(params=P)
    da, db = gpu.upload(src), gpu.upload(tgt)
    gpu.inner_product_gpu(da, db, init, 0.3)
    assert gpu.debug_last_score_batch() == (1, 0, 1)
    gpu.function_angle(da, db, init, 0.3, True)
    assert gpu.debug_last_score_batch() == (1, 0, 1)
    gpu.function_angle(da, db, init, 0.3, False)
    assert gpu.debug_last_score_batch() == (3, 0, 1)
    gpu.function_angle(da, da, init, 0.3, False)  # <X, X> once
    assert gpu.debug_last_score_batch() == (2, 0, 1)
    P.nearest_neighbors_max = 6  # void: the chain repeats the call's evaluations
    gpu.params = P
    gpu.inner_product_gpu(da, db, init, 0.5)
    assert gpu.debug_last_score_batch() == (1, 1, 2)
    gpu.function_angle(da, db, init, 0.5, False)
    assert gpu.debug_last_score_batch() == (3, 3, 2)
    P.nearest_neighbors_max = K
    gpu.params = P
    gpu.set_option("IP_CHAIN", "1")
    gpu.inner_product_gpu(da, db, init, 0.3)
    assert gpu.debug_last_score_batch() == (0, 1, 1)
    gpu.function_angle(da, db, init, 0.3, False)
    assert gpu.debug_last_score_batch() == (0, 3, 1)


def test_batch_against_the_oracle(oracle):
    P, src, tgt, init = cases.config4(n=1500)
    gpu = CvoGPU(params=P)
    op = oracle.params_from(P)
    ox, oy = oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt)
    Ts = [init, synth.gt_motion().astype(np.float32), init]
    ells = [P.ell_init, 0.25, 0.4]
    ip = gpu.inner_product_batch([src] * 3, [tgt] * 3, Ts, ells)
    for approx in (True, False):
        fa = gpu.function_angle_batch([src] * 3, [tgt] * 3, Ts, ells, approx)
        for k in range(3):
            assert fa[k] == pytest.approx(oracle.function_angle(op, ox, oy, Ts[k], ells[k], approx), rel=1e-4, abs=1e-12)
    for k in range(3):
        assert ip[k] == pytest.approx(oracle.inner_product(op, ox, oy, Ts[k], ells[k]), rel=1e-4, abs=1e-12)


def test_thousands_of_jobs_across_chunks():
    P = cases.config2(n=64)[0]
    gpu = CvoGPU(params=P)
    rng = np.random.default_rng(3)
    clouds = []
    for c in range(16):
        src, tgt, _ = synth.geometric_pair(96 + 24 * c, c)
        clouds += [gpu.upload(CvoPointCloud.from_xyz(src)), gpu.upload(CvoPointCloud.from_xyz(tgt))]
    n = 4096
    I = rng.integers(0, len(clouds), n)
    S = [clouds[i] for i in I]
    D = [clouds[i ^ 1] for i in I]
    Ts = [_pose(0.001 * (k % 50), (0.002 * (k % 7), 0, 0)) for k in range(n)]
    ells = np.where(np.arange(n) % 2 == 0, 0.3, 0.45).astype(np.float32)
    a = gpu.function_angle_batch(S, D, Ts, ells, False)
    ov, ch, launches = gpu.debug_last_score_batch()
    assert launches >= 2 and ch == 0 and ov == n + 2 * len(clouds)  # (one chunk boundary at least; no voids)
    b = gpu.function_angle_batch(S, D, Ts, ells, False)  # gate words reset: the same output again
    assert np.array_equal(a, b)
    ip = gpu.inner_product_batch(S, D, Ts, ells)
    for k in range(0, n, 97):  # single calls between batch calls
        assert gpu.inner_product_gpu(S[k], D[k], Ts[k], float(ells[k])) == ip[k]
        assert gpu.function_angle(S[k], D[k], Ts[k], float(ells[k]), False) == a[k]
    assert np.array_equal(gpu.inner_product_batch(S, D, Ts, ells), ip)
    want = np.array([gpu.inner_product_gpu(s, d, T, float(e)) for s, d, T, e in zip(S, D, Ts, ells)], np.float32)
    assert np.array_equal(ip, want) and np.all(ip > 0)


def test_empty_clouds_and_kdtree():
    P, src, tgt, init = cases.config2(n=800)
    gpu = CvoGPU(params=P)
    empty = CvoPointCloud.from_xyz(np.zeros((0, 3), np.float32))
    S, D = [src, empty, src, src], [tgt, tgt, empty, tgt]
    Ts = [init] * 4
    for got in _batches(gpu, S, D, Ts, 0.3):
        assert got[1] == 0.0 and got[2] == 0.0 and got[0] > 0 and got[3] == got[0]
    assert gpu.inner_product_batch([], [], [], 0.3).shape == (0,)
    # kd-tree parameters: CVO_E_UNSUPPORTED, nothing written
    P.is_using_kdtree = 1
    gpu.params = P
    da, db = gpu.upload(src), gpu.upload(tgt)
    L = gpu.L
    p = P.to_ctypes()
    h = (C.c_void_p * 2)(da.handle, da.handle)
    g = (C.c_void_p * 2)(db.handle, db.handle)
    T = np.tile(np.eye(4, dtype=np.float32).reshape(16), 2)
    ell = np.full(2, 0.3, np.float32)
    out = np.full(2, 42.0, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert L.cvo_inner_product_batch(gpu.ctx, C.byref(p), 2, h, g, fp(T), fp(ell), fp(out)) == _capi.CVO_E_UNSUPPORTED
    assert L.cvo_function_angle_batch(gpu.ctx, C.byref(p), 2, h, g, fp(T), fp(ell), 0, fp(out)) == _capi.CVO_E_UNSUPPORTED
    assert np.all(out == 42.0)
    assert L.cvo_inner_product_batch(gpu.ctx, C.byref(p), -1, h, g, fp(T), fp(ell), fp(out)) == _capi.CVO_E_INVALID
    with pytest.raises(CvoError):
        gpu.inner_product_batch([da], [db], [np.eye(4)], 0.3)
    P.is_using_kdtree = 0
    assert L.cvo_inner_product_batch(gpu.ctx, C.byref(P.to_ctypes()), 0, None, None, None, None, None) == _capi.CVO_OK
    with pytest.raises(CvoError):
        gpu.inner_product_batch([da], [db], [np.eye(4)], -1.0)


def test_cpp_driver_prints_the_python_batch_values(tmp_path):
    from test_cpp_host import _write_pcd
    drv = os.path.join(cases.ROOT, "host", "cvo_score_batch")
    sx, sr, tx, tr = cases.demo_clouds()
    _write_pcd(tmp_path / "source.pcd", sx, sr)
    _write_pcd(tmp_path / "target.pcd", tx, tr)
    yaml = os.path.join(cases.CONFIGS, "outdoor.yaml")
    ell = 2.5
    out = subprocess.check_output([drv, str(tmp_path / "source.pcd"), str(tmp_path / "target.pcd"), yaml, str(ell), "6"],
                                  text=True)
    poses, scores = [], []
    for line in out.strip().splitlines():
        w = line.split()
        if w[0] == "pose":
            poses.append(np.array([float(v) for v in w[2:]], np.float32).reshape(4, 4).T)
        elif w[0] == "score":
            scores.append([float(v) for v in w[2:]])
    assert len(poses) == len(scores) == 6
    import warnings
    from unified_cvo_amd import read_cvo_params_yaml
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = read_cvo_params_yaml(yaml)
    gpu = CvoGPU(params=P)
    src, tgt = CvoPointCloud.from_xyzrgb(sx, sr), CvoPointCloud.from_xyzrgb(tx, tr)
    got = _batches(gpu, [src] * 6, [tgt] * 6, poses, ell)
    cpp = np.array(scores, np.float32).T
    for g, c in zip(got, cpp):
        assert np.array_equal(g, c), (g, c)
    assert np.any(cpp[0] > 0)
