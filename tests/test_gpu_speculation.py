"""The production path of align() over whole runs, bit for bit against the traced path.

An untraced call does two things a traced one does not:
  * it speculates: an extra block per pair of k_coeff runs the update's scalar tail on the predicted (clamped) step
    (update_speculate), and the update adopts that state when the real step equals the prediction;
  * geometry-only calls take the association's fast path (geo_fast_path): no column of any ELL entry is kept.
Every oracle comparison of the suite is traced, so it covers neither.  Here one input runs four ways -

    variant        speculation  association path
    traced         off          general (columns kept)      trace_capacity = 1
    default        on           fast
    keep_columns   on           general                     CVO_KEEP_COLUMNS
    no_speculate   off          fast                        CVO_NO_SPECULATE

- and the four must end on the same transform bytes, iteration count, return code, final ell and K.  Where steps sit on
a clamp (speculation follows clamped steps only) the speculative update must really have been adopted
(cvo_debug_speculation); it never is in the traced and NO_SPECULATE runs.  On a mismatch the first iteration count at
which the traced and the differing run part is bisected (every prefix run starts from the initial pose and is
deterministic) and reported."""
import os
import time

import numpy as np
import pytest

import cases
import fuzz_draws
from unified_cvo_amd import CvoGPU, CvoPointCloud, synth

pytestmark = pytest.mark.gpu

VARIANTS = ("traced", "default", "keep_columns", "no_speculate")
OPTION = {"keep_columns": "KEEP_COLUMNS", "no_speculate": "NO_SPECULATE"}
FUZZ_SEEDS = int(os.environ.get("CVO_FUZZ_SEEDS", "48"))
FUZZ_CLUSTERED = int(os.environ.get("CVO_FUZZ_CLUSTERED", "12"))
# adopted / iterations of the default run, measured on an MI355X: config 2 at 5k 0.942, config 3 at 10k 0.977 (the clustered
# scene 0.969, with colour 0.990, config 1 0.139).  The floors sit well below: adoption depends on timing (a speculative
# run that is late is not waited for), the results never do.
ADOPTION_FLOOR = {"config2_n5000": 0.6, "config3_n10000": 0.6}


def _key(r):
    return (np.ascontiguousarray(r.transform, np.float32).tobytes(), r.iterations, r.ret, r.final_ell,
            r.final_num_neighbors)


def _run(gpu, src, tgt, init, variant, max_iterations=0):
    """One align of `variant`; returns (result, adopted iterations)."""
    opt = OPTION.get(variant)
    if opt:
        gpu.set_option(opt, "1")
    try:
        kw = dict(trace_capacity=1) if variant == "traced" else {}
        r = gpu.align(src, tgt, init, max_iterations=max_iterations, **kw)
        adopted, its = gpu.debug_speculation()
        assert its == r.iterations
    finally:
        if opt:
            gpu.set_option(opt, None)
    return r, adopted


def _first_divergence(gpu, src, tgt, init, variant, hi):
    """Smallest max_iterations at which `variant` and the traced run differ (they differ at `hi`)."""
    lo = 0   # (equal: nothing has run)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        a, _ = _run(gpu, src, tgt, init, "traced", mid)
        b, _ = _run(gpu, src, tgt, init, variant, mid)
        if _key(a) == _key(b):
            lo = mid
        else:
            hi = mid
    return hi


def check_variants(gpu, P, a, b, init, label, max_iterations=0):
    """The four variants of one input; returns {variant: (result, adopted)} after the assertions above."""
    gpu.write_params(P)
    src, tgt = gpu.upload(a), gpu.upload(b)
    out = {v: _run(gpu, src, tgt, init, v, max_iterations) for v in VARIANTS}
    ref = _key(out["traced"][0])
    bad = [v for v in VARIANTS if _key(out[v][0]) != ref]
    if bad:
        v = "default" if "default" in bad else bad[0]   # (one bisection: it is a diagnosis, not a check)
        hi = max(out[v][0].iterations, out["traced"][0].iterations)
        hi = min(hi, max_iterations) if max_iterations else hi
        first = _first_divergence(gpu, src, tgt, init, v, hi)
        its = {v: out[v][0].iterations for v in VARIANTS}
        pytest.fail(f"{label}: {bad} differ from the traced run (iterations {its}); the traced and {v} runs first differ "
                    f"at max_iterations = {first}")
    assert out["traced"][1] == 0 and out["no_speculate"][1] == 0, label
    return out


def _fraction(out):
    r, adopted = out["default"]
    return adopted / max(r.iterations, 1)


# ---- a. whole runs of the named shapes ----------------------------------------------------------------------------

SHAPES = {
    "config2_n5000": (lambda: cases.config2(n=5000), 0),           # 2000 iterations, clamped at min_step
    "config3_n10000": (lambda: cases.config3(n=10000), 0),         # 5000 iterations, clamped at min_step
    "config4_n10000": (lambda: cases.config4(n=10000), 0),         # ends on dist < eps_2, never clamped: nothing to adopt
    "config1_demo": (lambda: cases.config1(), 1000),               # clamped at max_step
    "scene_n10000": (lambda: cases.scene(n=10000), 0),             # dense and overflow rows
    "scene_colour_n4000": (lambda: cases.scene_colour(n=4000), 0),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shape_whole_run_equals_traced(name):
    build, n_it = SHAPES[name]
    P, src, tgt, init = build()
    gpu = CvoGPU(params=P)
    out = check_variants(gpu, P, src, tgt, init, name, n_it)
    r = out["default"][0]
    print(f"{name}: {r.iterations} iterations, adopted {out['default'][1]} (default) / {out['keep_columns'][1]} "
          f"(keep_columns), fraction {_fraction(out):.3f}")
    if name != "config4_n10000":   # (speculation follows clamped steps only; config 4 steps between 1e-7 and 0.01)
        assert out["default"][1] > 0 and out["keep_columns"][1] > 0, name
    if name in ADOPTION_FLOOR:
        assert _fraction(out) >= ADOPTION_FLOOR[name], (name, _fraction(out))
    if name == "config2_n5000":
        assert r.iterations == P.MAX_ITER == 2000 and r.ret == 0
    if name == "config3_n10000":
        assert r.iterations == P.MAX_ITER == 5000 and r.ret == 0
    if name == "config4_n10000":
        assert r.ret == 0 and r.iterations < P.MAX_ITER
    if name == "scene_n10000":
        assert gpu.debug_row_classes(0)[0] > 0 or gpu.debug_row_classes(0)[2]


# ---- b. the fuzz matrix, run whole -------------------------------------------------------------------------------

FUZZ_ADOPTION = {}   # ("trajectory" | "clustered", seed) -> per-draw record (filled by _fuzz_whole)


def _fuzz_whole(family, seed):
    key = (family, seed)
    if key in FUZZ_ADOPTION:
        return FUZZ_ADOPTION[key]
    P, a, b, init = (fuzz_draws.trajectory if family == "trajectory" else fuzz_draws.clustered)(seed)
    gpu = CvoGPU(params=P)
    out = check_variants(gpu, P, a, b, init, f"{family} seed {seed}")
    n_ovf, _, dense = gpu.debug_row_classes(0)     # (of the last run, keep_columns / no_speculate: the same lists)
    kind = ("geometry", "colour", "semantics")[seed % 3]
    rec = dict(kind=kind, overflow=n_ovf > 0 or dense, range_ell=bool(P.is_using_range_ell),
               adopted=out["default"][1] + out["keep_columns"][1], iterations=out["default"][0].iterations)
    FUZZ_ADOPTION[key] = rec
    gpu.close()
    return rec


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_draw_whole_run_equals_traced(seed):
    _fuzz_whole("trajectory", seed)


@pytest.mark.parametrize("seed", range(FUZZ_CLUSTERED))
def test_clustered_fuzz_draw_whole_run_equals_traced(seed):
    _fuzz_whole("clustered", seed)


def test_fuzz_matrix_adopts_in_every_class():
    """Speculation was adopted, summed over the fuzz draws, for every feature kind, for the draws with overflow rows or
    in the dense regime, and for is_using_range_ell.  Self-contained: runs draws not yet run in this session."""
    recs = [_fuzz_whole("trajectory", s) for s in range(FUZZ_SEEDS)] + \
           [_fuzz_whole("clustered", s) for s in range(FUZZ_CLUSTERED)]
    groups = {k: [r for r in recs if r["kind"] == k] for k in ("geometry", "colour", "semantics")}
    groups["overflow_or_dense"] = [r for r in recs if r["overflow"]]
    groups["range_ell"] = [r for r in recs if r["range_ell"]]
    for g, rs in groups.items():
        ad, it = sum(r["adopted"] for r in rs), sum(r["iterations"] for r in rs)
        print(f"fuzz {g}: {len(rs)} draws, adopted {ad} of 2 x {it} iterations")
        assert rs and ad > 0, g


# ---- c. the oracle link ------------------------------------------------------------------------------------------

def test_default_prefix_equals_traced_on_oracle_strict_draws(oracle):
    """The fuzz draws whose traced 90-iteration prefix followed the oracle strictly (test_gpu_parity.FUZZ_OUTCOMES, worked
    out here for draws not yet run in this session): their untraced 90-iteration prefix ends on the same bytes as that
    traced run, so the production path is held to the oracle iteration by iteration through it."""
    import test_gpu_parity as parity
    strict = [s for s in range(FUZZ_SEEDS) if parity._fuzz_one(oracle, s)]
    n_it = 90
    for seed in strict:
        P, a, b, init = fuzz_draws.trajectory(seed)
        gpu = CvoGPU(params=P)
        src, tgt = gpu.upload(a), gpu.upload(b)
        t = gpu.align(src, tgt, init, max_iterations=n_it, trace_capacity=n_it, trace_dense=n_it)
        d = gpu.align(src, tgt, init, max_iterations=n_it)
        assert _key(d) == _key(t), seed
        gpu.close()
    print(f"oracle link: {len(strict)} of {FUZZ_SEEDS} draws strict")
    assert len(strict) >= 0.9 * FUZZ_SEEDS


# ---- d. batches and the queue against traced solo runs -----------------------------------------------------------

def _solo_traced(gpu, s, t, init, n_it=0):
    return gpu.align(s, t, init, max_iterations=n_it, trace_capacity=1)


def _mixed_pairs(kind, k, seed, min_step=None):
    """k ragged pairs of one feature kind (a batch shares one parameter set): slab and clustered clouds for geometry and
    colour, the semantic slab for semantics."""
    rs = np.random.default_rng(seed)
    out = []
    for p in range(k):
        n = int(rs.integers(1200, 3200))
        if kind == "geometry":
            P, a, b, init = (cases.config2 if p % 2 else cases.scene)(n=n, pair_id=p)
        elif kind == "colour":
            P, a, b, init = (cases.config3 if p % 2 else cases.scene_colour)(n=n, pair_id=p)
        else:
            P, a, b, init = cases.config4(n=n, pair_id=p)
        if p % 3 == 1:   # ragged: fewer source rows than targets
            xs, fs, ls, gs = a.device_arrays()
            cut = int(n * 0.7)
            a = CvoPointCloud.from_arrays(xs[:cut], None if fs is None else fs[:cut], None if ls is None else ls[:cut], gs[:cut])
        if min_step is not None:
            P.min_step = min_step
        out.append((P, a, b, init))
    return out


@pytest.mark.parametrize("kind,n_it,min_step", [("geometry", 0, None), ("colour", 600, None), ("semantics", 0, None),
                                                ("semantics", 800, 2e-3)])
def test_untraced_batch_equals_traced_solo(kind, n_it, min_step):
    """Untraced align_batch of ragged pairs (slab and clustered): every pair bit-identical to the same pair solved alone
    with a trace (no speculation, general association path).  Geometry and semantics run to their own stops; config 4's
    own steps never sit on a clamp, so a second semantic batch raises min_step to 2e-3 (as the fuzz draws do) to be
    speculated on."""
    pairs = _mixed_pairs(kind, 12, {"geometry": 31, "colour": 32, "semantics": 33}[kind], min_step)
    P = pairs[0][0]
    gpu = CvoGPU(params=P)
    res = gpu.align_batch([p[1] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs], max_iterations=n_it)
    adopted = sum(gpu.debug_speculation(q)[0] for q in range(len(pairs)))
    solo = CvoGPU(params=P)
    for q, ((_, s, t, init), r) in enumerate(zip(pairs, res)):
        assert _key(r) == _key(_solo_traced(solo, s, t, init, n_it)), (kind, q)
    print(f"batch {kind} (min_step {P.min_step}): adopted {adopted} of {sum(r.iterations for r in res)} iterations")
    assert adopted > 0 or (kind == "semantics" and min_step is None)


SOAK_TRIALS = 5


@pytest.mark.parametrize("trial", range(SOAK_TRIALS))
def test_full_chip_batch_soak_equals_traced_solo(trial):
    """scripts/soak_batch.py shortened and with fixed seeds, on full-chip batches (48-64 pairs of slab and clustered
    clouds: speculative blocks start late and abandon their runs): every pair bit-identical to a traced solo run."""
    rs = np.random.default_rng(6100 + trial)
    P = cases.load_params("geometric_gpu")
    P.ell_init = float(rs.choice([0.3, 0.6, 0.95, 1.4]))
    P.nearest_neighbors_max = int(rs.choice([40, 200, 512]))
    P.ell_decay_start = int(rs.choice([5, 30]))
    n_pairs = int(rs.integers(48, 65))
    pairs = []
    for q in range(n_pairs):
        n, m = int(rs.integers(300, 3500)), int(rs.integers(300, 3500))
        if rs.integers(0, 2):
            s, t, _ = synth.scene_pair(n, 100 * trial + q, m=m)
        else:
            s, t, _ = synth.geometric_pair(n, 100 * trial + q, m=m)
        init = (synth.gt_motion() @ synth.warm_start_delta()).astype(np.float32) if rs.integers(0, 2) else np.eye(4, dtype=np.float32)
        pairs.append((CvoPointCloud.from_xyz(s), CvoPointCloud.from_xyz(t), init))
    n_it = int(rs.choice([150, 400, 0]))
    gpu = CvoGPU(params=P)
    t0 = time.perf_counter()
    res = gpu.align_batch([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], max_iterations=n_it)
    dt = time.perf_counter() - t0
    adopted = sum(gpu.debug_speculation(q)[0] for q in range(n_pairs))
    solo = CvoGPU(params=P)
    diff = [q for q, (p, r) in enumerate(zip(pairs, res)) if _key(r) != _key(_solo_traced(solo, p[0], p[1], p[2], n_it))]
    print(f"soak trial {trial}: {n_pairs} pairs, ell {P.ell_init} K {P.nearest_neighbors_max}, {n_it or 'full'} "
          f"iterations, batch {dt:.2f} s, adopted {adopted} of {sum(r.iterations for r in res)}")
    assert not diff, (trial, diff)
    assert adopted > 0


def test_queue_random_mix_equals_traced_solo():
    """test_gpu_queue.py's random mix (36 submissions of slab and clustered pairs with random iteration limits through
    six slots, polled at random): every result bit-identical to the traced solo run of the same pair and limit."""
    rng = np.random.default_rng(7)
    kinds = [cases.config2(n=1800, pair_id=1), cases.config2(n=2600, pair_id=2), cases.scene(n=2200, pair_id=3)]
    P = kinds[0][0]
    gpu = CvoGPU(params=P)
    dev = [(gpu.upload(k[1]), gpu.upload(k[2]), k[3]) for k in kinds]
    jobs = [(int(rng.integers(0, 3)), int(rng.choice([15, 60, 140, 260]))) for _ in range(36)]
    solo = {}
    for kind, lim in sorted(set(jobs)):
        s, t, T = dev[kind]
        solo[(kind, lim)] = _solo_traced(gpu, s, t, T, lim)
    q = gpu.open_queue(6, 2600, 2600, min_source_points=1800, max_iterations=300)
    got = []
    for kind, lim in jobs:
        s, t, T = dev[kind]
        q.submit(s, t, T, lim)
        if rng.random() < 0.5:
            got.extend(q.poll(wait=int(rng.integers(0, 2))))
    while q.pending():
        got.extend(q.poll(wait=1))
    q.close()
    assert [r.ticket for r in got] == list(range(36))
    for r, (kind, lim) in zip(got, jobs):
        assert _key(r) == _key(solo[(kind, lim)]), (r.ticket, kind, lim)
