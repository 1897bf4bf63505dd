"""The multi-frame trust-region solve on its own, without a GPU: host/cvo_irls_solve_check (cvo_irls_solve.h over plain
host evaluations of the edges' records) against np_multiframe.solve on the same inputs.  Steps, accepted steps and the
termination must be equal, costs within rel 1e-8 and poses within 1e-6: what tests/test_gpu_multiframe.py holds the
device path to.  The program's switches inject what no finite cloud reaches, so terminations 4 (trust-region radius
below its minimum) and 6 (five invalid steps in a row) are asserted here."""
import os
import subprocess

import numpy as np
import pytest

import np_multiframe as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "cvo_irls_solve_check")
I12 = np.eye(4)[:3].reshape(12)
FAIL_STATUS = 7  # what --fail-normal / --fail-cost make the callback return


def _run(tmp_path, X, held, edges_terms, cap, *switches):
    """The program on (X, held, edges_terms, cap), every double written as a hex float.  Returns (X, dict)."""
    assert os.path.exists(EXE), "host/cvo_irls_solve_check is missing: run `make -C host`"
    hx = lambda v: " ".join(float(x).hex() for x in v)  # noqa: E731
    lines = [f"frames {len(X)}"] + [f"{int(h)} {hx(x)}" for h, x in zip(held, X)] + [f"cap {cap}", f"edges {len(edges_terms)}"]
    for f1, f2, P1, P2, w in edges_terms:
        lines.append(f"{f1} {f2} {len(w)}")
        lines += [hx(list(a) + list(b) + [c]) for a, b, c in zip(P1, P2, w)]
    path = tmp_path / "problem.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([EXE, str(path), *switches], text=True, timeout=60).splitlines()
    o = {l.split()[0]: l.split()[1] for l in out if not l.startswith("pose ")}
    o = {k: float.fromhex(v) if k.startswith("cost") else int(v) for k, v in o.items()}
    got = np.array([[float.fromhex(v) for v in l.split()[2:]] for l in out if l.startswith("pose ")]).reshape(-1, 12)
    return got, o


def _eval_cost(terms):
    return lambda Y: sum(0.5 * float(np.sum(nm.edge_terms(P1, P2, w, Y[f1], Y[f2])[0] ** 2)) for f1, f2, P1, P2, w in terms)


def _edge(rs, f1, f2, T1, T2, n):
    """n terms of edge (f1, f2): points of one cloud seen from both frames (true poses T1, T2), 1 cm of noise."""
    world = rs.uniform(-2, 2, (n, 3))
    to_frame = lambda T: (world - T.reshape(3, 4)[:, 3]) @ T.reshape(3, 4)[:, :3]  # noqa: E731
    return f1, f2, to_frame(T1) + rs.normal(0, 0.01, (n, 3)), to_frame(T2) + rs.normal(0, 0.01, (n, 3)), rs.uniform(0.2, 0.9, n)


def _plain():
    """Two frames, frame 0 held, 200 terms; frame 1 starts a twist of (0.05, -0.02, 0.03, 0.02, -0.01, 0.015) off."""
    rs = np.random.default_rng(17)
    X = np.stack([I12, nm.plus(I12, [0.05, -0.02, 0.03, 0.02, -0.01, 0.015])])
    return X, [True, False], [_edge(rs, 0, 1, I12, I12, 200)]


def _compare(tmp_path, X, held, terms, cap):
    free = ~np.array(held)
    want, o = nm.solve(X, free, terms, cap, _eval_cost(terms))
    got, c = _run(tmp_path, X, held, terms, cap)
    print({k: o[k] for k in ("steps", "accepted", "termination", "cost_initial", "cost_final")}, "".join(e[0] for e in o["events"]), c)
    assert c["status"] == 0
    assert (c["steps"], c["accepted"], c["termination"]) == (o["steps"], o["accepted"], o["termination"])
    assert c["cost_initial"] == pytest.approx(o["cost_initial"], rel=1e-8)
    assert c["cost_final"] == pytest.approx(o["cost_final"], rel=1e-8)
    assert np.max(np.abs(got - want)) <= 1e-6
    assert np.array_equal(got[~free].view(np.uint64), X[~free].view(np.uint64))  # a held frame's pose: the same bits
    return o


def test_plain_problem_matches_restatement(tmp_path):
    X, held, terms = _plain()
    o = _compare(tmp_path, X, held, terms, 50)
    # the draw is there for a solve that rejects steps, accepts others and ends on a tolerance before the cap
    assert o["steps"] > o["accepted"] > 0 and o["termination"] in (nm.TERM_FUNCTION, nm.TERM_GRADIENT, nm.TERM_PARAMETER)
    assert o["cost_final"] < 0.1 * o["cost_initial"]


def test_step_cap(tmp_path):
    X, held, terms = _plain()
    o = _compare(tmp_path, X, held, terms, 3)
    assert (o["steps"], o["termination"]) == (3, nm.TERM_ITERATIONS)


def test_held_frame_in_the_middle_and_reversed_edges(tmp_path):
    """Three frames, the middle one held, edges (1, 0), (2, 1), (0, 2): the free-index map (frame 2 is unknown 1) and the
    placement of every H block - held-free, free-held and the off-diagonal free-free one - show in the same fields."""
    rs = np.random.default_rng(23)
    T = [nm.plus(I12, [0.3, 0.0, -0.1, 0.0, 0.05, 0.0]), I12, nm.plus(I12, [-0.2, 0.1, 0.0, 0.02, 0.0, -0.04])]
    X = np.stack([nm.plus(T[0], [0.03, 0.01, -0.02, 0.01, -0.02, 0.01]), T[1], nm.plus(T[2], [-0.02, 0.03, 0.01, -0.015, 0.01, 0.02])])
    terms = [_edge(rs, a, b, T[a], T[b], n) for (a, b), n in zip([(1, 0), (2, 1), (0, 2)], (120, 90, 70))]
    o = _compare(tmp_path, X, [False, True, False], terms, 50)
    assert o["accepted"] > 0 and o["cost_final"] < 0.1 * o["cost_initial"]


def test_every_frame_held(tmp_path):
    X, _, terms = _plain()
    o = _compare(tmp_path, X, [True, True], terms, 50)
    assert (o["steps"], o["termination"]) == (0, nm.TERM_GRADIENT)


def test_nan_step_cost_ends_on_invalid_steps(tmp_path):
    """Termination 6: five invalid steps in a row (max_num_consecutive_invalid_steps), nothing accepted, X as given."""
    X, held, terms = _plain()
    want, o = nm.solve(X, ~np.array(held), terms, 50, lambda Y: float("nan"))
    assert (o["steps"], o["accepted"], o["termination"], o["events"]) == (5, 0, nm.TERM_INVALID, ["invalid"] * 5)
    got, c = _run(tmp_path, X, held, terms, 50, "--nan-cost")
    assert (c["status"], c["steps"], c["accepted"], c["termination"]) == (0, 5, 0, nm.TERM_INVALID)
    assert c["cost_initial"] == pytest.approx(o["cost_initial"], rel=1e-8) and c["cost_final"] == c["cost_initial"]
    assert np.array_equal(got.view(np.uint64), X.view(np.uint64)) and np.array_equal(want, X)


def test_rejected_steps_end_on_the_minimum_radius(tmp_path):
    """Termination 4: a synthetic normal (cost 1, every g 1e24, H 0) under a step cost that is always twice the current
    one.  Every step is rejected; the radius goes 1e4 / 2^(k(k+1)/2) and falls below 1e-32 at the 15th."""
    X = np.stack([I12, I12])
    held, terms = [True, False], [(0, 1, np.zeros((1, 3)), np.zeros((1, 3)), np.ones(1))]
    synthetic = lambda P1, P2, w, T1, T2: (1.0, np.full(12, 1e24), np.zeros((12, 12)))  # noqa: E731
    want, o = nm.solve(X, ~np.array(held), terms, 100, lambda Y: 2.0, normal=synthetic)
    assert (o["steps"], o["accepted"], o["termination"], o["events"]) == (15, 0, nm.TERM_RADIUS, ["reject"] * 15)
    assert 1e4 / 2.0 ** (14 * 15 / 2) >= nm.MIN_TRUST_REGION_RADIUS > 1e4 / 2.0 ** (15 * 16 / 2)
    got, c = _run(tmp_path, X, held, terms, 100, "--synthetic-normal", "--double-cost")
    assert (c["status"], c["steps"], c["accepted"], c["termination"]) == (0, 15, 0, nm.TERM_RADIUS)
    assert c["cost_initial"] == c["cost_final"] == 1.0
    assert np.array_equal(got.view(np.uint64), X.view(np.uint64)) and np.array_equal(want, X)


@pytest.mark.parametrize("switch", ["--fail-normal", "--fail-cost"])
def test_failing_callback_returns_its_status(tmp_path, switch):
    X, held, terms = _plain()
    got, c = _run(tmp_path, X, held, terms, 50, switch)
    assert c["status"] == FAIL_STATUS and (c["steps"], c["accepted"], c["termination"]) == (0, 0, nm.TERM_NONE)
    assert np.array_equal(got.view(np.uint64), X.view(np.uint64))
