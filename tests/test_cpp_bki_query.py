"""The read side of the semantic voxel map through the C++ side: host/cvo_bki_query_check builds
semantic_bki::SemanticBKIOctoMap, fills it with the driver's statements and asks it through search (upstream's names:
SemanticOcTreeNode::get_state / get_semantics / get_probs / get_vars / get_features), raycast and render - the CPU twin, and
the device under -m gpu - against the numpy statement (np_bki_query.py), by hash over the bytes."""
import os
import subprocess

import numpy as np
import pytest

import bki_query_cases as qc
import cases

CHECK = os.path.join(cases.ROOT, "host", "cvo_bki_query_check")
NAMES = ("classes_19", "classes_0", "sparse", "one_hit_unknown", "sized_65", "room", "empty_prior", "key_range")  # (a frame without hits, as "wall" has, is beyond the driver's case file)
F32 = np.float32


def _fnv(parts):
    h = 14695981039346656037
    for a in parts:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _args(tmp, name):
    """the driver's arguments for the case: its frames, its points, its first ray batch and its first view"""
    c = qc.case(name)
    cfg, C = c.cfg, c.cfg.num_classes
    case_file = "-"
    if c.frames:
        rows = []
        for f, (xyz, feat, label, origin) in enumerate(c.frames):
            n = xyz.shape[0]
            lab = label if C else np.zeros((n, 0), F32)
            rows.append(np.concatenate([np.full((n, 1), f, F32), np.tile(origin, (n, 1)), xyz, feat, lab], axis=1))
        case_file = str(tmp / "case.npy")
        np.save(case_file, np.concatenate(rows).astype(F32))
    np.save(tmp / "points.npy", c.points)
    rays_file, mask, steps = "-", 0, 1
    if c.rays:
        o, e, mask, steps = c.rays[0]
        rays_file = str(tmp / "rays.npy")
        np.save(rays_file, np.concatenate([np.asarray(o, F32), np.asarray(e, F32)], axis=1))
    view_file = "-"
    if c.views:
        v = c.views[0]
        view_file = str(tmp / "view.npy")
        np.save(view_file, np.array([list(np.asarray(v["pose"], F32).reshape(12)) + [v["fx"], v["fy"], v["cx"], v["cy"], v["z_far"], v["rows"], v["cols"], v["stop_mask"]]], F32))
    return [case_file, C] + [repr(float(x)) for x in (cfg.resolution, cfg.prior, cfg.free_thresh, cfg.occupied_thresh, cfg.free_resolution, cfg.max_range)] + [
        c.kernel, repr(float(cfg.sf2)), repr(float(cfg.ell)), str(tmp / "points.npy"), rays_file, mask, steps, view_file]


def _want(name):
    c, w = qc.case(name), qc.expected(name)
    q = w["query"]
    per_point = [[q["found"][i], q["state"][i], q["semantics"][i], q["probs"][i], q["vars"][i], q["feat"][i], q["centre"][i]] for i in range(len(c.points))]
    out = [f"query {len(c.points)} " + _fnv([a for row in per_point for a in row]), "single " + _fnv(per_point[0])]
    if c.rays:
        r = w["rays"][0]
        rows = [[np.int32(r["status"][i]), r["steps"][i], r["key"][i], r["centre"][i], r["t"][i], np.int32(r["state"][i]), r["semantics"][i]] for i in range(len(r["t"]))]
        out.append(f"rays {len(rows)} " + _fnv([a for row in rows for a in row]))
    if c.views:
        v = w["views"][0]
        out.append(f"view {c.views[0]['rows']} {c.views[0]['cols']} " + _fnv([v["depth"], v["semantics"], v["feat"], v["label"]]))
    return out


def _check(tmp_path, extra=(), env=None):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    for name in NAMES:
        args = _args(tmp_path, name)
        out = subprocess.check_output([CHECK] + [str(a) for a in args] + list(extra), text=True, timeout=300, env=env).splitlines()
        assert out == _want(name), name


def test_twin_through_the_veneer(tmp_path):
    _check(tmp_path)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    args = [str(a) for a in _args(tmp_path, "one_hit_unknown")]
    for bad in (args[:14] + ["0"] + args[15:], args[:13] + ["16"] + args[14:], args + ["--what"]):  # max_steps 0, a mask of 16, an option
        res = subprocess.run([CHECK] + bad, capture_output=True, text=True)
        assert res.returncode == 1 and "cvo_bki_query_check:" in res.stderr, bad


@pytest.mark.gpu
def test_device_through_the_veneer(tmp_path):
    env = dict(os.environ, CVO_BKI_HOST="0")
    _check(tmp_path, extra=["--device", os.path.join(cases.ROOT, "configs", "geometric_gpu.yaml")], env=env)
