"""RGB-D front end, CPU twin (cvo_rgbd_points_host) against the numpy statement np_rgbd.py.  Every comparison is exact:
indices equal, float rows bit-equal.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import np_rgbd
import rgbd_cases as rc
from unified_cvo_amd import CvoError, RGBDFrame, _capi, rgbd_points_host, synth
from unified_cvo_amd.api import DSO_EDGES, FULL


def test_schedule_branches_of_the_statement():
    """The frames make every branch of dso_select_pixels' schedule run (the statement returns the potentials tried)."""
    seen = set()
    for name, (_, tried) in rc.FRAMES.items():
        if tried is None:
            continue
        f = rc.frame(name)
        uv, got, counts = np_rgbd.dso_select(np_rgbd.gray_plane(f.image))
        assert got == tried, (name, got, counts)
        seen.add(tuple(got))
        if name == "edge":
            assert counts[0] > 10000 and counts[1] < 6666 and len(uv) == counts[2] == counts[0]
        if name == "noisy720":
            assert min(counts) > 10000  # left the loop through `times == 5`, not through the count
    assert {(3, 4, 5), (3, 4), (3, 2), (3, 4, 3), (3, 4, 5, 6, 7)} <= seen


def test_gradient_is_exact_in_float32_and_has_perfect_squares():
    """dx, dy are multiples of 0.5, g2 a multiple of 0.25 below 2^16: float32 holds them exactly (no contraction can
    change them); int(sqrtf(g2)) must come out right at dx = 3, dy = 4."""
    for name in ("textured", "small", "mono"):
        f = rc.frame(name)
        I = np_rgbd.gray_plane(f.image, f.gray)
        grad, g2 = np_rgbd.gradient(I)
        I64 = I.astype(np.float64)
        dx = np.zeros_like(I64)
        dy = np.zeros_like(I64)
        dx[1:-1, 1:-1] = 0.5 * (I64[1:-1, 2:] - I64[1:-1, :-2])
        dy[1:-1, 1:-1] = 0.5 * (I64[2:, 1:-1] - I64[:-2, 1:-1])
        assert np.array_equal(grad.reshape(-1, 2)[:, 0].astype(np.float64), dx.reshape(-1))
        assert np.array_equal(g2.astype(np.float64), (dx * dx + dy * dy).reshape(-1))
        assert np.all(np.mod(g2.astype(np.float64) * 4, 1) == 0) and g2.max() < 2 ** 16
        assert np.count_nonzero(g2 == 25.0) > 0 and np.count_nonzero(g2 == 169.0) > 0, name
        assert np.all(np.sqrt(g2[g2 == 25.0]).astype(np.int64) == 5)


def test_threshold_index_aliases_on_odd_shapes():
    """200 x 150 reads block column 6 of 6 (the next block row's first entry); 1241 x 376 reads into the zero slack."""
    idx = np_rgbd.threshold_index(150, 200)[np_rgbd.considered(150, 200)]
    assert 200 // 32 == 6 and np.any(idx % 6 == 0) and idx.max() >= 24
    idx = np_rgbd.threshold_index(376, 1241)[np_rgbd.considered(376, 1241)]
    assert idx.max() >= (1241 // 32) * (376 // 32)


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_points_equal_the_statement(name, depth):
    f = rc.frame(name, depth)
    for method in (DSO_EDGES, FULL):
        rc.assert_points_equal(rgbd_points_host(f, method), rc.statement_points(f, method), (name, depth, method))


def _bins(name, bx, by):
    f, s = rc.edge_frame(name), rc.edge_statement(name)
    return rc.block_bins(s["g2"], f.rows, f.cols, bx, by), s["ths"][bx + by * (f.cols // 32)]


def test_the_edge_cases_reach_their_edges():
    """Each case of rc.EDGE_CASES does, on the statement, what its name says."""
    st = rc.edge_statement
    # shapes: the first considered pixel; blocks; 1024 cells at potential 2; the residues of every potential's 4 pot blocks
    assert not np_rgbd.considered(7, 9).any() and np_rgbd.considered(8, 10).sum() == 1
    assert [len(st("shape_7x9")["selected"][p]) for p in rc.POTS] == [0] * 6
    assert [len(st("shape_8x10")["selected"][p]) for p in (3, 2)] == [1, 1]
    assert st("shape_8x10")["points"][DSO_EDGES]["schedule"] == ([3, 2], [1, 1])
    assert {r * c for r, c in rc.STRUCTURE_SHAPES} >= {1023, 1024, 1025}
    for (r, c), blocks in (((31, 31), 0), ((31, 33), 0), ((25, 41), 0), ((32, 32), 1), ((33, 33), 1), ((63, 63), 1), ((64, 64), 4), ((65, 65), 4)):
        assert (r // 32) * (c // 32) == blocks and np.count_nonzero(st("shape_%dx%d" % (r, c))["ths"]) == blocks
    cells2 = {s: -(-s[0] // 2) * -(-s[1] // 2) for s in ((64, 64), (64, 65), (65, 64))}
    assert cells2 == {(64, 64): 1024, (64, 65): 1024 + 32, (65, 64): 1024 + 32}
    for pot in rc.POTS:
        for axis in (0, 1):
            assert {s[axis] % (4 * pot) for s in rc.RESIDUE_SHAPES} >= {0, 1, 4 * pot - 1}, (pot, axis)
    for name in rc.EDGE_CASES:
        f = rc.edge_frame(name)
        assert f.rows * f.cols <= 36 * 3205 and (name == "shape_36x3205" or max(f.rows, f.cols) <= 130), name
    # the threshold index: the next block row's first entry, the zero slack, and its last entry
    for (r, c), reach in (((63, 63), 2), ((33, 63), 1), ((64, 95), 4), ((95, 64), 5), ((36, 3205), 199)):
        idx = np_rgbd.threshold_index(r, c)[np_rgbd.considered(r, c)]
        assert idx.max() == reach and reach >= (r // 32) * (c // 32) and reach < len(st("shape_%dx%d" % (r, c))["sm"]), (r, c)
    idx = np_rgbd.threshold_index(64, 95)[np_rgbd.considered(64, 95)]
    assert np.any(idx == 2) and 95 // 32 == 2  # block column 2 of 2 in block row 0: the next block row's first entry
    assert len(st("shape_36x3205")["sm"]) == 200 and np.all(st("shape_36x3205")["sm"][100:] == 0)
    idx = np_rgbd.threshold_index(*rc.WIDE_REFUSED)[np_rgbd.considered(*rc.WIDE_REFUSED)]
    assert idx.max() == 200
    # histogram and quantile
    bins, th = _bins("hist_flat", 1, 1)
    assert bins[0] == 1024 and th == 7 and np.all(st("hist_flat")["sm"][:9] == 49)
    bins, th = _bins("hist_cap", 1, 1)
    g2 = st("hist_cap")["g2"][32:64, 32:64]
    assert np.all(np.sqrt(g2).astype(np.int64) == 127) and bins[48] == 1024 and th == 55
    bins, th = _bins("hist_47_48_49", 1, 1)
    roots = np.sqrt(st("hist_47_48_49")["g2"][32:64, 32:64]).astype(np.int64)
    assert [np.count_nonzero(roots == r) for r in (47, 48, 49)] == [256, 128, 640] and roots.min() == 47
    assert bins[47] == 256 and bins[48] == 768 and th == 48 + 7
    for name, extra, q in (("quantile_at", 0, 5), ("quantile_above", 1, 0)):
        for (bx, by), count in (((1, 1), 1024), ((1, 0), 992), ((2, 2), 961)):
            bins, th = _bins(name, bx, by)
            t = int(np.float32(count) * np.float32(0.5) + np.float32(0.5))
            assert bins.sum() == count and bins[0] == t + extra and bins[5] == count - t - extra and th == q + 7, (name, bx, by, bins[:6])
    roots = np.minimum(np.sqrt(st("hist_wave_ramp")["g2"][32:64, 32:64]).astype(np.int64), 48)
    assert all(len(np.unique(roots[2 * k:2 * k + 2])) >= 40 for k in range(16))
    ths = st("smooth_3x3")["ths"][:9]
    assert len(np.unique(ths)) == 9
    sm = st("smooth_3x3")["sm"][:9].reshape(3, 3)
    t = ths.reshape(3, 3).astype(np.float64)
    square = lambda total, n: np.float32(total / n) * np.float32(total / n)  # noqa: E731
    assert sm[0, 0] == square(t[:2, :2].sum(), 4) and sm[0, 1] == square(t[:2].sum(), 6) and sm[1, 1] == square(t.sum(), 9)
    # selection rules: the tie ...
    s = st("sel_tie")
    g2, w = s["g2"].reshape(-1), 96
    for pot in rc.POTS:
        tied = 0
        sel = set(s["selected"][pot].tolist())
        for y, x in rc.TIE_POKES:
            plus = [(y - 1) * w + x, y * w + x - 1, y * w + x + 1, (y + 1) * w + x]  # (row-major order)
            assert all(g2[p] == 900 for p in plus)
            cells = {}
            for p in plus:
                cells.setdefault((p // w // pot, p % w // pot), []).append(p)
            for members in cells.values():
                assert members[0] in sel and not sel & set(members[1:]), (pot, y, x)
                tied += len(members) > 1
        assert tied >= 10, pot
    # ... the threshold itself ...
    s = st("sel_threshold")
    (ye, xe), (ya, xa) = rc.THRESHOLD_EQUAL, rc.THRESHOLD_ABOVE
    assert s["g2"][ye, xe] == s["sm"][np_rgbd.threshold_index(64, 64)[ye, xe]] == 49 and s["g2"][ya, xa] == 49.25
    for pot in rc.POTS:
        assert ye * 64 + xe not in s["selected"][pot] and ya * 64 + xa in s["selected"][pot]
    # ... the considered region ...
    s = st("sel_border")
    h, w = rc.BORDER_SHAPE
    for targets in rc.border_targets():
        assert [c for _, _, c in targets] == [False, True, True, False]
        for y, x, is_considered in targets:
            assert s["g2"][y, x] == 3600 and np_rgbd.considered(h, w)[y, x] == is_considered
            for pot in rc.POTS:
                assert (y * w + x in s["selected"][pot]) == is_considered, (y, x, pot)
    # ... perfect squares in a histogrammed block, and gray levels on the rounding boundary
    g2 = st("sel_squares")["g2"]
    assert np.count_nonzero(g2[1:63, 1:63] == 25.0) > 0 and np.count_nonzero(g2[1:63, 1:63] == 169.0) > 0
    reached, missed = rc.bgr_boundary_triples()
    for trip, rem in ((reached, 0), (missed, (1 << 14) - 1)):
        assert len(trip) > 100 and np.all((1868 * trip[:, 0] + 9617 * trip[:, 1] + 4899 * trip[:, 2] + 8192) % (1 << 14) == rem)
    f = rc.edge_frame("bgr_rounding")
    px = f.image.reshape(-1, 3).astype(np.int64)
    rem = (1868 * px[:, 0] + 9617 * px[:, 1] + 4899 * px[:, 2] + 8192) % (1 << 14)
    assert f.channels == 3 and np.all((rem == 0) | (rem == (1 << 14) - 1)) and 400 < np.count_nonzero(rem == 0) < 1200
    # depth: every special value is met by both methods; a NaN coordinate comes from u == cx under an infinite depth
    for name, values in (("depth_f32", rc.DEPTH_F32), ("depth_u16", rc.DEPTH_U16)):
        f = rc.edge_frame(name)
        uv = st(name)["selected"][st(name)["points"][DSO_EDGES]["schedule"][0][-1]]
        for v in values:
            same = f.depth == v
            if f.depth.dtype == np.float32:
                same = np.isnan(f.depth) if np.isnan(v) else same & (np.signbit(f.depth) == np.signbit(v))
            assert same.any() and same.reshape(-1)[uv].any(), (name, v)
    p = st("depth_f32")["points"][FULL]
    nan = np.isnan(p["xyz"])
    assert nan[:, 0].any() and np.all(p["pixel"][nan[:, 0]] % 48 == 12) and np.all(np.isinf(p["xyz"][nan[:, 0], 2])) and not nan[:, 2].any()
    kept = rc.edge_frame("depth_f32").depth.reshape(-1)[p["pixel"]]
    assert np.any(kept == np.float32(1e-45)) and np.any(kept == -1.5) and not np.any(kept == 0)


def test_first_difference_names_the_stage_and_the_index():
    want = rc.edge_statement("shape_33x33")
    back = dict(g2=want["g2"].copy(), ths=want["ths"].copy(), sm=want["sm"].copy(), selected={p: v.copy() for p, v in want["selected"].items()})
    assert rc.first_difference(back, want) is None
    back["selected"][6] = back["selected"][6][:-1]
    assert "potential 6: %d entries for %d" % (len(back["selected"][6]), len(want["selected"][6])) in rc.first_difference(back, want)
    back["selected"][4][3] += 1
    assert "potential 4: 1 entries differ, first at 3" in rc.first_difference(back, want)
    back["sm"][100] = 1.0  # (the last slack entry of 1 + 100)
    assert "stage sm: 1 entries differ, first at 100: 1.0 for 0.0" in rc.first_difference(back, want)
    back["g2"][2, 5] += 0.25
    assert "stage g2: 1 entries differ, first at %d" % (2 * 33 + 5) in rc.first_difference(back, want)


@pytest.mark.parametrize("name", list(rc.EDGE_CASES))
def test_twin_equals_the_statement_on_the_edge_cases(name):
    f = rc.edge_frame(name)
    for method in (DSO_EDGES, FULL):
        rc.assert_points_equal(rgbd_points_host(f, method), rc.edge_statement(name)["points"][method], (name, method), name in rc.NAN_COORDINATES)


def test_the_widest_accepted_image_and_the_first_refused_one():
    f = rc.refused_frame()
    assert (f.rows, f.cols) == rc.WIDE_REFUSED
    with pytest.raises(np_rgbd.Unsupported):
        np_rgbd.dso_select(np_rgbd.gray_plane(f.image))
    assert _raw_call(f.c_struct(), DSO_EDGES) == _capi.CVO_E_UNSUPPORTED
    rc.assert_points_equal(rgbd_points_host(f, FULL), rc.statement_points(f, FULL), "refused, FULL")


def test_caller_gray_plane_overrides_the_formula():
    f = rc.own_gray(rc.frame("small"))
    got = rgbd_points_host(f, DSO_EDGES)
    rc.assert_points_equal(got, rc.statement_points(f, DSO_EDGES), "own-gray")
    assert not np.array_equal(got.pixel, rgbd_points_host(rc.frame("small"), DSO_EDGES).pixel)


def test_semantic_frame_drops_class_10_and_copies_rows():
    f = rc.frame("semantic")
    cls = np.argmax(f.semantic.reshape(-1, 19), axis=1)
    assert np.count_nonzero(cls == 10) > 1000
    for method in (DSO_EDGES, FULL):
        pc = rgbd_points_host(f, method)
        assert pc.num_classes() == 19 and not np.any(cls[pc.pixel] == 10)
        assert np.array_equal(pc.labels(), f.semantic.reshape(-1, 19)[pc.pixel])
    plain = RGBDFrame(f.image, f.depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor)
    assert rgbd_points_host(plain, FULL).num_points() > rgbd_points_host(f, FULL).num_points()


def test_all_zero_depth_is_an_empty_cloud():
    for depth in rc.DEPTHS:
        f = rc.zero_depth(rc.frame("small", depth))
        for method in (DSO_EDGES, FULL):
            pc = rgbd_points_host(f, method)
            assert pc.num_points() == 0 and len(pc.pixel) == 0


def test_full_is_column_major_with_type_half_half():
    f = rc.frame("small")
    pc = rgbd_points_host(f, FULL)
    u, v = pc.pixel % f.cols, pc.pixel // f.cols
    assert np.all(np.diff(u * f.rows + v) > 0) and np.any(np.diff(pc.pixel) < 0)
    assert np.all(pc.geometric_types_ == 0.5)
    e = rgbd_points_host(f, DSO_EDGES)
    assert np.all(e.geometric_types_ == np.array([0.9, 0.1], np.float32))


def test_gradient_index_quirk_matters():
    """Features 3 and 4 read gradient_[v w + u] and gradient_[v w + u + 1] of the interleaved array - the statement's
    values - and differ from the `intended` gradient_[2 (v w + u)], gradient_[2 (v w + u) + 1] on this frame."""
    f = rc.frame("small")
    pc = rgbd_points_host(f, DSO_EDGES)
    grad, _ = np_rgbd.gradient(np_rgbd.gray_plane(f.image))
    quirk = (grad[pc.pixel].astype(np.float64) / 500.0 + 0.5).astype(np.float32)
    intended = (grad[2 * pc.pixel].astype(np.float64) / 500.0 + 0.5).astype(np.float32)
    assert np.array_equal(pc.features()[:, 3], quirk)
    assert np.count_nonzero(pc.features()[:, 3] != intended) > len(quirk) // 4


def test_byte_round_trip_is_the_identity():
    c = np.arange(256)
    f = (c.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(np_rgbd.byte_round_trip(f), c.astype(np.uint8))


def test_recipe_of_the_statement_is_edges_then_surfaces():
    f = rc.frame("small")
    r = rc.statement_recipe(f, 0.1)
    ne = int(r["is_edge"].sum())
    assert 0 < ne < len(r["pixel"]) and np.all(r["is_edge"][:ne] == 1) and np.all(r["is_edge"][ne:] == 0)
    assert np.all(r["geotype"][:ne] == np.array([1, 0], np.float32)) and np.all(r["geotype"][ne:] == np.array([0, 1], np.float32))
    assert np.all(r["feat"][:, 3:] == 0)
    want = (f.image.reshape(-1, 3)[r["pixel"]].astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(r["feat"][:, :3], want)  # the pixel's channels over 255: the gradient features are dropped


def _raw_call(fs, method=FULL, pixel=True):
    L = _capi.lib()
    px = np.full(16, -7, np.int32)
    n = C.c_int(-7)
    rcode = L.cvo_rgbd_points_host(C.byref(fs), method, px.ctypes.data_as(C.POINTER(C.c_int)) if pixel else None, C.byref(n), None, None, None, None)
    assert n.value == -7 and np.all(px == -7)  # nothing written on a refusal
    return rcode


def test_refusals():
    f = rc.frame("tiny")
    for field, value in (("rows", 0), ("cols", -1), ("channels", 2), ("channels", 4), ("image", None), ("depth", None), ("depth_type", 5),
                         ("fx", 0.0), ("fx", float("nan")), ("fy", -1.0), ("fy", float("inf")), ("scaling_factor", 0.0),
                         ("scaling_factor", float("nan")), ("num_classes", 3)):
        fs = f.c_struct()
        setattr(fs, field, value)
        assert _raw_call(fs) == _capi.CVO_E_INVALID, (field, value)
    assert _raw_call(f.c_struct(), pixel=False) == _capi.CVO_E_INVALID
    for method in (0, 1, 3, 4, 5, 6, 7):  # CV_FAST, RANDOM ... LOAM: OpenCV detectors, rand(), LiDAR
        assert _raw_call(f.c_struct(), method) == _capi.CVO_E_UNSUPPORTED
    assert _raw_call(f.c_struct(), 9) == _capi.CVO_E_INVALID and _raw_call(f.c_struct(), -1) == _capi.CVO_E_INVALID
    with pytest.raises(CvoError):
        bad = rc.frame("tiny")
        bad.fx = 0.0
        rgbd_points_host(bad, FULL)
    # images under 32 pixels on a side are valid: zero whole blocks, zero thresholds
    assert rgbd_points_host(f, DSO_EDGES).num_points() > 0


def test_threshold_index_beyond_the_allocation_is_unsupported():
    """A 3210 x 36 image: (x >> 5) + (y >> 5) * (cols / 32) reaches 100 + 1 * 100 of 100 * 1 + 100 entries (it takes more
    than 100 block columns and a ragged last block row)."""
    rows, cols = 36, 3210
    img = np.zeros((rows, cols), np.uint8)
    f = RGBDFrame(img, np.ones((rows, cols), np.uint16), 500, 500, 1600, 18, 5000)
    assert ((rows - 4) >> 5) * (cols // 32) + ((cols - 6) >> 5) >= (cols // 32) * (rows // 32) + 100
    with pytest.raises(np_rgbd.Unsupported):
        np_rgbd.dso_select(np_rgbd.gray_plane(f.image))
    assert _raw_call(f.c_struct(), DSO_EDGES) == _capi.CVO_E_UNSUPPORTED
    assert rgbd_points_host(f, FULL).num_points() == rows * cols
