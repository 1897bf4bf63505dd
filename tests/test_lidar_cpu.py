"""LiDAR front end, CPU twin (cvo_lidar_select_host) against the numpy statement np_lidar.py: indices, is_edge and the draws
consumed are equal on every case; the library's atan2 against numpy's; the generator against the C library's own rand(); every
refusal by its return code - cvo_lidar_select_host takes no context, so there is no error text to read here: the messages
of the same refusals are checked through a context in tests/test_gpu_lidar.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import lidar_cases as lc
import np_lidar
from unified_cvo_amd import CvoError, LidarConfig, LidarRand, LidarScan, _capi, debug_lidar_atan2, lidar_select_host


def _copy(rand):
    r = LidarRand()
    C.memmove(C.byref(r.c), C.byref(rand.c), C.sizeof(r.c))
    return r


@pytest.mark.parametrize("name", lc.CASES)
def test_twin_equals_the_statement(name):
    scan, cfg = lc.case(name)
    want = lc.statement(name)
    rand = LidarRand(1)
    start = _copy(rand)
    index, is_edge = lidar_select_host(scan, cfg, rand)
    assert np.array_equal(index, want["index"]) and np.array_equal(is_edge, want["is_edge"]), name
    for _ in range(want["draws"]):
        start.next()
    assert start.state() == rand.state(), name  # exactly the statement's draws were consumed
    assert want["segmented"] > 0 and want["edges"] > 0 and 0 < want["thinned"] < want["draws"]


def test_the_cases_reach_their_branches():
    """Statement-side: what each case was made for is there."""
    st = lc.statement("room16")
    assert st["valid"] >= 3 and st["invalid"] >= 1 and st["ground"] >= 1 and st["occluded"] >= 1 and st["edge_detected"] > 0
    # More than 20 edge candidates in a sixth need more than 20 x 11 points in it (a pick suppresses 5 neighbours on either
    # side), a ring of 1320 or more columns: the cap is reached on the 1800-column images, not at 256 columns.
    assert lc.statement("hdl64")["capped"] >= 1 and lc.statement("cap")["capped"] >= 1 and st["capped"] == 0
    scan, cfg = lc.case("hdl64")
    assert cfg.n_scan == 64 and cfg.horizon_scan == 1800 and 110000 < scan.n < 120000
    H = cfg_small_H = lc.SMALL["H"]
    seam, cfg = lc.statement("seam"), lc.case("seam")[1]
    c = lc.component_of(seam, cfg, 13, H - 1)
    assert c is lc.component_of(seam, cfg, 13, 0) and len(c["cells"]) == 12 and c["valid"] and c["seed"] == 13 * H
    for name, cell, size, valid in (("size4", (13, 200), 4, False), ("size5_valid", (13, 200), 5, True), ("size5_seed_alone", (13, 201), 5, False),
                                    ("size29", (13, 190), 29, False), ("size30", (14, 185), 30, True)):
        c = lc.component_of(lc.statement(name), lc.case(name)[1], *cell)
        assert c is not None and len(c["cells"]) == size and c["valid"] == valid and c["seed"] == cell[0] * cfg_small_H + cell[1], name
    col = lc.statement("collide")
    scan, cfg = lc.case("collide")
    assert np_lidar.frange(*(scan.xyzi[:, k] for k in range(3))).min() < cfg.sensor_min_range
    assert col["projected"] < scan.n - 3  # duplicates and short returns hold no cell of their own
    extra = lc.statement("extra_rings")
    assert extra["ring"].max() == lc.SMALL["R"] + 2 and extra["win"].max() < np.nonzero(extra["ring"] >= lc.SMALL["R"])[0].min()
    thin = lc.statement("thin_ring")
    rows = np.array(thin["seg_cell"]) // H
    assert 0 < np.count_nonzero(rows == 14) < 12 and np.count_nonzero(rows == 15) == 0 and not any(s[0] >= 14 for s in thin["sixths"])
    ties = lc.statement("ties")
    top = [s for s in ties["sixths"] if s[0] == lc.TOP]
    tied = [[k for k in range(sp, ep + 1) if ties["curvature"][k] == np.float32(0.390625)] for _, _, sp, ep in top]
    assert sorted(len(t) for t in tied)[-1] == 2  # two equal curvatures above the threshold in one sixth
    assert not np.array_equal(lc.statement("spill")["index"], lc.statement("spill", 1, True)["index"])  # suppression crosses a sixth boundary
    sem = lc.statement("semantic")
    scan, _ = lc.case("semantic")
    assert np.count_nonzero(scan.semantic == -1) > 100 and not np.any(scan.semantic[sem["index"]] == -1)
    dark = lc.case("dark")[0].xyzi
    assert np.count_nonzero(dark[:, 3] == 0) > 50 and all(np.count_nonzero(dark[:, k] == 0) >= 2 for k in range(3))
    chosen = dark[lc.statement("dark")["index"][:lc.statement("dark")["edge_detected"]]]
    assert np.all(chosen != 0)


@pytest.mark.parametrize("name", lc.EDGE_CASES)
def test_twin_equals_the_statement_at_the_edges(name):
    """The structural cases (lc.EDGE_CASES): indices, is_edge and draws, all exact; a result may be empty here."""
    scan, cfg = lc.case(name)
    want = lc.statement(name)
    rand = LidarRand(1)
    start = _copy(rand)
    index, is_edge = lidar_select_host(scan, cfg, rand)
    assert index.dtype == want["index"].dtype and np.array_equal(index, want["index"]) and np.array_equal(is_edge, want["is_edge"]), name
    for _ in range(want["draws"]):
        start.next()
    assert start.state() == rand.state(), name


def _np2(length):
    n = 64
    while n < length:
        n *= 2
    return n


def _transitions(st):
    return np.nonzero(np.diff(st["ring"]))[0] + 1


# which of these counts are zero in the empty and tiny cases; every other one of the four is positive
ZERO = {"n1": ("segmented", "draws", "edges"), "n3": ("segmented", "draws", "edges"), "all_near": ("projected", "segmented", "draws", "edges"),
        "blob30_alone": ("edges",), "blob11_alone": ("segmented", "draws", "edges"), "blob5_alone": ("draws", "edges"), "R1": ("edges",),
        "w255": (), "w257": ()}


def test_the_edge_cases_reach_their_edges():
    """Statement-side: every structural class the edge cases were drawn for is there, so that a case that stops reaching its
    edge fails here and does not pass vacuously on the device."""
    # k_lidar_pick's sort: the power of two at or above a sixth's entries, 64 at the least; 1024 is the class whose
    # compare-exchange loop makes a second trip
    classes = {name: {_np2(ep - sp) for _, _, sp, ep in lc.statement(name)["sixths"]} for name in lc.WIDE}
    assert classes == {"wide700": {64, 128}, "wide1200": {128, 256}, "wide2400": {256, 512}, "wide4096": {1024}}, classes
    lens = {name: sorted(ep - sp for _, _, sp, ep in lc.statement(name)["sixths"]) for name in lc.WIDE}
    assert (lens["wide700"][0], lens["wide700"][-1]) == (60, 114) and (lens["wide1200"][0], lens["wide1200"][-1]) == (101, 198)
    assert 1024 not in {_np2(ep - sp) for name in lc.CASES for _, _, sp, ep in lc.statement(name)["sixths"]}  # (the sixteen stop at 512)
    wide, cfg = lc.statement("wide4096"), lc.case("wide4096")[1]
    thr = np.float32(cfg.edge_threshold)
    above = [int(np.count_nonzero(wide["curvature"][sp:ep + 1] > thr)) for i, _, sp, ep in wide["sixths"] if i == 3]
    assert [ep - sp for i, _, sp, ep in wide["sixths"] if i == 3] == [680] * 6 and min(above) >= 113 and max(above) <= 115, above
    # every sixth of the case is above 512 entries, six of them stop at the cap: the order of the sort's top decides the output
    assert min(lens["wide4096"]) > 512 and wide["capped"] == 6 and wide["edges"] == 153
    # the row mask: four words of 32 rows; a small component's validity is its row count, the seed's row left out
    tall, cfg = lc.statement("tall128"), lc.case("tall128")[1]
    assert cfg.n_scan == 128 and cfg.ground_scan_ind == 20
    words = set()
    for cells, valid in lc.TALL_BLOBS:
        c = lc.component_of(tall, cfg, *cells[0])
        want = sorted(r * cfg.horizon_scan + col for r, col in cells)
        assert c is not None and sorted(c["cells"]) == want and c["valid"] == valid and c["seed"] == want[0] == c["cells"][0], cells
        rows = {cell // cfg.horizon_scan for cell in c["cells"][1:]}
        assert (len(rows) >= 3) == valid and len(cells) in (5, 6)
        words.add(tuple(sorted({r // 32 for r in rows})))
    assert words == {(0, 1), (2,), (1, 2), (2, 3), (3,)}  # every word, and a small component across each word boundary
    ground, cfg = lc.statement("tall128_ground"), lc.case("tall128_ground")[1]
    assert cfg.ground_scan_ind == cfg.n_scan - 1 == 127 and ground["ground"] > tall["ground"] and ground["segmented"] > 0
    assert ground["ground_cells"][22 * cfg.horizon_scan:].any() and not tall["ground_cells"][22 * cfg.horizon_scan:].any()
    # the ring id: block offset + wave counts + inclusive lane count, in blocks of 1024 and waves of 64
    res = {name: {int(t) % 1024 for t in _transitions(lc.statement(name))} for name in lc.SKIP}
    assert 1023 in res["skip1"] and 1022 in res["skip2"] and 63 in res["skip193"] and 65 in res["skip191"] and 1 in res["skip255"]
    assert {r % 64 for r in res["skip65"]} == {63} and {r % 64 for r in res["skip193"]} == {63} and {r % 64 for r in res["skip63"]} == {1}
    assert {r % 8 for name in lc.CASES if name != "extra_rings" for r in _transitions(lc.statement(name))[:3]} == {0}  # (the sixteen: lanes 0, 8, 16 ...)
    first = lc.statement("skip255")
    assert _transitions(first)[0] == 1 and 1025 in _transitions(first) and np.count_nonzero(first["ring"] == 0) == 1  # a ring of one point
    for name in lc.SKIP:
        assert lc.case(name)[0].n == 4096 - lc.SKIP[name] and lc.statement(name)["ring"].max() == 15, name
    last, scan = lc.statement("last_opens"), lc.case("last_opens")[0]
    assert _transitions(last)[-1] == scan.n - 1 and np.count_nonzero(last["ring"] == 15) == 1 and last["win"][15 * lc.SMALL["H"]:].max() == scan.n - 1
    lone, H = lc.statement("one_point_ring"), lc.SMALL["H"]
    assert np.count_nonzero(lone["ring"] == lc.LONE_RING) == 2 and np.count_nonzero(lone["win"][lc.LONE_RING * H:(lc.LONE_RING + 1) * H] >= 0) == 1
    assert lone["ring"].max() == 15 and np.count_nonzero(lone["ring"] == lc.LONE_RING + 1) == H
    # shapes that make k_lidar_union merge many trees late
    for name, (seed, size) in lc.SHAPES.items():
        st, cfg = lc.statement(name), lc.case(name)[1]
        c = lc.component_of(st, cfg, *seed)
        assert c is not None and len(c["cells"]) == size and c["valid"] and c["seed"] == seed[0] * H + seed[1], name
    loop = lc.component_of(lc.statement("loop"), lc.case("loop")[1], 14, 0)
    assert sorted(loop["cells"]) == list(range(14 * H, 15 * H))  # closed through the seam
    assert lc.case("comb")[1].ground_scan_ind == 8
    # empty and tiny results
    for name, zero in ZERO.items():
        st = lc.statement(name)
        assert all((st[k] == 0) == (k in zero) for k in ("projected", "segmented", "draws", "edges")), (name, {k: st[k] for k in zero})
    assert [lc.case(name)[0].n for name in ("n1", "n3")] == [1, 3] and all(len(lc.statement(name)["index"]) == 0 for name in ("n1", "n3"))
    assert [name for name in lc.EDGE_CASES if len(lc.statement(name)["index"]) == 0] == ["n1", "n3"]  # (edge_detection picks elsewhere)
    near = lc.statement("all_near")
    assert near["edge_detected"] == 1097 == len(near["index"])
    alone = lc.statement("blob30_alone")
    assert (alone["segmented"], alone["draws"], alone["valid"], alone["invalid"]) == (30, 20, 1, 0) and set(np.array(alone["seg_cell"]) // H) == {14}
    b11 = lc.statement("blob11_alone")
    assert (b11["projected"], b11["valid"], b11["invalid"]) == (11, 0, 1)
    assert 0 < lc.statement("blob5_alone")["segmented"] < 11  # no position has a curvature
    r1, cfg = lc.statement("R1"), lc.case("R1")[1]
    assert cfg.n_scan == 1 and cfg.ground_scan_ind == 0 and lc.case("R1")[0].n == 256 and r1["ring"].max() == 0 and r1["segmented"] > 10
    assert [lc.case(name)[1].horizon_scan for name in ("w255", "w257")] == [255, 257]
    # the largest image the validator admits
    scan, cfg = lc.case("max")
    big = lc.statement("max")
    assert (cfg.n_scan, cfg.horizon_scan, cfg.ground_scan_ind) == (128, 4096, 100) and scan.n == big["projected"] == 128 * 4096
    assert big["segmented"] > 100000 and 1024 in {_np2(ep - sp) for _, _, sp, ep in big["sixths"]}
    assert all(lc.case(name)[0].n <= 33000 for name in lc.EDGE_CASES if name != "max")


def test_shared_atan2_against_numpy():
    """lidar_atan2_deg of cvo_lidar_math.h - the copy the twin and the kernels compile, through cvo_debug_lidar_atan2 - on a
    dense grid that includes the axes and on 200 000 points of the unit circle: within 1e-6 degrees of numpy's arctan2, and
    bit for bit the statement's restatement (np_lidar.atan2_deg), which is held to the same bound."""
    v = np.concatenate([np.linspace(-50, 50, 1201), [0.0, 1e-30, -1e-30, 1e30, -1e30]])
    y, x = np.meshgrid(v, v)
    ang = np.radians(np.random.default_rng(0).uniform(-180, 180, 200000))
    for yy, xx in ((y, x), (np.sin(ang), np.cos(ang)), (np.array([0.0, 1.0, 0.0, -1.0, 0.0]), np.array([1.0, 0.0, -1.0, 0.0, 0.0]))):
        lib, stated, want = debug_lidar_atan2(yy, xx), np_lidar.atan2_deg(yy, xx), np.degrees(np.arctan2(yy, xx))
        want = np.where((yy == 0) & (xx == 0), 0.0, want)
        assert lib.shape == want.shape and np.array_equal(lib.view(np.int64), np.asarray(stated, np.float64).view(np.int64))
        assert np.abs(lib - want).max() < 1e-6 and np.abs(stated - want).max() < 1e-6
    assert list(debug_lidar_atan2(np.array([0.0, 1.0, 0.0, -1.0, 0.0]), np.array([1.0, 0.0, -1.0, 0.0, 0.0]))) == [0, 90, 180, -90, 0]


def test_generator_is_glibc_rand():
    libc = C.CDLL(None)
    if not hasattr(libc, "gnu_get_libc_version"):
        pytest.skip("not glibc: its rand() is another generator")
    for seed in (1, 12345):
        libc.srand(seed)
        want = [libc.rand() for _ in range(10000)]
        ours, stated = LidarRand(seed), np_lidar.Rand(seed)
        # (LidarRand.next is cvo_lidar_rand_next: the stepping function the library's calls draw with)
        assert [ours.next() for _ in range(10000)] == want and [stated.next() for _ in range(10000)] == want, seed
    libc.srand(1)


def test_chained_frames_equal_one_statement_run():
    rand, stated = LidarRand(12345), np_lidar.Rand(12345)
    for name in ("room16", "dark"):
        scan, cfg = lc.case(name)
        want = np_lidar.select(scan.xyzi, cfg, stated, scan.semantic)
        index, is_edge = lidar_select_host(scan, cfg, rand)
        assert np.array_equal(index, want["index"]) and np.array_equal(is_edge, want["is_edge"]), name
    assert rand.next() == stated.next()
    assert not np.array_equal(lidar_select_host(*lc.case("dark"), LidarRand(1))[0], want["index"])  # (the seed matters)


def _refused(scan_s, cfg_c, rand, code, n_points):
    index, edge, n = np.full(2 * max(n_points, 1), -7, np.int32), np.full(2 * max(n_points, 1), 7, np.uint8), C.c_int(-7)
    before = rand.state() if rand is not None else None
    rc = _capi.lib().cvo_lidar_select_host(C.byref(scan_s) if scan_s is not None else None, C.byref(cfg_c) if cfg_c is not None else None,
                                           C.byref(rand.c) if rand is not None else None, index.ctypes.data_as(C.POINTER(C.c_int)),
                                           edge.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(n))
    assert rc == code and n.value == -7 and np.all(index == -7) and np.all(edge == 7)
    assert rand is None or rand.state() == before


BAD_FIELDS = (("n_scan", 0), ("n_scan", 129), ("horizon_scan", 0), ("horizon_scan", 4097), ("ang_res_x", 0.0), ("ang_res_x", float("nan")),
              ("ground_scan_ind", -1), ("ground_scan_ind", 16), ("sensor_min_range", 0.0), ("sensor_mount_angle", 46.0), ("segment_theta", 0.0),
              ("segment_theta", 1.6), ("segment_alpha_x", -0.1), ("segment_alpha_y", 2.0), ("segment_valid_point_num", 0),
              ("segment_valid_line_num", 0), ("edge_threshold", 0.0), ("surf_threshold", -1.0), ("intensity_bound", 0.0),
              ("depth_bound", float("inf")), ("distance_bound", -1.0), ("beam_num", 0))


def test_refusals_write_nothing():
    scan, cfg = lc.case("room16")
    rand = LidarRand(1)
    s = scan.c_struct()
    _refused(None, cfg.c, rand, _capi.CVO_E_INVALID, scan.n)
    _refused(s, None, rand, _capi.CVO_E_INVALID, scan.n)
    _refused(s, cfg.c, None, _capi.CVO_E_INVALID, scan.n)
    for field, value in BAD_FIELDS:
        bad = lc.small_config()
        setattr(bad.c, field, value)
        _capi.lib().cvo_lidar_config_derive(C.byref(bad.c))
        _refused(s, bad.c, rand, _capi.CVO_E_INVALID, scan.n)
    stale = lc.small_config()
    stale.c.segment_theta = 0.9  # the derived tangent no longer matches
    _refused(s, stale.c, rand, _capi.CVO_E_INVALID, scan.n)
    for field, value in (("xyzi", None), ("n", 0), ("n", -3), ("num_classes", 4), ("num_classes", -1)):
        t = scan.c_struct()
        setattr(t, field, value)
        _refused(t, cfg.c, rand, _capi.CVO_E_INVALID, scan.n)
    for value in (float("nan"), float("inf"), -float("inf"), 2e15):
        for column in range(4):
            if value == 2e15 and column == 3:
                continue
            bad = LidarScan(scan.xyzi.copy())
            bad.xyzi[scan.n // 2, column] = value
            _refused(bad.c_struct(), cfg.c, rand, _capi.CVO_E_INVALID, scan.n)
    labels = np.zeros(scan.n, np.int32)
    labels[5] = 3
    _refused(LidarScan(scan.xyzi, labels, 3).c_struct(), cfg.c, rand, _capi.CVO_E_INVALID, scan.n)
    unseeded = LidarRand(1)
    unseeded.c.front = 31
    _refused(s, cfg.c, unseeded, _capi.CVO_E_INVALID, scan.n)
    big = scan.c_struct()
    big.n = (1 << 24) + 1  # refused on its size, before a point is read
    _refused(big, cfg.c, rand, _capi.CVO_E_UNSUPPORTED, scan.n)
    with pytest.raises(CvoError, match="error -2"):
        lidar_select_host(LidarScan(np.zeros((0, 4), np.float32)), cfg, rand)
    assert rand.state() == LidarRand(1).state()


def test_default_config_is_the_hdl64_preset():
    c, s = LidarConfig(), LidarConfig(semantic=True)
    assert (c.n_scan, c.horizon_scan, c.ground_scan_ind, c.segment_valid_point_num, c.segment_valid_line_num, c.beam_num) == (64, 1800, 50, 5, 3, 64)
    assert c.ang_res_x == np.float32(0.2) and c.sensor_min_range == 1 and c.sensor_mount_angle == 0 and c.edge_threshold == np.float32(0.1)
    assert c.segment_theta == np.float32(60.0 / 180.0 * np.pi) and c.segment_alpha_x == np.float32(float(np.float32(0.2)) / 180.0 * np.pi)
    assert c.segment_alpha_y == np.float32(float(np.float32(0.427)) / 180.0 * np.pi)
    assert (c.intensity_bound, c.depth_bound, c.distance_bound, s.distance_bound) == (0.4, 4.0, 40.0, 75.0)
    assert abs(c.tan_theta - np.tan(c.segment_theta)) < 1e-12 and abs(c.tan_ground_hi - np.tan(np.radians(10))) < 1e-12 and c.tan_ground_lo == -c.tan_ground_hi
    assert abs(c.tan_self_hi - np.tan(np.radians(3))) < 1e-12 and abs(c.sin_alpha_x - np.sin(c.segment_alpha_x)) < 1e-15
