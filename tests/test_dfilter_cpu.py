"""The disparity post-filter without a GPU: the numpy statement (np_dfilter.py) against what libelas's own compiled passes left
of the golden map (tests/golden/dfilter_elas.npz, scripts/make_dfilter_golden.py), the CPU twin (cvo_disparity_filter_host)
against the statement on every case of dfilter_cases.py, the refusals, the no-op settings, out == in, and two properties.  All
comparisons are exact (bit patterns).

Quality figures (test_the_filter_does_not_raise_the_outlier_share; valid pixels and the share of them more than 1 from the
truth, before -> after the default filter, on sgm_cases.two_planes through the matcher's twin at max_disparity 64):
   64 x 200 seed 3: 11547 valid, 1.86 % -> 11395 valid, 0.33 %
   96 x 320 seed 0: 28878 valid, 1.17 % -> 28580 valid, 0.04 %
  120 x 160 seed 5: 16856 valid, 2.15 % -> 16552 valid, 0.13 %"""
import ctypes as C

import numpy as np
import pytest

import dfilter_cases as dc
import np_dfilter
import sgm_cases as sc
from unified_cvo_amd import CvoError, DFilterConfig, SGMConfig, _capi, disparity_filter_host, stereo_disparity_host

CASES = dc.cases()


def _config(cfg):
    return DFilterConfig(cfg.speckle_sim_threshold, cfg.speckle_size, cfg.ipol_gap_width, cfg.adaptive_mean)


def test_statement_equals_libelas_compiled_passes():
    g = dc.golden()
    assert np.array_equal(g["input"].view(np.uint32), dc.golden_input().view(np.uint32)), "the fixture is not of this generator: run scripts/make_dfilter_golden.py"
    st = np_dfilter.stages(g["input"])
    assert not dc.first_difference(st["speckle"], g["speckle"])
    assert not dc.first_difference(st["gap"], g["gap"])
    H, W = g["input"].shape
    band = np.zeros((H, W), bool)
    band[:, 3] = band[4:7, :] = band[H - 6:H - 3, :] = True
    assert not (~g["agree"] & ~band).any()              # libelas's runs differ only where it reads memory it never wrote
    assert np.array_equal(g["pinned"], g["agree"] & ~band) and g["pinned"].sum() > 0.9 * H * W
    bad = np.argwhere((st["out"].view(np.uint32) != g["mean"].view(np.uint32)) & g["pinned"])
    assert not len(bad), (len(bad), bad[:5].tolist())
    # every pass acted on the fixture
    assert (g["speckle"] != g["input"]).sum() > 200 and (g["gap"] != g["speckle"]).sum() > 100 and (g["mean"] != g["gap"]).sum() > 5000


def test_the_fixture_holds_what_it_was_built_for():
    d = dc.golden_input()
    st = dc.statement("golden")
    for value, n, kept in ((60, 199, False), (70, 200, True), (80, 201, True)):
        island = np.abs(d - value) < 0.5
        assert island.sum() == n and bool((st["speckle"][island] >= 0).all()) == kept and (kept or (st["speckle"][island] == -10).all())
    assert (st["gap"][33:38, 33:36] >= 0).all() and (st["gap"][42:46, 33:37] == -10).all() and (st["gap"][20:23, 70:75] >= 0).all()
    for hole in (np.s_[58:63, 0:2], np.s_[58:63, -2:], np.s_[0:2, 48:53], np.s_[-2:, 48:53]):  # holes at the line ends
        assert (st["gap"][hole] == -10).all(), hole
    assert (st["speckle"][25, 5:8] == -10).all() and st["speckle"][64, 40] == -10
    # the mean's three weight classes occur among horizontal neighbours
    diff = np.abs(np.diff(st["gap"], axis=1))[(st["gap"][:, 1:] >= 0) & (st["gap"][:, :-1] >= 0)]
    assert (diff < 2).any() and ((diff >= 2) & (diff < 8)).any() and (diff >= 8).any()


@pytest.mark.parametrize("name", list(CASES))
def test_twin_equals_the_statement(name):
    d, cfg = CASES[name]
    assert not dc.first_difference(disparity_filter_host(d, _config(cfg)), dc.statement(name)["out"])


def test_the_mean_weight_is_the_mask_libelas_compiles():
    """4 below a difference of 2, 2 in [2, 8), 0 from 8 on; the sign does not matter"""
    for diff, w in ((0, 4), (1.9999999, 4), (2, 2), (-2, 2), (7.9999995, 2), (8, 0), (-30, 0), (1e-30, 4)):
        assert np_dfilter._weights(np.float32(diff), np.float32(0)) == w, diff
    assert np.float32(0x7FFFFFFF).view(np.uint32) == np_dfilter.ABS_BITS


def test_refusals_write_nothing():
    L = _capi.lib()
    fp = C.POINTER(C.c_float)
    for what, d, cfg, code in dc.refusals():
        out = np.full(d.shape, 77, np.float32)
        with pytest.raises(CvoError, match="cvo_disparity_filter_host"):
            disparity_filter_host(d, _config(cfg), out=out)
        c = _config(cfg).c_struct()
        assert L.cvo_disparity_filter_host(d.shape[0], d.shape[1], d.ctypes.data_as(fp), C.byref(c), out.ctypes.data_as(fp)) == getattr(_capi, "CVO_E_" + code), what
        assert np.all(out == 77), what
    d, out, c = np.ones((4, 4), np.float32), np.full((4, 4), 77, np.float32), DFilterConfig().c_struct()
    ptr = lambda a: a.ctypes.data_as(fp)  # noqa: E731
    for rows, cols, src, cfg, dst, code in ((4, 4, None, C.byref(c), ptr(out), "INVALID"), (4, 4, ptr(d), None, ptr(out), "INVALID"), (4, 4, ptr(d), C.byref(c), None, "INVALID"),
                                            (0, 4, ptr(d), C.byref(c), ptr(out), "INVALID"), (4, 0, ptr(d), C.byref(c), ptr(out), "INVALID"),
                                            (4097, 4096, ptr(d), C.byref(c), ptr(out), "UNSUPPORTED")):
        assert L.cvo_disparity_filter_host(rows, cols, src, cfg, dst) == getattr(_capi, "CVO_E_" + code), (rows, cols, code)
    assert np.all(out == 77)
    assert L.cvo_disparity_filter_host(4, 4, ptr(d), C.byref(c), ptr(out)) == 0  # and a good call


def test_defaults_are_libelas_robotics_setting():
    c = _capi.cvo_dfilter_config_t()
    _capi.lib().cvo_dfilter_config_default(C.byref(c))
    assert (c.speckle_sim_threshold, c.speckle_size, c.ipol_gap_width, c.adaptive_mean) == (1.0, 200, 3, 1)
    d = DFilterConfig()
    assert (d.speckle_sim_threshold, d.speckle_size, d.ipol_gap_width, d.adaptive_mean) == (1.0, 200, 3, 1)


def test_no_op_settings():
    d = dc.blobs(30, 90, 9)
    assert not dc.first_difference(disparity_filter_host(d, DFilterConfig(1.0, 0, 0, 0)), d)
    assert not dc.first_difference(disparity_filter_host(d, DFilterConfig(1.0, 1, 0, 0)), d)  # (negative values other than -10 stay too)
    only_gap, only_mean = disparity_filter_host(d, DFilterConfig(1.0, 0, 3, 0)), disparity_filter_host(d, DFilterConfig(1.0, 1, 0, 1))
    assert not dc.first_difference(only_gap, np_dfilter.gap(d, 3)[0]) and dc.first_difference(only_gap, d)
    assert not dc.first_difference(only_mean, np_dfilter.mean(d)[0]) and dc.first_difference(only_mean, d)
    assert (only_mean[d == -3] == -3).all()  # the mean writes no negative result: such a pixel keeps the INPUT's value


def test_out_may_be_the_input():
    for name in ("golden", "blobs"):
        d = CASES[name][0].copy()
        assert disparity_filter_host(d, _config(CASES[name][1]), out=d) is d
        assert not dc.first_difference(d, dc.statement(name)["out"])


def test_speckle_never_validates_and_gap_never_changes_a_valid_pixel():
    for name in ("golden", "blobs", "blobs sim 0", "1x70", "70x1", "speckle straddle"):
        d, cfg = CASES[name]
        st = dc.statement(name)
        assert not ((st["speckle"] >= 0) & (d < 0)).any(), name
        kept = st["speckle"] >= 0
        assert np.array_equal(st["speckle"][kept], d[kept]) and (st["speckle"][~kept] == -10).all(), name
        assert np.array_equal(st["gap"][kept], st["speckle"][kept]), name
        twin_speckle = disparity_filter_host(d, DFilterConfig(cfg.speckle_sim_threshold, cfg.speckle_size, 0, 0))
        assert not dc.first_difference(twin_speckle, st["speckle"]), name
        twin_gap = disparity_filter_host(twin_speckle, DFilterConfig(cfg.speckle_sim_threshold, 0, cfg.ipol_gap_width, 0))
        assert not dc.first_difference(twin_gap, st["gap"]), name


def quality(rows, cols, seed, D=64):
    """-> ((valid, outlier share) before, after) the default filter of the matcher twin's map of a two_planes pair"""
    left, right, truth = sc.two_planes(rows, cols, seed)
    raw = stereo_disparity_host(left, right, SGMConfig(max_disparity=D))
    out = np_dfilter.dfilter(raw)
    assert not dc.first_difference(disparity_filter_host(raw), out)
    figures = []
    for m in (raw, out):
        valid = m >= 0
        figures.append((int(valid.sum()), float((np.abs(m[valid] - truth[valid]) > 1).mean())))
    return figures


@pytest.mark.parametrize("rows,cols,seed", ((64, 200, 3), (96, 320, 0), (120, 160, 5)))
def test_the_filter_does_not_raise_the_outlier_share(rows, cols, seed):
    before, after = quality(rows, cols, seed)
    print(f"{rows} x {cols} seed {seed}: {before[0]} valid, {100 * before[1]:.2f} % -> {after[0]} valid, {100 * after[1]:.2f} %")
    assert after[1] <= before[1], (before, after)
