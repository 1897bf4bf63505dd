"""Non-local-means denoising without a GPU: the statement (np_nlm.py) against its own literal four-loop form; cvo_nlm_weights
against the statement's table, with the check that no weight sits near a rounding tie; the CPU twin (cvo_nlm_denoise_host,
cvo_nlm_denoise_lab_host) equal to the statement; in place; every refusal by its return code, nothing written."""
import ctypes as C

import numpy as np
import pytest

import nlm_cases as nc
import np_nlm
from unified_cvo_amd import CvoError, _capi, nlm_denoise_host, nlm_denoise_lab_host, nlm_weights

WINDOWS = ((7, 21), (3, 5), (1, 1), (5, 11), (6, 20))
HS = (3, 10, 10.5, 20)


@pytest.mark.parametrize("rows,cols,channels,windows", [(1, 4, 1, (3, 5)), (3, 3, 2, (3, 5)), (3, 3, 1, (7, 21)), (1, 4, 2, (5, 11)),
                                                         (6, 6, 1, (3, 5)), (5, 6, 3, (3, 3)), (1, 1, 1, (7, 21)), (4, 1, 1, (4, 6))])
def test_the_statement_equals_its_literal_form(rows, cols, channels, windows):
    """Images of at most 6 x 6, 1 x 4 and 3 x 3 among them: the border reflects several times."""
    for kind in ("random", "steps"):
        img = nc.image(kind, rows, cols, channels)
        assert np.array_equal(np_nlm.denoise(img, 10, *windows), np_nlm.literal(img, 10, *windows)), (kind, rows, cols)


def test_the_constants_of_the_default_call():
    k = np_nlm.constants(7, 21)
    assert (k["mult"], k["shift"], k["tw"], k["sw"]) == (19096, 6, 7, 21)
    assert [np_nlm.weights(10, c)["n_nonzero"] for c in (1, 2, 3)] == [528, 1055, 1582]
    assert np_nlm.constants(8, 20)["tw"] == 9 and np_nlm.constants(6, 20) == k  # an even size grows by one


@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("h", HS)
def test_weights_equal_the_statements_table(channels, h):
    """... and no mult w lies within 1e-6 of a rounding tie, so a last-bit difference between two exp implementations
    cannot change a weight: the table is pinned by its definition, not by one libm."""
    for windows in ((7, 21), (3, 5)):
        want = np_nlm.weights(h, channels, *windows)
        assert want["tie"] > 1e-6, (h, channels, windows, want["tie"])
        got = nlm_weights(h, *windows, channels=channels)
        assert (got["mult"], got["shift"], got["n_nonzero"]) == (want["mult"], want["shift"], want["n_nonzero"])
        assert np.array_equal(got["weight"], want["weight"])


def test_weights_sizes_only_and_capacity():
    cfg = _capi.cvo_nlm_config_t(10.0, 7, 21)
    L = _capi.lib()
    nt, nz = C.c_int(), C.c_int()
    assert L.cvo_nlm_weights(C.byref(cfg), 1, None, 0, C.byref(nt), C.byref(nz), None, None) == 0
    assert (nt.value, nz.value) == (len(np_nlm.weights(10, 1)["weight"]), 528)
    buf = np.full(600, -7, np.int32)
    assert L.cvo_nlm_weights(C.byref(cfg), 1, buf.ctypes.data_as(C.POINTER(C.c_int)), 530, None, None, None, None) == 0
    assert np.array_equal(buf[:530], np_nlm.weights(10, 1)["weight"][:530]) and np.all(buf[530:] == -7)


def test_the_step_cases_are_not_passed_by_an_identity():
    """The statement changes more than half of the pixels of a noisy step image and brings it nearer its base."""
    img = nc.image("steps", 40, 70)
    out = nc.statement("steps", 40, 70)
    assert (out != img).mean() > 0.5
    for ch in (2, 3):
        assert (nc.statement("steps", 20, 30, ch) != nc.image("steps", 20, 30, ch)).mean() > 0.5


SHAPES = ((1, 1), (1, 9), (9, 1), (13, 14), (14, 27), (27, 13), (17, 59), (33, 20))


@pytest.mark.parametrize("channels", (1, 2, 3))
def test_twin_equals_the_statement(channels):
    for rows, cols in SHAPES:
        for kind in ("steps", "random"):
            got = nlm_denoise_host(nc.image(kind, rows, cols, channels))
            assert np.array_equal(got, nc.statement(kind, rows, cols, channels)), (kind, rows, cols)


@pytest.mark.parametrize("windows", WINDOWS[1:])
def test_twin_on_other_windows_and_h(windows):
    for h in HS:
        for channels in (1, 3):
            img = nc.image("steps", 14, 27, channels)
            assert np.array_equal(nlm_denoise_host(img, h, *windows), nc.statement("steps", 14, 27, channels, h, windows)), (h, channels)


def test_twin_on_the_special_planes():
    for kind in ("constant", "white", "checker"):
        img = nc.image(kind, 16, 23)
        got = nlm_denoise_host(img)
        assert np.array_equal(got, nc.statement(kind, 16, 23)) and np.array_equal(got, img), kind
    assert np.array_equal(nlm_denoise_host(nc.image("white", 9, 30, 3)), nc.image("white", 9, 30, 3))


def test_lab_equals_the_two_plane_calls():
    lab = nc.image("steps", 20, 31, 3)
    got = nlm_denoise_lab_host(lab, 10, 7)
    assert np.array_equal(got, nc.statement_lab("steps", 20, 31, 10, 7))
    assert np.array_equal(got[..., 0], nlm_denoise_host(np.ascontiguousarray(lab[..., 0]), 10))
    assert np.array_equal(got[..., 1:], nlm_denoise_host(np.ascontiguousarray(lab[..., 1:]), 7))
    assert not np.array_equal(got, nlm_denoise_host(lab, 10))  # (the 3-channel call is another computation)


def test_in_place_equals_out_of_place():
    for channels in (1, 3):
        img = nc.image("steps", 15, 22, channels)
        want = nlm_denoise_host(img)
        work = img.copy()
        assert nlm_denoise_host(work, out=work) is work and np.array_equal(work, want)
    lab = nc.image("random", 9, 12, 3)
    work = lab.copy()
    nlm_denoise_lab_host(work, out=work)
    assert np.array_equal(work, nlm_denoise_lab_host(lab))


def test_refusals_write_nothing():
    L = _capi.lib()
    bp = C.POINTER(C.c_ubyte)
    src = np.full(75, 9, np.uint8)
    for what, rows, cols, ch, h, tw, sw, hc, code in nc.refusals():
        want = getattr(_capi, "CVO_E_" + code)
        cfg = _capi.cvo_nlm_config_t(h, tw, sw)
        dst = np.full(75, 77, np.uint8)
        lab_only = what.startswith("h_color")
        if not lab_only:
            assert L.cvo_nlm_denoise_host(rows, cols, ch, src.ctypes.data_as(bp), C.byref(cfg), dst.ctypes.data_as(bp)) == want, what
        if ch == 3 or not what.startswith("channels"):
            assert L.cvo_nlm_denoise_lab_host(rows, cols, src.ctypes.data_as(bp), C.byref(cfg), hc, dst.ctypes.data_as(bp)) == want, what
        assert np.all(dst == 77), what
        if what.split()[0] in ("h", "template", "search", "th", "sh"):
            assert L.cvo_nlm_weights(C.byref(cfg), 1, None, 0, None, None, None, None) == want, what
    cfg = _capi.cvo_nlm_config_t(10.0, 7, 21)
    dst = np.full(75, 77, np.uint8)
    assert L.cvo_nlm_denoise_host(5, 5, 1, None, C.byref(cfg), dst.ctypes.data_as(bp)) == _capi.CVO_E_INVALID
    assert L.cvo_nlm_denoise_host(5, 5, 1, src.ctypes.data_as(bp), None, dst.ctypes.data_as(bp)) == _capi.CVO_E_INVALID
    assert L.cvo_nlm_denoise_host(5, 5, 1, src.ctypes.data_as(bp), C.byref(cfg), None) == _capi.CVO_E_INVALID
    assert L.cvo_nlm_denoise_lab_host(5, 5, None, C.byref(cfg), 10.0, dst.ctypes.data_as(bp)) == _capi.CVO_E_INVALID
    assert L.cvo_nlm_weights(C.byref(cfg), 0, None, 0, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_nlm_weights(None, 1, None, 0, None, None, None, None) == _capi.CVO_E_INVALID
    assert np.all(dst == 77)
    with pytest.raises(CvoError):
        nlm_denoise_host(np.zeros((5, 5), np.uint8), h=0)
    d = _capi.cvo_nlm_config_t()
    L.cvo_nlm_config_default(C.byref(d))
    assert (d.h, d.template_window, d.search_window) == (10.0, 7, 21)
