"""Batched scores (cvo_inner_product_batch / cvo_function_angle_batch): the boundary, without a GPU."""
import ctypes as C

import numpy as np

from unified_cvo_amd import _capi


def test_batch_symbols_are_exported_and_bound():
    for name in ("cvo_inner_product_batch", "cvo_function_angle_batch", "cvo_debug_last_score_batch"):
        assert name in _capi.EXPORTED
        assert getattr(_capi.lib(), name).argtypes  # (a ctypes signature is declared)


def test_null_context_or_arrays_are_invalid():
    L = _capi.lib()
    p = _capi.cvo_params_t()
    L.cvo_params_default(C.byref(p))
    out = np.full(2, 7.0, np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    T = np.eye(4, dtype=np.float32).reshape(16)
    Tp = T.ctypes.data_as(C.POINTER(C.c_float))
    ell = np.full(1, 0.3, np.float32)
    ep = ell.ctypes.data_as(C.POINTER(C.c_float))
    clouds = (C.c_void_p * 1)()
    # no context
    assert L.cvo_inner_product_batch(None, C.byref(p), 1, clouds, clouds, Tp, ep, fp) == _capi.CVO_E_INVALID
    assert L.cvo_function_angle_batch(None, C.byref(p), 1, clouds, clouds, Tp, ep, 0, fp) == _capi.CVO_E_INVALID
    assert L.cvo_inner_product_batch(None, C.byref(p), 0, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_function_angle_batch(None, None, 0, None, None, None, None, 1, None) == _capi.CVO_E_INVALID
    assert L.cvo_debug_last_score_batch(None, None, None, None) == _capi.CVO_E_INVALID
    assert np.all(out == 7.0)
