"""CPU tests of the forecast quantiles' host side: the column names fc.quantile_columns gives the levels, what it
refuses, the layout of Quantiles.frame, and that the binding of tsf_predict_quantiles loads beside an unchanged tsf_spec
(no compute: no GPU here)."""
import ctypes

import numpy as np
import pytest

from time_series_spark_amd import _lib, forecaster as fc


def test_names():
    assert fc.quantile_columns([0, 0.1, 0.5, 0.975, 1]) == ['yhat_q0', 'yhat_q10', 'yhat_q50', 'yhat_q97.5', 'yhat_q100']
    assert fc.quantile_columns([0.9, 0.1], prefix='yhat_cum_q') == ['yhat_cum_q90', 'yhat_cum_q10']      # order kept
    assert fc.quantile_columns(np.array([0.25]), prefix='trend_q') == ['trend_q25']
    assert fc.quantile_columns([]) == []
    assert len(fc.quantile_columns(np.linspace(0, 1, _lib.MAX_QUANT))) == _lib.MAX_QUANT == 64


@pytest.mark.parametrize('levels', [[-0.1], [0.5, 1.5], [float('nan')], [float('inf')], [0.1, 0.5, 0.1],
                                    [0.1, 0.1 + 1e-12], list(np.linspace(0, 1, 65))])
def test_refusals(levels):
    """out of range, not finite, two levels with one name (equal, or equal to 6 digits), 65 levels"""
    with pytest.raises(ValueError):
        fc.quantile_columns(levels)


def test_frame_layout():
    N, H = 2, 4
    lv = np.array([0.1, 0.5, 0.975])
    yhat = np.arange(N * H, dtype=np.float64).reshape(N, H)
    q = np.arange(N * 3 * H, dtype=np.float64).reshape(N, 3, H)
    ds = np.datetime64('2024-01-01', 'ns') + np.arange(H) * np.timedelta64(1, 'D')
    f = fc.Quantiles(yhat, lv, q).frame(1, ds)
    assert list(f.columns) == ['ds', 'yhat', 'yhat_q10', 'yhat_q50', 'yhat_q97.5']
    assert np.array_equal(f['yhat'].values, yhat[1]) and np.array_equal(f['yhat_q50'].values, q[1, 1])
    f = fc.Quantiles(yhat, lv, q, cum_q=q + 1, trend_q=q + 2).frame(0, ds.astype(np.int64))
    assert list(f.columns) == ['ds', 'yhat', 'yhat_q10', 'yhat_q50', 'yhat_q97.5', 'yhat_cum_q10', 'yhat_cum_q50',
                               'yhat_cum_q97.5', 'trend_q10', 'trend_q50', 'trend_q97.5']
    assert np.array_equal(f['ds'].values, ds) and np.array_equal(f['yhat_cum_q97.5'].values, q[0, 2] + 1)
    assert np.array_equal(f['trend_q10'].values, q[0, 0] + 2)


def test_binding(built):
    """the library exports both entries, tsf_spec is what it was (the binding's own self-check passes on load), and
    tsf_quantile_out is six pointers"""
    L = _lib.load()
    assert L.tsf_spec_size() == ctypes.sizeof(_lib.TsfSpec) == 1584
    for sym in ('tsf_predict_quantiles', 'tsf_predict_quantiles_dev'):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    assert ctypes.sizeof(_lib.TsfQuantileOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in _lib.TsfQuantileOut._fields_] == ['yhat', 'q', 'cum_q', 'trend_q', 'samples', 'trend_samples']
