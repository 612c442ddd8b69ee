"""CPU tests of the group roll-ups' host side: fc.rollup_groups (labels -> dense group indices), the layout of
RollupQuantiles.frame, the ValueErrors that predict_rollup raises before any library is loaded, and that the binding of
the four tsf_rollup_* entries loads beside an unchanged tsf_spec (no compute: no GPU here)."""
import ctypes

import numpy as np
import pytest

from tests import forecast_cases as fcs
from time_series_spark_amd import _lib, forecaster as fc


def test_groups_of_unsorted_labels():
    uniq, g = fc.rollup_groups(np.array([751, 3, 751, 90, 3, 3], dtype=np.int32))
    assert np.array_equal(uniq, [3, 90, 751]) and np.array_equal(g, [2, 0, 2, 1, 0, 0])
    assert g.dtype == np.int64 and g.flags['C_CONTIGUOUS']
    assert np.array_equal(uniq[g], [751, 3, 751, 90, 3, 3])
    # one label: one group
    uniq, g = fc.rollup_groups(np.full(4, -7))
    assert np.array_equal(uniq, [-7]) and np.array_equal(g, [0, 0, 0, 0])


def test_groups_of_tuple_labels():
    sid = np.array([9, 8, 9, 8, 9])
    region = np.array([1, 1, 0, 1, 1])
    uniq, g = fc.rollup_groups((sid, region))
    assert np.array_equal(uniq, [[8, 1], [9, 0], [9, 1]]) and np.array_equal(g, [2, 0, 1, 0, 2])
    assert g.dtype == np.int64 and np.array_equal(uniq[g], np.stack([sid, region], axis=1))
    # a tuple of one array groups as the array does
    u1, g1 = fc.rollup_groups((sid,))
    u0, g0 = fc.rollup_groups(sid)
    assert np.array_equal(u1[:, 0], u0) and np.array_equal(g1, g0)


def test_groups_of_nothing():
    for labels in (np.zeros(0, dtype=np.int64), (np.zeros(0, dtype=np.int32),), []):
        uniq, g = fc.rollup_groups(labels)
        assert len(uniq) == 0 and g.shape == (0,) and g.dtype == np.int64


@pytest.mark.parametrize('labels', [np.zeros((2, 2), dtype=np.int64), (np.arange(3), np.arange(4)), (),
                                    np.array([0.5, 1.5]), (np.arange(2), np.array([0.5, 1.0]))])
def test_group_refusals(labels):
    """not one-dimensional, unequal lengths, an empty tuple, labels that are not integers"""
    with pytest.raises(ValueError):
        fc.rollup_groups(labels)


def test_frame_layout():
    G, H = 3, 4
    lv = np.array([0.1, 0.5, 0.975])
    yhat = np.arange(G * H, dtype=np.float64).reshape(G, H)
    q = np.arange(G * 3 * H, dtype=np.float64).reshape(G, 3, H)
    count = np.array([2, 0, 5])
    ds = np.datetime64('2024-01-01', 'ns') + np.arange(H) * np.timedelta64(1, 'D')
    r = fc.RollupQuantiles(yhat, count, lv, q)
    assert r.cum_q is None and np.array_equal(r.count, count)
    f = r.frame(2, ds)
    assert list(f.columns) == ['ds', 'yhat', 'yhat_q10', 'yhat_q50', 'yhat_q97.5']
    assert np.array_equal(f['yhat'].values, yhat[2]) and np.array_equal(f['yhat_q50'].values, q[2, 1])
    f = fc.RollupQuantiles(yhat, count, lv, q, cum_q=q + 1).frame(0, ds.astype(np.int64))
    assert list(f.columns) == ['ds', 'yhat', 'yhat_q10', 'yhat_q50', 'yhat_q97.5', 'yhat_cum_q10', 'yhat_cum_q50',
                               'yhat_cum_q97.5']
    assert np.array_equal(f['ds'].values, ds) and np.array_equal(f['yhat_cum_q97.5'].values, q[0, 2] + 1)


def test_errors_before_the_library(monkeypatch):
    """a bad level, labels / series_key / extra columns of the wrong shape and series_key=None are ValueErrors raised
    before anything is loaded: _lib.load and get_context fail the test if they are reached"""
    def reached(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', reached)
    monkeypatch.setattr(fc, 'get_context', reached)
    c = fcs.make('iv129')
    args = (c.spec, c.theta, c.y_scale, c.grid, c.fut)
    keys = np.arange(c.N, dtype=np.int64)
    labels = np.zeros(c.N, dtype=np.int64)
    ok = dict(labels=labels, quantiles=[0.1, 0.9], series_key=keys, extra_future=c.extra)
    for change, match in ((dict(quantiles=[0.5, 1.5]), 'quantile level'),
                          (dict(quantiles=[float('nan')]), 'quantile level'),
                          (dict(quantiles=[0.1, 0.1]), 'two levels'),
                          (dict(quantiles=[]), 'at least one'),
                          (dict(labels=np.zeros(c.N + 1, dtype=np.int64)), 'group must be'),
                          (dict(labels=np.zeros(0, dtype=np.int64)), 'nothing to roll up'),
                          (dict(series_key=None), 'series_key is required'),
                          (dict(series_key=keys[:1]), 'series_key must be'),
                          (dict(extra_future=None), 'extra_future is required'),
                          (dict(extra_future=c.extra[:, :5]), 'extra_future must be'),
                          (dict(extra_future=np.zeros((c.N + 1,) + c.extra.shape)), 'extra_future must be')):
        with pytest.raises(ValueError, match=match):
            fc.predict_rollup(*args, **dict(ok, **change))
    with pytest.raises(ValueError, match='one calendar'):
        fc.predict_rollup(c.spec, c.theta, c.y_scale, c.grid, np.tile(c.fut, (c.N, 1)), **ok)
    # the Rollup itself: its own arguments are checked before a context is asked for
    for kw in (dict(n_groups=0), dict(n_groups=2, uncertainty_samples=1), dict(n_groups=2, uncertainty_samples=4097)):
        with pytest.raises(ValueError):
            fc.Rollup(c.fut, **kw)
    with pytest.raises(ValueError, match='one calendar'):
        fc.Rollup(np.zeros((2, 3), dtype=np.int64), 2)


def test_binding(built):
    """the library exports the four entries, tsf_spec is what it was (the binding's self-check passes on load), and
    tsf_rollup_out is five pointers in the header's order"""
    L = _lib.load()
    assert L.tsf_spec_size() == ctypes.sizeof(_lib.TsfSpec) == 1584
    for sym in ('tsf_rollup_create', 'tsf_rollup_add', 'tsf_rollup_quantiles', 'tsf_rollup_free'):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    assert ctypes.sizeof(_lib.TsfRollupOut) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in _lib.TsfRollupOut._fields_] == ['yhat', 'count', 'q', 'cum_q', 'samples']
