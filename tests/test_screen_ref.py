"""CPU tests of the screening contract (include/tsf.h, "outlier screening"): the numpy restatement (tests/screen_ref.py,
what tests/test_gpu_screen.py holds the kernels to bit for bit) on cases worked by hand; what fc.screen_rows refuses
before the library is touched; the modeler's `model.screen` section."""
import numpy as np
import pytest

from tests import screen_ref as sr
from time_series_spark_amd import _lib, forecaster as fc
from time_series_spark_amd.jobs import prophet_modeler as pm


def _one(r, **kw):
    """the rule on residuals given directly: y = r, fitted = 0"""
    r = np.asarray(r, dtype=np.float64)
    return sr.screen_series(r, np.zeros(len(r)), **kw)


def test_constants_are_the_headers():
    assert (sr.OK, sr.TOO_FEW, sr.TOO_LONG, sr.NONFINITE) == (_lib.SCREEN_OK, _lib.SCREEN_TOO_FEW, _lib.SCREEN_TOO_LONG,
                                                              _lib.SCREEN_NONFINITE)
    assert sr.MAX_ROWS == _lib.SCREEN_MAX_ROWS


def test_m_odd_by_hand():
    # a = [0 1 2 3 100]: center = a[2] = 2; d = [2 1 0 1 98], b = [0 1 1 2 98]: mad = b[2] = 1, scale = 1.4826
    # B = floor(0.4 * 5) = 2; cut = max(5 * 1.4826, b[5 - 1 - 2] = 1) = 7.413: only the 98 is beyond
    o = _one([3, 100, 0, 2, 1], threshold=5.0, max_share=0.4, min_rows=2)
    assert o['status'] == sr.OK and o['center'] == 2.0 and o['scale'] == 1.4826 * 1.0
    assert list(o['flag']) == [0, 1, 0, 0, 0] and (o['n_new'], o['n_flagged']) == (1, 1)
    assert list(o['resid']) == [3, 100, 0, 2, 1]


def test_m_even_by_hand():
    # a = [0 1 2 3 4 50]: center = (2 + 3) / 2; d = [2.5 1.5 .5 .5 1.5 47.5], b = [.5 .5 1.5 1.5 2.5 47.5]: mad = 1.5
    # B = floor(0.5 * 6) = 3; cut = max(5 * 1.4826 * 1.5, b[2] = 1.5)
    o = _one([0, 1, 2, 3, 4, 50], threshold=5.0, max_share=0.5, min_rows=2)
    assert o['center'] == 2.5 and o['scale'] == 1.4826 * 1.5
    assert list(o['flag']) == [0, 0, 0, 0, 0, 1] and o['n_new'] == 1
    # the same rows with one excluded: m = 5 is odd, the excluded row keeps its flag and its residual, and uses the budget
    o = _one([0, 1, 2, 3, 4, 50], excluded=[1, 0, 0, 0, 0, 0], threshold=5.0, max_share=0.5, min_rows=2)
    assert o['center'] == 3.0                       # a = [1 2 3 4 50]
    assert list(o['flag']) == [1, 0, 0, 0, 0, 1] and (o['n_new'], o['n_flagged']) == (1, 2)


def test_zero_mad_with_and_without_a_scale_floor():
    r = [0.0] * 9 + [1.0]
    # mad = 0: scale = 0, B = floor(0.1 * 10) = 1, cut = max(0, b[8] = 0) = 0: the one row off the median is flagged
    o = _one(r, threshold=5.0, max_share=0.1, min_rows=2)
    assert o['scale'] == 0.0 and list(o['flag']) == [0] * 9 + [1]
    # with a floor under the scale the cut is 5 * 1 and nothing is beyond it
    o = _one(r, min_scale=1.0, threshold=5.0, max_share=0.1, min_rows=2)
    assert o['scale'] == 1.0 and o['n_new'] == 0 and not o['flag'].any()


def test_ties_at_the_budget_boundary_flag_nothing():
    # m0 = 20, max_share = 0.1: B = 2, but three rows tie at the largest deviation: b[20 - 1 - 2] = 100 is the cut and
    # the comparison is strict
    r = np.array([1.0, -1.0] * 8 + [0.0] + [100.0] * 3)
    o = _one(r, threshold=5.0, max_share=0.1, min_rows=10)
    assert o['status'] == sr.OK and o['n_new'] == 0 and not o['flag'].any()
    # two tied rows fit the budget
    r[17] = 0.5
    o = _one(r, threshold=5.0, max_share=0.1, min_rows=10)
    assert o['n_new'] == 2 and list(np.flatnonzero(o['flag'])) == [18, 19]
    # at most B rows whatever the data: 4 spikes, budget 2, all different -> the two largest
    r = np.concatenate([np.tile([1.0, -1.0], 8), 100.0 + np.arange(4)])
    o = _one(r, threshold=5.0, max_share=0.1, min_rows=10)
    assert list(np.flatnonzero(o['flag'])) == [18, 19]


def test_no_budget_left_after_earlier_exclusions():
    r = np.array([1.0, -1.0] * 9 + [500.0, 1000.0])
    ex = np.zeros(20, np.uint8)
    ex[[0, 1]] = 1                                  # B = floor(0.1 * 20) - 2 = 0
    o = _one(r, excluded=ex, threshold=5.0, max_share=0.1, min_rows=10)
    assert o['status'] == sr.OK and o['n_new'] == 0 and o['n_flagged'] == 2 and list(o['flag']) == list(ex)
    assert np.isfinite(o['center']) and np.isfinite(o['scale'])
    ex[1] = 0                                       # B = 1: the largest one
    o = _one(r, excluded=ex, threshold=5.0, max_share=0.1, min_rows=10)
    assert list(np.flatnonzero(o['flag'])) == [0, 19] and (o['n_new'], o['n_flagged']) == (1, 2)
    o = _one(r, threshold=5.0, max_share=0.0, min_rows=10)         # no budget at all
    assert o['n_new'] == 0


def test_each_status():
    r = np.arange(12.0)
    ex = np.zeros(12, np.uint8)
    ex[:3] = 1
    o = _one(r, excluded=ex, min_rows=10)           # m = 9 < 10
    assert o['status'] == sr.TOO_FEW and list(o['flag']) == list(ex) and np.isnan(o['center']) and np.isnan(o['scale'])
    assert (o['n_new'], o['n_flagged']) == (0, 3)
    assert _one(r, excluded=ex, min_rows=9)['status'] == sr.OK
    o = _one(np.zeros(sr.MAX_ROWS + 1), min_rows=2)
    assert o['status'] == sr.TOO_LONG and not o['flag'].any() and np.isnan(o['center'])
    assert _one(np.zeros(sr.MAX_ROWS), min_rows=2)['status'] == sr.OK
    # a NaN in fitted on a live row flags nothing; on an excluded row it is not looked at
    fitted = np.zeros(12)
    fitted[5] = np.nan
    o = sr.screen_series(r, fitted, min_rows=2)
    assert o['status'] == sr.NONFINITE and not o['flag'].any() and np.isnan(o['resid'][5])
    ex = np.zeros(12, np.uint8)
    ex[5] = 1
    assert sr.screen_series(r, fitted, ex, min_rows=2)['status'] == sr.OK
    y = r.copy()
    y[0] = np.inf
    assert sr.screen_series(y, np.zeros(12), min_rows=2)['status'] == sr.NONFINITE
    assert _one([], min_rows=2)['status'] == sr.TOO_FEW


def test_panel_layouts_and_dtypes_agree():
    rng = np.random.default_rng(4)
    y = np.round(rng.normal(0, 30, (3, 40))).astype(np.int32)
    y[1, 7] = 4000
    fitted = rng.normal(0, 1, (3, 40))
    kw = dict(threshold=5.0, max_share=0.1, min_rows=10)
    a = sr.screen(y, fitted, **kw)
    b = sr.screen(y.reshape(-1), fitted.reshape(-1), offsets=np.array([0, 40, 80, 120]), **kw)
    for k in a:
        assert sr.same(a[k].reshape(-1), b[k].reshape(-1)), k
    assert a['flag'][1, 7] == 1 and a['n_flagged'].dtype == np.int32 and a['flag'].dtype == np.uint8
    c = sr.screen(y.astype(np.float32), fitted, **kw)          # integers below 2^24: the same doubles
    assert all(sr.same(a[k], c[k]) for k in a)
    off, ds, yc, ex = sr.cut_panel(np.arange(40), y, a['flag'])
    assert list(np.diff(off)) == [40 - int(n) for n in a['n_flagged']] and len(ds) == len(yc) == off[-1] and ex is None
    assert 4000 not in yc


# ---- fc.screen_rows: what is refused before the library is touched -----------------------------------------------

def test_argument_errors_before_the_library(monkeypatch):
    def never(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', never)
    monkeypatch.setattr(fc, 'get_context', never)
    y, f = np.zeros((3, 12)), np.zeros((3, 12))
    off = np.array([0, 12, 36])
    for args, kw in (((y, np.zeros((3, 11))), {}),
                     ((y, f), dict(excluded=np.zeros((2, 12)))),
                     ((y.reshape(-1), f.reshape(-1)), {}),                                   # 1-D without offsets
                     ((y, f), dict(offsets=off)),                                            # 2-D with offsets
                     ((y.reshape(-1), f.reshape(-1)), dict(offsets=np.array([0, 12, 35]))),
                     ((y, f), dict(min_scale=np.zeros(2))),
                     ((y, f), dict(threshold=0.0)), ((y, f), dict(threshold=np.inf)), ((y, f), dict(threshold=np.nan)),
                     ((y, f), dict(max_share=0.6)), ((y, f), dict(max_share=-0.1)), ((y, f), dict(min_rows=1))):
        with pytest.raises(ValueError):
            fc.screen_rows(*args, **kw)
    with pytest.raises(TypeError):
        fc.screen_rows(y.astype(np.int64), f)
    with pytest.raises(AssertionError, match='touched'):
        fc.screen_rows(y, f)                        # a good call gets as far as the library


# ---- the modeler's model.screen section ----------------------------------------------------------------------------

def test_modeler_screen_section():
    assert pm.screen_settings({'model': {'floor': 0}}) is None
    assert pm.screen_settings({}) is None
    assert pm.screen_settings({'model': {'screen': {}}}) == dict(threshold=5.0, max_share=0.05, min_rows=10, passes=1)
    got = pm.screen_settings({'model': {'screen': {'threshold': 4, 'max_share': 0.1, 'min_rows': 20, 'passes': 2}}})
    assert got == dict(threshold=4.0, max_share=0.1, min_rows=20, passes=2)
    for bad in ({'thresh': 5}, {'threshold': 0}, {'max_share': 0.51}, {'min_rows': 1}, {'passes': 0}, {'passes': 9},
                {'passes': 1.5}, [5.0]):
        with pytest.raises(ValueError):
            pm.screen_settings({'model': {'screen': bad}})
    assert pm.SCREENED_COLUMNS == ['series_id', 'dim_id', 'ds', 'y', 'resid', 'center', 'scale']
