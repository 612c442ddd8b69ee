"""CPU tests of temporal reconciliation's host side (include/tsf.h "temporal reconciliation"): tsf_temporal_shares
against hand-computed cases and the numpy restatement of tests/temporal_ref.py bit for bit, its refusals, the Python
helpers on top of it (period_history, temporal_shares), the argument checks of predict_temporal that come before the
library is touched, and the restatement itself against the laws of the method on synthetic normal draws."""
import ctypes

import numpy as np
import pytest

from tests import temporal_ref as tr

DAY = 86400 * 10 ** 9


@pytest.fixture(scope='module')
def lib(built):
    from time_series_spark_amd import _lib, forecaster as fc
    return _lib.load(), fc, _lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _call(L, N, H, w0, w1, w, v):
    w0, w1 = np.ascontiguousarray(w0, dtype=np.int32), np.ascontiguousarray(w1, dtype=np.int32)
    v = np.ascontiguousarray(v, dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    share, share_total = np.full((N, H), -7.0), np.full((N, len(w0)), -7.0)
    rc = L.tsf_temporal_shares(N, H, len(w0), w0.ctypes.data, w1.ctypes.data, None if w is None else w.ctypes.data,
                               v.ctypes.data, share.ctypes.data, share_total.ctypes.data)
    return rc, share, share_total


# 10 rows; windows out of order: [6, 10), [0, 1) (one row), [2, 6); row 1 is in no window
W0, W1 = [6, 0, 2], [10, 1, 6]


def test_exports(lib):
    L, fc, _lib = lib
    for sym in ('tsf_temporal_shares', 'tsf_temporal_out_size', 'tsf_predict_temporal'):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.tsf_temporal_out_size() == ctypes.sizeof(_lib.TsfTemporalOut) == 56


def test_shares_by_hand(lib):
    L, fc, _lib = lib
    # all weights 1: v = 4, 0.5, 4 -> 1 / (4 + 4), 1 / (0.5 + 1), 1 / (4 + 4)
    rc, share, mu = _call(L, 1, 10, W0, W1, None, [[4.0, 0.5, 4.0]])
    assert rc == 0
    assert _bits(share, [[1 / 1.5, 0.0, .125, .125, .125, .125, .125, .125, .125, .125]])
    assert _bits(mu, [[4 / 8.0, 1 / 1.5, 4 / 8.0]])
    # given weights, two series, the second with a NaN v in window 0
    w = np.array([[1, 9, 2, 2, 4, 8, .5, .5, 1, 2], [3, 3, 3, 3, 3, 3, 1, 1, 1, 1]], dtype=np.float64)
    v = np.array([[4.0, 1.0, 16.0], [np.nan, 3.0, 12.0]])
    rc, share, mu = _call(L, 2, 10, W0, W1, w, v)
    assert rc == 0
    assert _bits(share[0], [1 / 2.0, 0.0, 2 / 32.0, 2 / 32.0, 4 / 32.0, 8 / 32.0, .5 / 8, .5 / 8, 1 / 8.0, 2 / 8.0])
    assert _bits(mu[0], [4 / 8.0, 1 / 2.0, 16 / 32.0])
    assert _bits(share[1], [3 / 6.0, 0.0, 3 / 24.0, 3 / 24.0, 3 / 24.0, 3 / 24.0, 0.0, 0.0, 0.0, 0.0])
    assert np.isnan(mu[1, 0]) and _bits(mu[1, 1:], [3 / 6.0, 12 / 24.0])


@pytest.mark.parametrize('weights', ['given', 'null'])
def test_shares_are_the_restatement(lib, weights):
    L, fc, _lib = lib
    rng = np.random.default_rng(5)
    N, H = 4, 17
    w0, w1 = [12, 0, 5], [17, 5, 12]
    w = None if weights == 'null' else rng.uniform(1e-3, 30.0, (N, H))
    v = rng.uniform(0.1, 50.0, (N, 3))
    v[1, 2] = v[3, 0] = np.nan
    rc, share, mu = _call(L, N, H, w0, w1, w, v)
    assert rc == 0
    want = tr.shares(N, H, w0, w1, w, v)
    assert _bits(share, want[0]) and _bits(mu, want[1])
    assert np.array_equal(np.isnan(mu), np.isnan(v)) and _bits(share[1, 5:12], np.zeros(7)) and _bits(share[3, 12:], np.zeros(5))
    ok = ~np.isnan(mu)
    assert (mu[ok] > 0).all() and (mu[ok] < 1).all() and (share >= 0).all() and (share < 1).all()
    # the shares of a window sum to its share_total up to the rounding of m divides and m - 1 adds
    for n in range(N):
        for k in range(3):
            if ok[n, k]:
                tot = 0.0
                for h in range(w0[k], w1[k]):
                    tot = tot + share[n, h]
                assert abs(tot - mu[n, k]) <= 2 * (w1[k] - w0[k]) * np.spacing(mu[n, k])


def test_refusals(lib):
    L, fc, _lib = lib
    w, v = np.ones((2, 10)), np.array([[4.0, 1.0, 4.0], [4.0, np.nan, 4.0]])

    def bad(a, i, x):
        a = a.copy()
        a[i] = x
        return a

    assert _call(L, 2, 10, W0, W1, w, v)[0] == 0
    for x in (0.0, -1.0, np.inf, np.nan):
        assert _call(L, 2, 10, W0, W1, bad(w, (1, 3), x), v)[0] == -1, x
        assert _call(L, 2, 10, W0, W1, bad(w, (0, 1), x), v)[0] == -1, x      # (a row in no window: still a bad weight)
    for x in (0.0, -2.0, np.inf, -np.inf):
        assert _call(L, 2, 10, W0, W1, w, bad(v, (0, 2), x))[0] == -1, x
    # windows: out of range, empty, reversed, two that share a row
    for w0, w1 in (([6, 0, 2], [11, 1, 6]), ([6, -1, 2], [10, 1, 6]), ([6, 1, 2], [10, 1, 6]), ([6, 0, 2], [10, 1, 7]),
                   ([6, 0, 0], [10, 1, 6])):
        assert _call(L, 2, 10, w0, w1, w, v)[0] == -1, (w0, w1)
    z = np.zeros(1, dtype=np.int32)
    assert L.tsf_temporal_shares(2, 10, 0, z.ctypes.data, z.ctypes.data, None, v.ctypes.data, w.ctypes.data, v.ctypes.data) == -1
    assert L.tsf_temporal_shares(2, 10, 3, None, None, None, v.ctypes.data, w.ctypes.data, v.ctypes.data) == -1


def _calendar():
    """a daily calendar from Wednesday 2024-01-03 over 40 days with 2024-01-17 (a Wednesday) missing: a partial first
    week of 5 rows, a full one, a week of 6 rows, then three full ones (the calendar ends on Sunday 2024-02-11)"""
    start = np.datetime64('2024-01-03', 'ns').astype(np.int64)
    ds = start + DAY * np.arange(40, dtype=np.int64)
    return ds[ds != np.datetime64('2024-01-17', 'ns').astype(np.int64)]


def test_period_history(lib):
    L, fc, _lib = lib
    ds = _calendar()
    assert len(ds) == 39
    y = np.random.default_rng(2).uniform(1, 9, (3, 39))
    w = fc.period_windows(ds, 'W')
    assert list(w.n_rows) == [5, 7, 6, 7, 7, 7]
    ds_p, y_p, kept = fc.period_history(ds, y, 'W')
    assert list(kept.start) == [5, 18, 25, 32] and list(kept.n_rows) == [7] * 4
    assert np.array_equal(ds_p, ds[[5, 18, 25, 32]]) and np.array_equal(ds_p, kept.label_ns)
    assert [str(d)[:10] for d in ds_p.view('datetime64[ns]')] == ['2024-01-08', '2024-01-22', '2024-01-29', '2024-02-05']
    assert y_p.shape == (3, 4) and _bits(y_p, fc.window_totals(y, kept))
    want = y[:, 5].copy()
    for h in range(6, 12):
        want = want + y[:, h]
    assert _bits(y_p[:, 0], want)
    # full_rows given: the 6-row week alone; a NaN row makes its period's total NaN; no period with that many rows
    ds6, y6, k6 = fc.period_history(ds, y, 'W', full_rows=6)
    assert list(k6.start) == [12] and y6.shape == (3, 1)
    y2 = y.copy()
    y2[1, 20] = np.nan
    assert np.isnan(fc.period_history(ds, y2, 'W')[1][1, 1]) and np.isfinite(fc.period_history(ds, y2, 'W')[1][[0, 2]]).all()
    for a in ((ds, y, 'W', 3), (ds, y[:, :-1], 'W'), (ds, y[0], 'W'), (ds, y, 'fortnight')):
        with pytest.raises(ValueError):
            fc.period_history(*a)
    # months: January (28 rows here) and February (11), one period each: the default keeps the larger of a tie
    assert list(fc.period_history(ds, y, 'M')[2].n_rows) == [28]


def test_python_policies(lib):
    L, fc, _lib = lib
    ds = np.datetime64('2024-01-03', 'ns').astype(np.int64) + DAY * np.arange(24, dtype=np.int64)
    w = fc.period_windows(ds, 'W')                      # 5, 7, 7, 5 rows
    assert list(w.n_rows) == [5, 7, 7, 5]
    s = fc.temporal_shares(w, 2, 24)
    assert s.windows is w and s.share.shape == (2, 24) and s.share_total.shape == (2, 4)
    assert np.isnan(s.share_total[:, [0, 3]]).all() and _bits(s.share_total[:, 1:3], np.full((2, 2), 0.5))
    assert _bits(s.share[:, 5:19], np.full((2, 14), 1 / 14.0)) and _bits(s.share[:, :5], np.zeros((2, 5)))
    s = fc.temporal_shares(w, 2, 24, period_weight='ols', active=np.ones(4, dtype=bool))
    assert _bits(s.share_total, np.tile([5 / 6.0, 7 / 8.0, 7 / 8.0, 5 / 6.0], (2, 1)))
    rng = np.random.default_rng(8)
    wt, v = rng.uniform(0.5, 2.0, 24), rng.uniform(1.0, 9.0, (2, 4))
    act = np.array([[1, 1, 0, 1], [0, 1, 1, 1]], dtype=bool)
    s = fc.temporal_shares(w, 2, 24, weight=wt, period_weight=v, active=act)
    want = tr.shares(2, 24, w.start, w.end, np.tile(wt, (2, 1)), np.where(act, v, np.nan))
    assert _bits(s.share, want[0]) and _bits(s.share_total, want[1])
    rows = fc.row_windows(24, 7, step=3)                # rolling windows overlap
    for kw in (dict(weight=wt[:-1]), dict(weight=-wt), dict(period_weight='mint'), dict(period_weight=v[:, :3]),
               dict(period_weight=-v), dict(active=np.ones(3, dtype=bool)), dict(active=np.ones(4)), dict(windows=rows),
               dict(windows=(w.start, w.end)), dict(H=20), dict(N=-1)):
        a = dict(dict(windows=w, N=2, H=24), **kw)
        with pytest.raises(ValueError):
            fc.temporal_shares(a.pop('windows'), a.pop('N'), a.pop('H'), **a)
    s = fc.temporal_shares(w, 0, 24)
    assert s.share.shape == (0, 24) and s.share_total.shape == (0, 4)


def test_predict_temporal_checks_come_before_the_library(lib, monkeypatch):
    """every argument-shape error of predict_temporal is a ValueError raised with the library out of reach"""
    L, fc, _lib = lib
    spec = fc.ModelSpec(growth='linear', n_changepoints=2, seasonalities=[{'name': 'w', 'period': 7, 'fourier_order': 1}])
    pspec = fc.ModelSpec(growth='linear', n_changepoints=1, seasonalities=[])
    N, H = 2, 24
    ds = np.datetime64('2024-01-03', 'ns').astype(np.int64) + DAY * np.arange(H, dtype=np.int64)
    w = fc.period_windows(ds, 'W')
    shares = fc.temporal_shares(w, N, H)
    grid = np.zeros(1, dtype=_lib.GRID_DTYPE)
    good = dict(spec=spec, theta=np.zeros((N, spec.theta_stride)), y_scale=np.ones(N), grid=grid, ds_future_ns=ds, windows=w,
                period_spec=pspec, period_theta=np.zeros((N, pspec.theta_stride)), period_y_scale=np.ones(N),
                period_grid=grid, ds_period_ns=w.label_ns, shares=shares, quantiles=[0.1, 0.9],
                series_key=np.arange(N), period_key=100 + np.arange(N))

    def unreachable():
        raise AssertionError('the library was loaded')

    monkeypatch.setattr(_lib, 'load', unreachable)
    monkeypatch.setattr(fc, 'get_context', unreachable)
    bad_shares = fc.TemporalShares(w, shares.share[:, :-1], shares.share_total)
    for kw in (dict(theta=np.zeros((N, 3))), dict(period_theta=np.zeros((N + 1, pspec.theta_stride))),
               dict(period_y_scale=np.ones(N + 1)), dict(ds_period_ns=w.label_ns[:-1]), dict(series_key=None),
               dict(period_key=None), dict(period_key=np.arange(N + 1)), dict(shares=(shares.share, shares.share_total)),
               dict(shares=bad_shares), dict(quantiles=[]), dict(quantiles=[0.5, 1.5]), dict(windows=fc.row_windows(H, 7, step=3)),
               dict(windows=fc.row_windows(H + 4, 7)), dict(uncertainty_samples=1), dict(uncertainty_samples=5000),
               dict(noise_ar=np.array([0.5, 1.0])), dict(noise_ar=np.array([-0.2, 0.1])), dict(period_noise_ar=np.zeros(3)),
               dict(cap=np.ones(N + 1)), dict(period_floor=np.ones(N + 1))):
        with pytest.raises(ValueError):
            fc.predict_temporal(**dict(good, **kw))


# ---- the restatement alone satisfies the laws of the method -----------------------------------------------------------

S = 20000
ROWS = (1, 4, 7)


@pytest.fixture(scope='module')
def synthetic():
    """one series, 13 rows, windows of 1, 4 and 7 rows (row 5 in none): x_h ~ N(m_h, w_h), t_k ~ N(sum m_h + bias, v_k),
    independent, S = 20 000 draws; weights equal to the true variances"""
    rng = np.random.default_rng(2025)
    H = 13
    w0, w1 = np.array([0, 1, 6]), np.array([1, 5, 13])
    m, w = rng.uniform(20.0, 200.0, H), rng.uniform(0.5, 25.0, H)
    v, bias = np.array([3.0, 10.0, 60.0]), np.array([4.0, -15.0, 30.0])
    x = (m[:, None] + np.sqrt(w)[:, None] * rng.standard_normal((H, S)))[None]
    tm = np.array([m[a:b].sum() for a, b in zip(w0, w1)]) + bias
    t = (tm[:, None] + np.sqrt(v)[:, None] * rng.standard_normal((3, S)))[None]
    share, share_total = tr.shares(1, H, w0, w1, w[None], v[None])
    xr, win = tr.reconcile(x, t, w0, w1, share, share_total)
    return dict(w0=w0, w1=w1, w=w, v=v, x=x, t=t, share=share, share_total=share_total, xr=xr, win=win)


def test_reconciled_rows_sum_to_the_reconciled_total(synthetic):
    """within tr.coherence_bound, which is derived there from the operation count (not fitted)"""
    s = synthetic
    sums = tr.window_sums(s['x'], s['w0'], s['w1'])
    for k, (a, b) in enumerate(zip(s['w0'], s['w1'])):
        tot = s['xr'][0, a].copy()
        for h in range(a + 1, b):
            tot = tot + s['xr'][0, h]
        d = s['t'][0, k] - sums[0, k]
        bound = tr.coherence_bound(b - a, np.abs(s['x'][0, a:b]).sum(axis=0), np.abs(d))
        err = np.abs(tot - s['win'][0, k])
        print('window of %d rows: max |sum of rows - total| / bound = %.3f' % (b - a, (err / bound).max()))
        assert (err <= bound).all()
        # the incoherent pair it started from is far apart: the bound is not vacuous
        assert np.abs(d).mean() > 1e10 * bound.max()
    assert _bits(s['xr'][0, 5], s['x'][0, 5])                      # the row in no window


def test_reconciled_variances(synthetic):
    """With weights equal to the true variances and independent draws, total' = sum + mu (t - sum) has variance
    (1 - mu)^2 W + mu^2 v = v W / (v + W) and row' = x_h + lam_h (t - sum) has w_h - w_h^2 / (v + W).  Both are linear in
    the normal draws, so each is normal, and the sample variance of S normal draws has the standard error
    sqrt(2 / (S - 1)) times the variance: sqrt(2 / S) at S = 20 000 to three digits.  The tolerance is six of them,
    6 sqrt(2 / S) = 6 %, relative: a correct rule fails this with probability below 1e-8 per comparison (13 here)."""
    s = synthetic
    tol = 6 * np.sqrt(2.0 / S)
    for k, (a, b) in enumerate(zip(s['w0'], s['w1'])):
        W, v = s['w'][a:b].sum(), s['v'][k]
        want = v * W / (v + W)
        got = s['win'][0, k].var(ddof=1)
        assert abs(got - want) <= tol * want, (k, got, want)
        for h in range(a, b):
            want = s['w'][h] - s['w'][h] ** 2 / (v + W)
            got = s['xr'][0, h].var(ddof=1)
            assert want < s['w'][h] and abs(got - want) <= tol * want, (h, got, want)


def test_inactive_windows_and_zero_shares_are_neutral(synthetic):
    s = synthetic
    mu = s['share_total'].copy()
    mu[0, 1] = np.nan
    xr, win = tr.reconcile(s['x'], s['t'], s['w0'], s['w1'], s['share'], mu)
    sums = tr.window_sums(s['x'], s['w0'], s['w1'])
    assert _bits(xr[0, 1:5], s['x'][0, 1:5]) and _bits(win[0, 1], sums[0, 1])       # (even with nonzero shares on its rows)
    assert _bits(xr[0, 6:], s['xr'][0, 6:]) and _bits(win[0, 2], s['win'][0, 2]) and not _bits(xr[0, 0], s['x'][0, 0])
    xr, win = tr.reconcile(s['x'], s['t'], s['w0'], s['w1'], np.zeros((1, 13)), np.zeros((1, 3)))
    assert _bits(xr, s['x']) and _bits(win, sums)
    y, yp = s['x'][:, :, 0], s['t'][:, :, 0]
    r = tr.contract(s['x'][:, :, :50], s['t'][:, :, :50], y, yp, s['w0'], s['w1'], s['share'], s['share_total'], [0.1, 0.9])
    assert r['q'].shape == (1, 2, 13) and r['cum_q'].shape == (1, 2, 13) and r['win_q'].shape == (1, 2, 3)
    assert _bits(r['yhat'][0], s['xr'][0, :, 0]) and _bits(r['total'][0], s['win'][0, :, 0])
    assert _bits(r['cum_q'][:, :, 0], r['q'][:, :, 0])
