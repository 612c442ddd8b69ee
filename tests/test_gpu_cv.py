"""GPU tests of batched cross-validation (run with `-m gpu` on an MI355X): tsf_cross_validate against the library's own
fit_ragged / predict / predict_intervals on the explicitly cut prefix panels (bit for bit), a sample of folds against
the canonical CPU oracle, and the metrics against Prophet's rolling_mean_by_h in exact arithmetic
(oracle/cv_metrics_ref.py) within its tolerance -- on benign panels and at the call's edges: outliers, mape's NaN
threshold, 4-byte y, row counts around the wave width, one-row groups, many folds, failed fits and zero-fold series
among OK ones, ragged explicit columns, and more folds than one launch grid holds."""
import os
import subprocess
import types

import numpy as np
import pytest

from oracle import cv_metrics_ref as cref
from tests import helpers
from tests.test_cv_plan import window_rows

pytestmark = pytest.mark.gpu
DAY = 86400 * 10 ** 9
SEAS = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _series_rows(ds, y, extra, offsets, n):
    """ds, y, extra columns of series n of an aligned (offsets None) or ragged panel."""
    if offsets is None:
        return ds, y[n], None if extra is None else extra
    a, b = int(offsets[n]), int(offsets[n + 1])
    return ds[a:b], y[a:b], None if extra is None else extra[:, a:b]


def _by_hand(fc, _lib, spec, cv, ds, y, offsets=None, floor=None, cap=None, extra=None, intervals=False,
             n_samples=200, width=0.8, seed=0, series_key=None):
    """The folds done by hand: prefix panels cut on the host, one fit_ragged per optimiser (fbprophet's rule for
    algorithm AUTO, with its Newton retry), predict / predict_intervals on the padded holdout rows."""
    F = len(cv.cutoff)
    N = len(cv.status)
    fs = cv.fold_series
    parts = [_series_rows(ds, y, extra, offsets, int(fs[f])) for f in range(F)]
    hist, hold = cv.hist_rows.astype(np.int64), cv.hold_rows.astype(np.int64)
    fl = None if floor is None else np.broadcast_to(np.asarray(floor, np.float64), (N,))[fs]
    cp = None if cap is None else np.broadcast_to(np.asarray(cap, np.float64), (N,))[fs]
    algo = spec.lbfgs.get('algorithm', _lib.ALGO_LBFGS)
    kw = {k: v for k, v in spec.to_dict().items() if k not in ('lbfgs',)}
    opts = {k: v for k, v in spec.lbfgs.items() if k != 'algorithm'}
    sp_l = fc.ModelSpec(algorithm=_lib.ALGO_LBFGS, **kw, **opts)
    sp_n = fc.ModelSpec(algorithm=_lib.ALGO_NEWTON, **kw, **opts)
    out = {k: None for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval', 'grid')}
    res = {k: [None] * F for k in out}

    def fit(sp, idx):
        if len(idx) == 0:
            return
        off = np.concatenate([[0], np.cumsum(hist[idx])]).astype(np.int64)
        dsp = np.concatenate([parts[f][0][:hist[f]] for f in idx])
        yp = np.concatenate([parts[f][1][:hist[f]] for f in idx])
        exp = None if extra is None else np.concatenate([parts[f][2][:, :hist[f]] for f in idx], axis=1)
        r = fc.fit_ragged(sp, off, dsp, yp, floor=None if fl is None else fl[idx], cap=None if cp is None else cp[idx],
                          extra=exp)
        for i, f in enumerate(idx):
            for k in res:
                res[k][f] = getattr(r, k)[i]

    idx = np.arange(F)
    if algo == _lib.ALGO_AUTO:
        newton = hist < 100
        fit(sp_l, idx[~newton])
        st = np.array([res['status'][f] for f in idx[~newton]], dtype=np.int64)
        fit(sp_n, idx[~newton][np.isin(st, [_lib.ST_LSFAIL, _lib.ST_INIT_NONFINITE, _lib.ST_EVAL_LIMIT])])
        fit(sp_n, idx[newton])
    else:
        fit(sp_l if algo == _lib.ALGO_LBFGS else sp_n, idx)
    for k in res:
        res[k] = np.array(res[k]) if k != 'grid' else np.array(res[k], dtype=_lib.GRID_DTYPE)
    Hm = int(hold.max())
    fut = np.zeros((F, Hm), np.int64)
    exf = None if extra is None else np.zeros((F, extra.shape[0], Hm))
    for f in range(F):
        j = hist[f] + np.minimum(np.arange(Hm), hold[f] - 1)
        fut[f] = parts[f][0][j]
        if exf is not None:
            exf[f] = parts[f][2][:, j]
    if intervals:
        key = np.arange(N, dtype=np.int64) if series_key is None else np.asarray(series_key, np.int64)
        c = np.concatenate([np.arange(k) for k in cv.n_folds]).astype(np.uint64)
        with np.errstate(over='ignore'):
            fkey = (key[fs].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + c).view(np.int64)
        yh, lo, hi = fc.predict_intervals(spec, res['theta'], res['y_scale'], res['grid'], fut, floor=fl, cap=cp,
                                          extra_future=exf, series_key=fkey, uncertainty_samples=n_samples,
                                          interval_width=width, seed=seed)
    else:
        yh = fc.predict(spec, res['theta'], res['y_scale'], res['grid'], fut, floor=fl, cap=cp, extra_future=exf)
        lo = hi = None
    flat = lambda a: None if a is None else np.concatenate([a[f, :hold[f]] for f in range(F)])   # noqa: E731
    return res, flat(yh), flat(lo), flat(hi)


def _assert_same_folds(cv, res, yh, lo, hi, folds=None, rows=None):
    """cv's folds (all, or the plan indices `folds` with their holdout rows `rows`) are the by-hand ones, bit for bit."""
    fsel = slice(None) if folds is None else folds
    rsel = slice(None) if rows is None else rows
    for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval'):
        got = getattr(cv.fit, k)[fsel]
        assert helpers.n_bit_diff(got, res[k]) == 0 if k in ('theta', 'y_scale', 'fval') else \
            np.array_equal(got, res[k]), k
    assert cv.fit.grid[fsel].tobytes() == res['grid'].tobytes()
    assert helpers.n_bit_diff(cv.yhat[rsel], yh) == 0
    if lo is not None:
        assert helpers.n_bit_diff(cv.yhat_lower[rsel], lo) == 0 and helpers.n_bit_diff(cv.yhat_upper[rsel], hi) == 0


def _assert_metrics(_lib, cv, rolling_window, series=None):
    """Metrics against the exact reference (oracle/cv_metrics_ref.py), per series (all, or those in `series`) and metric
    row, within its tolerance TOL_C u (E - gb + 2) M_win; rmse is the square root of the returned mse, bit for bit;
    the metric rows of a series whose fit failed are NaN.  Returns the largest err / tol."""
    ro, mo = cv.row_offsets, cv.metric_offsets
    worst = 0.0
    for n in range(len(cv.status)) if series is None else series:
        a, b = int(ro[n]), int(ro[n + 1])
        m0, m1 = int(mo[n]), int(mo[n + 1])
        if b == a:
            assert m1 == m0 and cv.n_folds[n] == 0
            continue
        f = cv.row_fold[a:b]
        h = cv.ds[a:b] - cv.cutoff[f]
        y, yh = cv.y[a:b], cv.yhat[a:b]
        w = window_rows(rolling_window, b - a)
        if cv.status[n] == _lib.CV_FIT_FAILED:
            for k in ('mse', 'rmse', 'mae', 'mape') + (('coverage',) if cv.coverage is not None else ()):
                assert np.all(np.isnan(getattr(cv, k)[m0:m1])), (n, k)
            continue
        assert cv.status[n] == _lib.CV_OK
        lo = None if cv.coverage is None else cv.yhat_lower[a:b]
        hi = None if cv.coverage is None else cv.yhat_upper[a:b]
        r = cref.cv_metrics(y, yh, h, w, lo, hi)
        assert np.array_equal(cv.horizon[m0:m1], r['horizon']), n
        for name in cref.METRICS:
            got = getattr(cv, name)
            if got is None:
                continue
            got = got[m0:m1]
            if r[name] is None:
                assert np.all(np.isnan(got)), (n, name)
                continue
            q = r[name].err_over_tol(got)
            assert q.max() <= 1.0, (n, name, int(np.argmax(q)), float(q.max()), got[np.argmax(q)],
                                    r[name].value()[np.argmax(q)])
            worst = max(worst, float(q.max()))
        assert helpers.n_bit_diff(cv.rmse[m0:m1], np.sqrt(cv.mse[m0:m1])) == 0, n
    return worst


def _sub_plan(cv, idx):
    """The plan of series idx of a call, as _by_hand takes it, with their fold and holdout-row indices in the call."""
    fo, ro = cv.fold_offsets, cv.row_offsets
    folds = np.concatenate([np.arange(fo[n], fo[n + 1]) for n in idx]).astype(np.int64)
    rows = np.concatenate([np.arange(ro[n], ro[n + 1]) for n in idx]).astype(np.int64)
    sub = types.SimpleNamespace(cutoff=cv.cutoff[folds], status=cv.status[idx], hist_rows=cv.hist_rows[folds],
                                hold_rows=cv.hold_rows[folds], n_folds=cv.n_folds[idx],
                                fold_series=np.repeat(np.arange(len(idx), dtype=np.int64), cv.n_folds[idx]))
    return sub, folds, rows


def _ragged(parts):
    """(offsets, ds, y) of a ragged panel from per-series (ds, y) pairs."""
    off = np.concatenate([[0], np.cumsum([len(d) for d, _ in parts])]).astype(np.int64)
    return off, np.concatenate([d for d, _ in parts]).astype(np.int64), np.concatenate([v for _, v in parts])


def test_cfg2_like_aligned_quadratic_route(env):
    """BASELINE cfg2's model and shape (linear / additive yearly + weekly, 730 daily rows, horizon 90 d: 9 cutoffs) on
    a small aligned panel: every fold as fit_ragged on its prefix, 9 grids for 9 cutoffs, intervals, metrics."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N = 24
    ds, y = synth.make_panel(N, 730, 'linear', seed=11)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    cv = fc.cross_validate(spec, ds, y, 90 * DAY, intervals=True, uncertainty_samples=200, seed=7)
    assert list(cv.n_folds) == [9] * N and (cv.status == 0).all()
    assert fc.last_cv_grids() == (9, 1)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, intervals=True, n_samples=200, seed=7)
    _assert_same_folds(cv, res, yh, lo, hi)
    _assert_metrics(_lib, cv, 0.1)
    # without intervals: the same fits and point forecasts
    cv2 = fc.cross_validate(spec, ds, y, 90 * DAY, rolling_window=0.3)
    assert np.array_equal(cv2.fit.theta, cv.fit.theta) and np.array_equal(cv2.yhat, cv.yhat) and cv2.coverage is None
    _assert_metrics(_lib, cv2, 0.3)
    df = fc.performance_metrics(cv2)
    assert list(df.columns) == ['series', 'horizon', 'mse', 'rmse', 'mae', 'mape'] and len(df) == len(cv2.horizon)


def test_reference_model_ragged_fixture(env):
    """The reference's model (logistic growth, multiplicative seasonality, auto seasonalities of the full history) on
    its own irregular fixture through the ragged entry point; a sample of folds against the canonical oracle."""
    fc, _lib = env
    from oracle import canon_lib as cl
    g = np.load(helpers.GOLDEN + '/fixture_751.npz')
    off, ds, y = g['offsets'], g['raw_ds_ns'], g['raw_y'].astype(np.float64)
    seas = fc.ModelSpec.auto_seasonalities(ds[off[0]:off[1]], seasonality_mode='multiplicative')
    spec = fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=seas,
                        algorithm=_lib.ALGO_AUTO)
    cap = np.array([y[off[n]:off[n + 1]].max() * 1.1 for n in range(2)])
    floor = np.zeros(2)
    kw = dict(offsets=off, floor=floor, cap=cap, period=20 * DAY, initial=300 * DAY)
    cv = fc.cross_validate(spec, ds, y, 40 * DAY, intervals=True, uncertainty_samples=100, series_key=[751, 752], **kw)
    assert (cv.status == 0).all() and cv.n_folds.min() >= 5
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off, floor, cap, intervals=True, n_samples=100,
                               series_key=[751, 752])
    _assert_same_folds(cv, res, yh, lo, hi)
    _assert_metrics(_lib, cv, 0.1)
    csp = cl.make_spec(growth='logistic', seasonalities=[(s['period'], s['fourier_order'], 'multiplicative', 10.0)
                                                         for s in seas])
    for f in (0, len(cv.cutoff) // 2, len(cv.cutoff) - 1):
        n = int(cv.fold_series[f])
        d, yy = ds[off[n]:off[n + 1]], y[off[n]:off[n + 1]]
        h0, h1 = int(cv.hist_rows[f]), int(cv.hist_rows[f] + cv.hold_rows[f])
        o = cl.fit(csp, d[:h0], yy[:h0], 0.0, cap[n])
        assert (cv.fit.status[f], cv.fit.n_iter[f], cv.fit.n_eval[f]) == (o['status'], o['n_iter'], o['n_eval'])
        assert helpers.n_bit_diff(cv.fit.fval[f:f + 1], np.array([o['f']])) == 0
        yo, _ = cl.predict(csp, o, d[h0:h1], 0.0, cap[n])
        r0 = int(cv.row_offsets[n]) + int(cv.hold_rows[int(cv.fold_offsets[n]):f].sum())
        assert np.max(np.abs(cv.yhat[r0:r0 + h1 - h0] - yo) / np.abs(yo)) <= 1e-4


def test_holidays_aligned(env):
    """Explicit columns (holiday indicators): the fold panel carries them, the holdout rows use their own values."""
    fc, _lib = env
    from time_series_spark_amd import synth
    ds = synth.daily_grid(500)
    ex, names = synth.holiday_matrix(ds, 6)
    _, y = synth.make_panel(6, 500, 'linear', seed=5, holidays=ex)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:], extra=[{'name': n} for n in names])
    cv = fc.cross_validate(spec, ds, y, 60 * DAY, extra=ex, period=60 * DAY)
    assert (cv.status == 0).all()
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, extra=ex)
    _assert_same_folds(cv, res, yh, lo, hi)
    _assert_metrics(_lib, cv, 0.1)


def test_folds_cross_100_rows_newton_per_fold(env):
    """algorithm AUTO: folds of fewer than 100 rows are fitted by Newton, the others by L-BFGS, in one call; a ragged
    irregular panel with an error series among them."""
    fc, _lib = env
    from time_series_spark_amd import synth
    rng = np.random.default_rng(3)
    ds_all, y_all = synth.make_panel(5, 160, 'linear', seed=9)
    keep = [np.sort(rng.choice(160, size=k, replace=False)) for k in (160, 140, 120, 150)] + [np.arange(5)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in keep])]).astype(np.int64)
    ds = np.concatenate([ds_all[k] for k in keep])
    y = np.concatenate([y_all[i][k] for i, k in enumerate(keep)])
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:], algorithm=_lib.ALGO_AUTO)
    cv = fc.cross_validate(spec, ds, y, 14 * DAY, offsets=off, period=7 * DAY, initial=60 * DAY)
    assert cv.status[4] == _lib.CV_LESS_THAN_HORIZON and cv.n_folds[4] == 0 and (cv.status[:4] == 0).all()
    assert (cv.hist_rows < 100).any() and (cv.hist_rows >= 100).any()
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off)
    _assert_same_folds(cv, res, yh, lo, hi)
    assert set(cv.fit.status[cv.hist_rows < 100]) <= {_lib.ST_NEWTON_CONVERGED, _lib.ST_MAXIT, _lib.ST_NEWTON_FAIL}
    _assert_metrics(_lib, cv, 0.1)


def test_auto_retries_failed_line_searches_with_newton(env):
    """algorithm AUTO with every tolerance zero on helpers.retry_panel (2 - 3 folds per series): the L-BFGS folds end in
    a failed line search and are fitted once more with Newton, beside the folds of fewer than 100 rows that go to Newton
    at once -- all three launches of the rule in one call.  The precondition is asserted on the by-hand L-BFGS fits."""
    fc, _lib = env
    off, ds, y, kw = helpers.retry_panel()
    spec = fc.ModelSpec(algorithm=_lib.ALGO_AUTO, **kw, **helpers.ZERO_TOL)
    cv = fc.cross_validate(spec, ds, y, 7 * DAY, offsets=off, period=56 * DAY, initial=25 * DAY)
    assert list(cv.n_folds) == [3, 3, 3, 2] and (cv.status == 0).all()
    launches = fc.last_cv_grids()[1]
    lb = cv.hist_rows >= 100
    assert lb.sum() == 5 and (~lb).sum() == 6
    first, _, _, _ = _by_hand(fc, _lib, helpers.explicit_algorithm(spec, _lib.ALGO_LBFGS), cv, ds, y, off)
    retried = np.isin(first['status'][lb], helpers.retry_statuses(_lib))
    print('L-BFGS statuses of the folds of >= 100 rows:', first['status'][lb])
    assert retried.any() and launches == 3                                  # the L-BFGS, the retry and the Newton launch
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off)
    _assert_same_folds(cv, res, yh, lo, hi)


def test_abi_cv_plain_c(env, tmp_path):
    """tests/c/abi_cv.c drives tsf_cross_validate from plain C99 and writes what the binding returns."""
    fc, _lib = env
    from time_series_spark_amd import synth
    root = helpers.ROOT
    N, T = 4, 400
    ds, y = synth.make_panel(N, T, 'linear', seed=2)
    ds.astype(np.int64).tofile(str(tmp_path / 'ds.i64'))
    np.ascontiguousarray(y, np.float64).tofile(str(tmp_path / 'y.f64'))
    exe = str(tmp_path / 'abi_cv')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_cv.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(N), str(T), str(tmp_path / 'ds.i64'), str(tmp_path / 'y.f64'), str(tmp_path / 'out.f64')])
    got = np.fromfile(str(tmp_path / 'out.f64'))
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:])
    cv = fc.cross_validate(spec, ds, y, 30 * DAY)
    want = np.concatenate([cv.fit.theta.ravel(), cv.yhat, cv.mse, cv.mape])
    assert helpers.n_bit_diff(got, want) == 0


def test_validator_driver_on_reference_fixture(env, tmp_path):
    """The validator job from files to files on the reference's fixture (hive layout, the reference's model, intervals)
    writes the numbers the Python API gives for the same series, keys and settings."""
    fc, _lib = env
    import pandas as pd
    import yaml
    from time_series_spark_amd import validator_driver
    g = np.load(helpers.GOLDEN + '/fixture_751.npz')
    d = tmp_path / 'in' / 'series_id=751'
    d.mkdir(parents=True)
    stamps = pd.DatetimeIndex(g['raw_ds_ns'].astype('datetime64[ns]')).strftime('%Y-%m-%d %H:%M:%S').values
    with open(str(d / 'part-0.csv'), 'w') as fh:
        fh.write(''.join('%d,%s,%d\n' % (k, s, v) for k, s, v in zip(g['raw_dim_id'], stamps, g['raw_y'])))
    cfg = {'model': {'floor': 0, 'cap_multiplier': 1.1},
           'io': {'input': str(tmp_path / 'in'), 'metrics': str(tmp_path / 'm'), 'folds': str(tmp_path / 'f')},
           'cv': {'horizon': '40 days', 'period': '20 days', 'initial': '300 days', 'rolling_window': 0.2,
                  'intervals': True, 'uncertainty_samples': 100, 'seed': 3}}
    with open(str(tmp_path / 'cfg.yaml'), 'w') as fh:
        yaml.safe_dump(cfg, fh)
    assert validator_driver.main(['x', str(tmp_path / 'cfg.yaml')]) == 0
    m = pd.read_parquet(str(tmp_path / 'm'))
    f = pd.read_parquet(str(tmp_path / 'f'))
    # the Python API on the same series
    off, ds, y = g['offsets'], g['raw_ds_ns'], g['raw_y'].astype(np.float64)
    seas = fc.ModelSpec.auto_seasonalities(ds[off[0]:off[1]], seasonality_mode='multiplicative')
    spec = fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=seas, algorithm=_lib.ALGO_AUTO)
    cap = np.array([y[off[n]:off[n + 1]].max() * 1.1 for n in range(2)])
    key = (np.int64(751) << 32) | g['dim_ids'].astype(np.int64)
    cv = fc.cross_validate(spec, ds, y, 40 * DAY, 20 * DAY, 300 * DAY, offsets=off, floor=np.zeros(2), cap=cap,
                           rolling_window=0.2, intervals=True, uncertainty_samples=100, seed=3, series_key=key)
    assert list(m.columns) == ['series_id', 'dim_id', 'horizon', 'mse', 'rmse', 'mae', 'mape', 'coverage']
    assert (m['series_id'] == 751).all() and np.array_equal(m['dim_id'].to_numpy(), g['dim_ids'][cv.metric_series])
    assert np.array_equal(m['horizon'].to_numpy().astype(np.int64), cv.horizon)
    for k in ('mse', 'rmse', 'mae', 'mape', 'coverage'):
        assert helpers.n_bit_diff(m[k].to_numpy(), getattr(cv, k)) == 0, k
    assert np.array_equal(f['ds'].to_numpy().astype(np.int64), cv.ds)
    assert helpers.n_bit_diff(f['yhat'].to_numpy(), cv.yhat) == 0
    assert helpers.n_bit_diff(f['yhat_upper'].to_numpy(), cv.yhat_upper) == 0


# ---- the call at its edges -----------------------------------------------------------------------------------------

# w = 81 is 9 whole groups of the 9-fold aligned panel (E - w on a group boundary), 80 and 82 are not; 0 -> w = 1,
# 1 -> w = n (one metric row)
CFG2_WINDOWS = (0.1, 80.5 / 810, 82.5 / 810, 0.0, 1.0)


def test_spike_after_last_cutoff(env):
    """Outliers on the row one day after the last cutoff -- in no fold's history, in the holdout of the last two folds
    (horizons 1 d and 46 d): y scaled by 1e6 and by 1e12 in two series, a large negative value in a third.  Every fit
    and forecast is the spike-free panel's, bit for bit; the metrics of every window after the spike's horizon must not
    cancel, and those of the untouched series are unchanged."""
    fc, _lib = env
    N = 8
    from time_series_spark_amd import synth
    ds, y = synth.make_panel(N, 730, 'linear', seed=21)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    T0 = 730 - 90
    ys = y.copy()
    ys[1, T0] *= 1e6
    ys[2, T0] *= 1e12
    ys[3, T0] = -3e13
    clean = fc.cross_validate(spec, ds, y, 90 * DAY, intervals=True, uncertainty_samples=200, seed=5)
    for rw in CFG2_WINDOWS:
        cv = fc.cross_validate(spec, ds, ys, 90 * DAY, rolling_window=rw, intervals=True, uncertainty_samples=200,
                               seed=5)
        assert (cv.status == 0).all() and list(cv.n_folds) == [9] * N
        for k in ('theta', 'y_scale', 'fval'):
            assert helpers.n_bit_diff(getattr(cv.fit, k), getattr(clean.fit, k)) == 0, k
        for k in ('status', 'n_iter', 'n_eval'):
            assert np.array_equal(getattr(cv.fit, k), getattr(clean.fit, k)), k
        for k in ('yhat', 'yhat_lower', 'yhat_upper'):
            assert helpers.n_bit_diff(getattr(cv, k), getattr(clean, k)) == 0, k
        assert np.sum(cv.y != clean.y) == 6                     # 3 series x 2 folds
        _assert_metrics(_lib, cv, rw)
        if rw == 0.1:
            mo = cv.metric_offsets
            for n in (0, 4, 5, 6, 7):
                for k in ('mse', 'mae', 'mape', 'coverage'):
                    assert helpers.n_bit_diff(getattr(cv, k)[mo[n]:mo[n + 1]], getattr(clean, k)[mo[n]:mo[n + 1]]) == 0
            assert np.all(cv.mse > 0) and np.all(np.isfinite(cv.rmse))
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, ys, intervals=True, n_samples=200, seed=5)
    _assert_same_folds(cv, res, yh, lo, hi)


def test_mape_threshold(env):
    """min |y| of exactly 0, 0.99e-8, 1e-8, 1.01e-8 and -0.99e-8 (on a holdout-only row), and a finite tiny |y| at
    horizon 1 d: mape is NaN for the whole series exactly when min |y| < 1e-8; the other metrics are unaffected."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N, T = 7, 400
    ds, y = synth.make_panel(N, T, 'linear', seed=4)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:])
    r = T - 30                                                  # the row one day after the last cutoff
    for n, v in enumerate((0.0, 0.99e-8, 1e-8, 1.01e-8, -0.99e-8, 3e-8)):
        y[n, r] = v
    y[5, r - 15] = -2e-8                                        # (another fold's horizon 1 d as well)
    cv = fc.cross_validate(spec, ds, y, 30 * DAY, intervals=True, uncertainty_samples=100)
    assert (cv.status == 0).all()
    mo = cv.metric_offsets
    nan = [bool(np.all(np.isnan(cv.mape[mo[n]:mo[n + 1]]))) for n in range(N)]
    assert nan == [True, True, False, False, True, False, False]
    assert np.isfinite(cv.mse).all() and np.isfinite(cv.mae).all()
    _assert_metrics(_lib, cv, 0.1)
    cv0 = fc.cross_validate(spec, ds, y, 30 * DAY, rolling_window=0.0)
    _assert_metrics(_lib, cv0, 0.0)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv0, ds, y)
    _assert_same_folds(cv0, res, yh, lo, hi)


def test_y_dtypes(env):
    """The same panel as float64, float32 and int32 y (aligned and ragged): the 4-byte copy of the fold panel and the
    holdout y conversion give fits, forecasts and metrics bit-identical to the float64 call on the converted values."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N, T = 6, 500
    ds, y = synth.make_panel(N, T, 'linear', seed=8)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    keys = ('mse', 'rmse', 'mae', 'mape', 'coverage', 'yhat', 'yhat_lower', 'yhat_upper')
    lens = [500, 430, 470, 380, 500, 455]
    for yt in (((y + 0.37) * 1.3).astype(np.float32), y.astype(np.int32), (y - 2e4).astype(np.int32)):
        for ragged in (False, True):
            if ragged:
                off, dsr, yr = _ragged([(ds[-k:], yt[n, -k:]) for n, k in enumerate(lens)])
                args, kw = (dsr, yr), dict(offsets=off)
                args64 = (dsr, yr.astype(np.float64))
            else:
                args, kw, args64 = (ds, yt), {}, (ds, yt.astype(np.float64))
            cv = fc.cross_validate(spec, *args, 60 * DAY, intervals=True, uncertainty_samples=100, **kw)
            ref = fc.cross_validate(spec, *args64, 60 * DAY, intervals=True, uncertainty_samples=100, **kw)
            assert (cv.status == 0).all()
            for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval'):
                assert helpers.n_bit_diff(getattr(cv.fit, k), getattr(ref.fit, k)) == 0, (yt.dtype, ragged, k)
            assert cv.fit.grid.tobytes() == ref.fit.grid.tobytes()
            for k in keys:
                assert helpers.n_bit_diff(getattr(cv, k), getattr(ref, k)) == 0, (yt.dtype, ragged, k)
            assert helpers.n_bit_diff(cv.y, ref.y) == 0
            _assert_metrics(_lib, cv, 0.1)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, *args, offsets=off, intervals=True, n_samples=100)
    _assert_same_folds(cv, res, yh, lo, hi)


WAVE_ROWS = (1, 63, 64, 65, 127, 128, 129, 4100)


def _one_fold_panel(rows, seed, horizon=30 * DAY, hist=200):
    """A ragged panel of one fold per series: `hist` daily rows, then rows[n] holdout rows spread over
    (cutoff, cutoff + horizon], every one at its own horizon.  period = horizon, initial = hist - 10 days."""
    from time_series_spark_amd import synth
    ds_h, y_h = synth.make_panel(len(rows), hist + 1, 'linear', seed=seed)
    rng = np.random.default_rng(seed)
    cut = int(ds_h[hist - 1])
    parts = []
    for n, k in enumerate(rows):
        step = horizon // k
        d = np.concatenate([ds_h[:hist], cut + horizon - step * np.arange(k - 1, -1, -1, dtype=np.int64)])
        v = np.concatenate([y_h[n, :hist], y_h[n, hist] * (1 + 0.1 * rng.standard_normal(k))])
        parts.append((d, v))
    return _ragged(parts) + (horizon, horizon, (hist - 10) * DAY)


def test_wave_boundaries(env):
    """Holdout rows per series of 1, 63, 64, 65, 127, 128, 129 and 4 100 (one fold each, distinct horizons): with
    w = 1 as many metric rows, across the 64-row steps of the output loop; w = n (one row); w = 10 %; windows that
    leave the 4 100-row series 64 and 128 metric rows."""
    fc, _lib = env
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:])
    off, ds, y, horizon, period, initial = _one_fold_panel(WAVE_ROWS, 12)
    # w = 4 100 - 64 + 1 and - 128 + 1 leave the long series 64 and 128 metric rows
    for rw in (0.0, 1.0, 0.1, 4037.5 / 4100, 3973.5 / 4100):
        cv = fc.cross_validate(spec, ds, y, horizon, period, initial, offsets=off, rolling_window=rw,
                               intervals=True, uncertainty_samples=50)
        assert (cv.status == 0).all() and list(cv.n_folds) == [1] * len(WAVE_ROWS)
        assert list(cv.n_holdout) == list(WAVE_ROWS)
        want = {0.0: list(WAVE_ROWS), 1.0: [1] * len(WAVE_ROWS)}.get(rw, [k - window_rows(rw, k) + 1 for k in WAVE_ROWS])
        assert list(cv.n_metric) == want
        assert rw in (0.0, 0.1, 1.0) or want[-1] in (64, 128)
        _assert_metrics(_lib, cv, rw)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off, intervals=True, n_samples=50)
    _assert_same_folds(cv, res, yh, lo, hi)


def test_group_shapes(env):
    """Groups of one row (irregular timestamps at ns resolution: every holdout row its own horizon), many folds per
    series (period 1 d: 90 folds, groups of 90 rows, w = 90 and 45), and folds of a single holdout row (horizon 1 d:
    one group of every fold's row)."""
    fc, _lib = env
    from time_series_spark_amd import synth
    rng = np.random.default_rng(17)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:])
    # one-row groups
    parts = []
    for n, T in enumerate((300, 260, 330)):
        d0, v = synth.make_panel(1, T, 'linear', seed=40 + n)
        parts.append((d0 + rng.integers(0, DAY, T), v[0]))
    off, ds, y = _ragged(parts)
    cv = fc.cross_validate(spec, ds, y, 20 * DAY, 10 * DAY, 100 * DAY, offsets=off, rolling_window=0.1)
    assert (cv.status == 0).all() and cv.n_folds.min() >= 10
    ro = cv.row_offsets
    for n in range(3):
        h = cv.ds[ro[n]:ro[n + 1]] - cv.cutoff[cv.row_fold[ro[n]:ro[n + 1]]]
        assert len(np.unique(h)) == len(h)
    _assert_metrics(_lib, cv, 0.1)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off)
    _assert_same_folds(cv, res, yh, lo, hi)
    # many folds
    ds, y = synth.make_panel(4, 200, 'linear', seed=41)
    for rw in (0.1, 0.05):
        cv = fc.cross_validate(spec, ds, y, 10 * DAY, DAY, 100 * DAY, rolling_window=rw)
        assert (cv.status == 0).all() and list(cv.n_folds) == [90] * 4 and list(cv.n_metric) == [10] * 4
        _assert_metrics(_lib, cv, rw)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y)
    _assert_same_folds(cv, res, yh, lo, hi)
    # one holdout row per fold
    cv = fc.cross_validate(spec, ds, y, DAY, DAY, 150 * DAY, rolling_window=0.1, intervals=True, uncertainty_samples=50)
    assert (cv.status == 0).all() and (cv.hold_rows == 1).all() and cv.n_folds.min() >= 49
    assert list(cv.n_metric) == [1] * 4
    _assert_metrics(_lib, cv, 0.1)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, intervals=True, n_samples=50)
    _assert_same_folds(cv, res, yh, lo, hi)


def _status_panel():
    """A ragged panel whose zero-fold series (LESS_THAN_HORIZON, NO_CUTOFF, TOO_FEW) sit between OK ones, for horizon
    30 d, period 30 d and the default initial (90 d)."""
    from time_series_spark_amd import synth
    d, v = synth.make_panel(4, 400, 'linear', seed=50)
    lone = np.array([d[0] - 400 * DAY])
    parts = [(d[:300], v[0, :300]), (d[:20], v[1, :20]), (d[:250], v[1, :250]), (d[:100], v[2, :100]),
             (d[:280], v[2, :280]), (np.concatenate([lone, d[:200]]), np.concatenate([[5e3], v[3, :200]])),
             (d[:320], v[3, :320])]
    return _ragged(parts)


def test_statuses_between_ok_series(env):
    """Zero-fold series placed between OK series have no fold, holdout or metric row and leave their neighbours'
    results as the panel without them gives them; a logistic series with cap <= floor has every fold fail with
    TSF_ST_CAP, comes back TSF_CV_FIT_FAILED with NaN metric rows, and its neighbours are unaffected."""
    fc, _lib = env
    from time_series_spark_amd import synth
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:])
    off, ds, y = _status_panel()
    cv = fc.cross_validate(spec, ds, y, 30 * DAY, 30 * DAY, offsets=off, intervals=True, uncertainty_samples=50)
    assert list(cv.status) == [0, _lib.CV_LESS_THAN_HORIZON, 0, _lib.CV_NO_CUTOFF, 0, _lib.CV_TOO_FEW, 0]
    assert list(cv.n_folds[[1, 3, 5]]) == [0, 0, 0] and list(cv.n_metric[[1, 3, 5]]) == [0, 0, 0]
    _assert_metrics(_lib, cv, 0.1)
    ok = [0, 2, 4, 6]
    parts = [(ds[off[n]:off[n + 1]], y[off[n]:off[n + 1]]) for n in ok]
    off2, ds2, y2 = _ragged(parts)
    cv2 = fc.cross_validate(spec, ds2, y2, 30 * DAY, 30 * DAY, offsets=off2, series_key=ok, intervals=True,
                            uncertainty_samples=50)
    for k in ('theta', 'fval', 'status', 'n_iter'):
        assert helpers.n_bit_diff(getattr(cv.fit, k), getattr(cv2.fit, k)) == 0, k
    for k in ('yhat', 'yhat_lower', 'yhat_upper', 'horizon', 'mse', 'rmse', 'mae', 'mape', 'coverage'):
        assert helpers.n_bit_diff(getattr(cv, k), getattr(cv2, k)) == 0, k
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off, intervals=True, n_samples=50)
    _assert_same_folds(cv, res, yh, lo, hi)
    # logistic, per-series floor / cap on an aligned panel; series 2 has cap == floor
    N = 5
    ds, y = synth.make_panel(N, 400, 'logistic', seed=51)
    floor = np.array([0.0, 100.0, 200.0, -50.0, 10.0])
    cap = y.max(axis=1) * 1.2
    cap[2] = floor[2]
    lspec = fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=SEAS[1:])
    cv = fc.cross_validate(lspec, ds, y, 40 * DAY, floor=floor, cap=cap, intervals=True, uncertainty_samples=50)
    fo = cv.fold_offsets
    assert list(cv.status) == [0, 0, _lib.CV_FIT_FAILED, 0, 0]
    assert (cv.fit.status[fo[2]:fo[3]] == _lib.ST_CAP).all() and cv.n_metric[2] > 0
    _assert_metrics(_lib, cv, 0.1)
    keep = [0, 1, 3, 4]
    cv2 = fc.cross_validate(lspec, ds, y[keep], 40 * DAY, floor=floor[keep], cap=cap[keep], series_key=keep,
                            intervals=True, uncertainty_samples=50)
    _, fk, rk = _sub_plan(cv, keep)
    mk = np.concatenate([np.arange(cv.metric_offsets[n], cv.metric_offsets[n + 1]) for n in keep])
    for k in ('theta', 'fval', 'status', 'n_iter'):
        assert helpers.n_bit_diff(getattr(cv.fit, k)[fk], getattr(cv2.fit, k)) == 0, k
    for k in ('yhat', 'yhat_lower', 'yhat_upper'):
        assert helpers.n_bit_diff(getattr(cv, k)[rk], getattr(cv2, k)) == 0, k
    for k in ('horizon', 'mse', 'rmse', 'mae', 'mape', 'coverage'):
        assert helpers.n_bit_diff(getattr(cv, k)[mk], getattr(cv2, k)) == 0, k
    res, yh, lo, hi = _by_hand(fc, _lib, lspec, cv, ds, y, floor=floor, cap=cap, intervals=True, n_samples=50)
    _assert_same_folds(cv, res, yh, lo, hi)


def test_ragged_holidays(env):
    """Explicit (holiday) columns on a ragged panel: each fold's columns are its own series' rows, cut on the device
    for the fit and read at the holdout rows for the forecast."""
    fc, _lib = env
    from time_series_spark_amd import synth
    ds_all = synth.daily_grid(520)
    ex_all, names = synth.holiday_matrix(ds_all, 6)
    _, y_all = synth.make_panel(5, 520, 'linear', seed=55, holidays=ex_all)
    spans = [(0, 520), (40, 500), (100, 520), (0, 360), (20, 470)]
    off, ds, y = _ragged([(ds_all[a:b], y_all[n, a:b]) for n, (a, b) in enumerate(spans)])
    ex = np.concatenate([ex_all[:, a:b] for a, b in spans], axis=1)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:], extra=[{'name': n} for n in names])
    cv = fc.cross_validate(spec, ds, y, 45 * DAY, 40 * DAY, offsets=off, extra=ex, intervals=True,
                           uncertainty_samples=50)
    assert (cv.status == 0).all() and cv.n_folds.min() >= 3
    _assert_metrics(_lib, cv, 0.1)
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, off, extra=ex, intervals=True, n_samples=50)
    _assert_same_folds(cv, res, yh, lo, hi)


def test_more_folds_than_one_launch_grid(env):
    """8 000 short series x 9 folds = 72 000 folds: the expand and holdout kernels loop past their 65 535-block grid.
    Folds above index 65 535 are checked bit for bit against the folds done by hand on their series alone."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N = 8000
    ds, y = synth.make_panel(N, 80, 'linear', seed=60)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS[1:])
    cv = fc.cross_validate(spec, ds, y, 4 * DAY, 4 * DAY, 40 * DAY, intervals=True, uncertainty_samples=50,
                           ctx=fc.get_context())
    assert list(set(cv.n_folds)) == [9] and len(cv.cutoff) == 72000
    # (a short history's L-BFGS fit may fail; such a series is TSF_CV_FIT_FAILED, its metric rows NaN)
    assert set(cv.status) <= {_lib.CV_OK, _lib.CV_FIT_FAILED} and np.mean(cv.status == 0) > 0.9, \
        np.unique(cv.fit.status, return_counts=True)
    idx = [7281, 7282, 7500, 7777, 7999]            # (series 7281 holds folds 65 529 .. 65 537)
    sub, folds, rows = _sub_plan(cv, idx)
    assert folds.min() < 65535 < folds[9] and folds.max() == 71999
    res, yh, lo, hi = _by_hand(fc, _lib, spec, sub, ds, y[idx], intervals=True, n_samples=50, series_key=idx)
    _assert_same_folds(cv, res, yh, lo, hi, folds=folds, rows=rows)
    rng = np.random.default_rng(0)
    _assert_metrics(_lib, cv, 0.1, series=sorted(set(idx) | set(rng.choice(N, 200, replace=False).tolist())))
