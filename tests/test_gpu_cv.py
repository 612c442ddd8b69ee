"""GPU tests of batched cross-validation (run with `-m gpu` on an MI355X): tsf_cross_validate against the library's own
fit_ragged / predict / predict_intervals on the explicitly cut prefix panels (bit for bit), a sample of folds against
the canonical CPU oracle, and the metrics against Prophet's rolling_mean_by_h restated in numpy
(tests/test_cv_plan.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests.test_cv_plan import rolling_mean_by_h, window_rows

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


def _assert_same_folds(cv, res, yh, lo, hi):
    for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval'):
        assert helpers.n_bit_diff(getattr(cv.fit, k), res[k]) == 0 if k in ('theta', 'y_scale', 'fval') else \
            np.array_equal(getattr(cv.fit, k), res[k]), k
    assert cv.fit.grid.tobytes() == res['grid'].tobytes()
    assert helpers.n_bit_diff(cv.yhat, yh) == 0
    if lo is not None:
        assert helpers.n_bit_diff(cv.yhat_lower, lo) == 0 and helpers.n_bit_diff(cv.yhat_upper, hi) == 0


def _assert_metrics(_lib, cv, rolling_window):
    """Metrics against the numpy restatement, per series, within a sum-of-|terms| tolerance (every term is >= 0)."""
    ro, mo = cv.row_offsets, cv.metric_offsets
    for n in range(len(cv.status)):
        a, b = int(ro[n]), int(ro[n + 1])
        if b == a:
            assert mo[n + 1] == mo[n]
            continue
        f = cv.row_fold[a:b]
        h = cv.ds[a:b] - cv.cutoff[f]
        y, yh = cv.y[a:b], cv.yhat[a:b]
        w = window_rows(rolling_window, b - a)
        m0, m1 = int(mo[n]), int(mo[n + 1])
        terms = {'mse': (y - yh) ** 2, 'mae': np.abs(y - yh), 'mape': np.abs((y - yh) / y)}
        if cv.coverage is not None:
            terms['coverage'] = ((y >= cv.yhat_lower[a:b]) & (y <= cv.yhat_upper[a:b])).astype(np.float64)
        for name, x in terms.items():
            hs, want = rolling_mean_by_h(x, h, w)
            assert np.array_equal(cv.horizon[m0:m1], hs), name
            got = getattr(cv, name)[m0:m1]
            if name == 'mape' and np.min(np.abs(y)) < 1e-8:
                assert np.all(np.isnan(got))
                continue
            assert np.allclose(got, want, rtol=1e-10, atol=1e-300), (n, name)
            if name == 'mse':
                assert np.allclose(cv.rmse[m0:m1], np.sqrt(want), rtol=1e-10, atol=1e-300)


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
