"""GPU tests of the forecast decomposition (tsf_predict_components: predict_kernel's trend output, component_kernel,
the sampled trend of interval_sample_kernel) on the shape matrix of tests/forecast_cases.py.  Every output is pinned
exactly against the two entry points the forecast tests already pin (tsf_predict, tsf_predict_intervals), through the
order contract of include/tsf.h: a component is tsf_predict on a derived model whose masked-out coefficients are 0
(fma(x, 0, acc) = acc), the trend is tsf_predict with beta = 0, and the trend's interval is tsf_predict_intervals with
beta = 0 and no observation noise (dm_exp(-800) = 0)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import forecast_cases as fcs, helpers

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU component tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _table(fc, c):
    """every component fbprophet would form for the case's model (each seasonality, each extra alone -- all are
    regressors here --, the group totals), a mask spanning a seasonality and an extra column (or two seasonalities)
    scaled and unscaled, an empty mask"""
    cols = list(fc.component_columns(c.spec))
    last = c.K - 1
    cols += [('mixed0', 1 | (1 << last) | (1 << (last - 1)), 0), ('mixed1', 1 | (1 << last) | (1 << (last - 1)), 1),
             ('empty', 0, 1)]
    return cols


def _derived(fc, c, mask, scaled):
    """linear growth, k = m = delta = 0, every column additive, beta masked, y_scale of the series or 1, no floor / cap"""
    spec = fc.ModelSpec(growth='linear', n_changepoints=c.spec.n_changepoints,
                        seasonalities=[dict(s, mode='additive') for s in c.spec.seasonalities],
                        extra=[dict(e, mode='additive') for e in c.spec.extra])
    ncp = c.spec.n_changepoints
    theta = np.zeros_like(c.theta)
    keep = np.array([(mask >> j) & 1 for j in range(c.K)], dtype=bool)
    theta[:, 3 + ncp:] = np.where(keep, c.theta[:, 3 + ncp:], 0.0)
    ys = c.y_scale if scaled else np.ones(c.N)
    return fc.predict(spec, theta, ys, c.grid, c.fut, extra_future=c.extra)


def _components(fc, c, cols, fut=None, extra=None, **kw):
    return fc.predict_components(c.spec, c.theta, c.y_scale, c.grid, c.fut if fut is None else fut, floor=c.floor,
                                 cap=c.cap, extra_future=c.extra if extra is None else extra, columns=cols, **kw)


def _beta0(c, log_sigma=None):
    th = c.theta.copy()
    th[:, 3 + c.spec.n_changepoints:] = 0.0
    if log_sigma is not None:
        th[:, 2] = log_sigma
    return th


@pytest.mark.parametrize('name', list(fcs.CASES))
def test_components_on_the_shape_matrix(env, name):
    fc, _lib = env
    c = fcs.make(name)
    cols = _table(fc, c)
    r = _components(fc, c, cols)
    assert r.names == [n for n, _, _ in cols] and r.comp.shape == (c.N, len(cols), c.H)
    # yhat: tsf_predict's bits
    yhat = fc.predict(c.spec, c.theta, c.y_scale, c.grid, c.fut, floor=c.floor, cap=c.cap, extra_future=c.extra)
    assert np.array_equal(r.yhat.view(np.int64), yhat.view(np.int64))
    # trend: tsf_predict with every beta 0 (values; +-0 alike)
    tr = fc.predict(c.spec, _beta0(c), c.y_scale, c.grid, c.fut, floor=c.floor, cap=c.cap, extra_future=c.extra)
    assert np.array_equal(r.trend, tr)
    # each component: tsf_predict on the derived model
    for i, (cname, mask, scaled) in enumerate(cols):
        want = _derived(fc, c, mask, scaled)
        assert np.array_equal(r.comp[:, i, :], want), (name, cname)
        assert np.array_equal(r.terms[cname], want)
    assert (r.terms['empty'] == 0.0).all()
    # the decomposition adds up to yhat (up to the rounding of that expression: the device may contract it)
    tm, add = r.trend * (1.0 + r.terms['multiplicative_terms']), r.terms['additive_terms']
    err = np.abs(r.yhat - (tm + add))
    assert (err <= 4 * U * (np.abs(tm) + np.abs(add))).all(), (name, err.max())
    # a shared future grid (design table) and the same dates per series (computed in place): the same bits
    if c.shared:
        futN = np.ascontiguousarray(np.broadcast_to(c.fut, (c.N, c.H)))
        exN = None if c.extra is None else np.ascontiguousarray(np.broadcast_to(c.extra, (c.N,) + c.extra.shape))
        r2 = _components(fc, c, cols, futN, exN)
        for k in ('yhat', 'trend', 'comp'):
            assert np.array_equal(getattr(r2, k).view(np.int64), getattr(r, k).view(np.int64)), (name, k)


def _check_intervals(fc, c, cols, keys, n_samples, width):
    r = _components(fc, c, cols, intervals=True, series_key=keys, uncertainty_samples=n_samples,
                    interval_width=width, seed=17)
    yhat, lo, hi = fc.predict_intervals(c.spec, c.theta, c.y_scale, c.grid, c.fut, floor=c.floor, cap=c.cap,
                                        extra_future=c.extra, series_key=keys, uncertainty_samples=n_samples,
                                        interval_width=width, seed=17)
    assert np.array_equal(r.yhat.view(np.int64), yhat.view(np.int64))
    assert np.array_equal(r.yhat_lower.view(np.int64), lo.view(np.int64))
    assert np.array_equal(r.yhat_upper.view(np.int64), hi.view(np.int64))
    # the sampled trend: the same draws with beta = 0 and sigma = exp(-800) = 0 -- every sample is its trend
    _, tlo, thi = fc.predict_intervals(c.spec, _beta0(c, -800.0), c.y_scale, c.grid, c.fut, floor=c.floor, cap=c.cap,
                                       extra_future=c.extra, series_key=keys, uncertainty_samples=n_samples,
                                       interval_width=width, seed=17)
    assert np.array_equal(r.trend_lower, tlo) and np.array_equal(r.trend_upper, thi)
    assert (r.trend_lower <= r.trend_upper).all()
    # the point outputs do not depend on the intervals
    p = _components(fc, c, cols)
    for k in ('yhat', 'trend', 'comp'):
        assert np.array_equal(getattr(p, k).view(np.int64), getattr(r, k).view(np.int64)), k
    return r


@pytest.mark.parametrize('name,n_samples,width', [
    ('iv65', 2, 0.01), ('iv65', 1000, 0.8), ('iv65', 4096, 0.99),
    ('iv129', 3, 0.01), ('iv129', 1000, 0.99), ('iv129', 4096, 0.8)])
def test_intervals_on_the_shape_subset(env, name, n_samples, width):
    fc, _lib = env
    c = fcs.make(name)
    _check_intervals(fc, c, _table(fc, c), np.arange(c.N, dtype=np.int64) * 7919 + 3, n_samples, width)


def test_intervals_over_several_chunks(env):
    """300 series x 960 steps x 1000 samples: 16 MB of scratch per series, so the call runs 9 chunks (34 series each)
    against tsf_predict_intervals' 5"""
    fc, _lib = env
    c = fcs.make('h960')
    rng = np.random.default_rng(9)
    rep = 100
    c.N = c.N * rep
    ncp = c.spec.n_changepoints
    c.theta = np.tile(c.theta, (rep, 1))
    c.theta[:, 3 + ncp:] *= rng.uniform(0.5, 1.5, (c.N, 1))
    c.theta[:, 2] += rng.normal(0, 0.3, c.N)
    c.y_scale = np.tile(c.y_scale, rep) * rng.uniform(0.5, 2.0, c.N)
    c.floor = np.tile(c.floor, rep)
    assert c.N == 300 and c.H == 960
    _check_intervals(fc, c, _table(fc, c)[:4], np.arange(c.N, dtype=np.int64) ^ 0x5555, 1000, 0.8)


def test_argument_checks(env):
    """each of these is refused (< 0, a message) before anything is launched, and the context stays usable"""
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    c = fcs.make('h1')
    N, H = c.N, c.H
    cs = c.spec.to_c()
    theta, ys = np.ascontiguousarray(c.theta), np.ascontiguousarray(c.y_scale)
    fut = np.ascontiguousarray(c.fut, dtype=np.int64)
    out = [np.zeros((N, H)) for _ in range(6)]
    comp = np.zeros((N, _lib.MAX_COMP + 1, H))

    def call(n_comp, masks, n_samples, grid=c.grid, iv=out[2:]):
        masks = np.ascontiguousarray(masks, dtype=np.uint64)
        scaled = np.ones(len(masks), dtype=np.int32)
        grid = np.ascontiguousarray(grid)
        return L.tsf_predict_components(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, ys.ctypes.data,
                                        grid.ctypes.data, len(grid), fut.ctypes.data, 1, None, None, None, n_comp,
                                        masks.ctypes.data, scaled.ctypes.data, None, n_samples, 0.8, 0,
                                        out[0].ctypes.data, out[1].ctypes.data, comp.ctypes.data,
                                        *[None if a is None else a.ctypes.data for a in iv])

    K = c.K
    ok = np.array([1, (1 << K) - 1], dtype=np.uint64)
    assert call(2, ok, 0) == 0 and call(2, ok, 10) == 0
    bad_grid = c.grid.copy()
    bad_grid['S'][1] = -1
    for rc_args, why in (((_lib.MAX_COMP + 1, np.ones(_lib.MAX_COMP + 1), 0), 'n_comp'),
                         ((-1, ok, 0), 'n_comp'),
                         ((2, [1, 1 << K], 0), 'comp_cols\\[1\\]'),
                         ((1, [1 << 63], 0), 'comp_cols\\[0\\]'),
                         ((2, ok, 1), 'n_samples'),
                         ((2, ok, 10, c.grid, [out[2], out[3], None, out[5]]), 'NULL interval'),
                         ((2, ok, 0, bad_grid), r'grid\[1\]')):
        rc = call(*rc_args)
        assert rc < 0, why
        assert re.search(why, L.tsf_last_error(ctx.handle).decode()), (why, L.tsf_last_error(ctx.handle))
    with pytest.raises(_lib.TsfError, match='comp_cols'):
        fc.predict_components(c.spec, c.theta, c.y_scale, c.grid, c.fut, columns=[('x', 1 << K, 0)])
    r = fc.predict_components(c.spec, c.theta, c.y_scale, c.grid, c.fut, floor=c.floor)
    assert np.array_equal(r.yhat, fc.predict(c.spec, c.theta, c.y_scale, c.grid, c.fut, floor=c.floor))


def _two_bucket_models(fc):
    """a model frame of two spec buckets: logistic / multiplicative with holidays (weekly only), linear / additive
    without (yearly + weekly)"""
    from time_series_spark_amd import synth
    from time_series_spark_amd.jobs import prophet_modeler as pm
    ds, y = synth.make_panel(3, 400, 'logistic', seed=12)
    days = pd.to_datetime(ds)
    hol = pd.DataFrame({'holiday': ['a'] * 3 + ['b'] * 2,
                        'ds': [days[40], days[200], days[-1] + pd.Timedelta(days=10), days[120], days[390]],
                        'lower_window': [-1] * 3 + [0] * 2, 'upper_window': [1] * 3 + [2] * 2})
    df = pd.concat([pd.DataFrame({'series_id': 7, 'dim_id': n, 'ds': days, 'y': y[n]}) for n in range(3)],
                   ignore_index=True)
    cfg_a = {'model': {'floor': 0, 'cap_multiplier': 1.1,
                       'prophet': {'holidays': hol, 'yearly_seasonality': False, 'growth': 'logistic',
                                   'seasonality_mode': 'multiplicative'}}}
    ma = pm.model_panel(cfg_a)(df)
    ds2, y2 = synth.make_panel(2, 800, 'linear', seed=4)
    df2 = pd.concat([pd.DataFrame({'series_id': 8, 'dim_id': n, 'ds': pd.to_datetime(ds2), 'y': y2[n]})
                     for n in range(2)], ignore_index=True)
    mb = pm.model_panel({'model': {'floor': 0, 'cap_multiplier': 1.1, 'prophet': {'growth': 'linear', 'seasonality_mode': 'additive'}}})(df2)
    return pd.concat([ma, mb], ignore_index=True)


def _by_hand(fc, models, H, fcfg):
    """fc.predict_components per bucket on the model blobs, as a user would call it: {(series_id, dim_id): Components
    row}"""
    from time_series_spark_amd import features, panel as pk
    out = {}
    blobs = models['model'].tolist()
    sids, dids = models['series_id'].to_numpy(), models['dim_id'].to_numpy()
    for spec_dict, idx, rec in pk.load_models(blobs):
        spec = fc.ModelSpec.from_dict(spec_dict)
        theta = np.zeros((len(idx), spec.theta_stride))
        theta[:, :rec['theta'].shape[1]] = rec['theta']
        fut = pk.future_dates(rec['last_ds_ns'], H, 'D')
        ex = None
        if spec.extra:
            ex = np.zeros((len(idx), len(spec.extra), H))
            names, _, days = features.holiday_columns(features.normalize_holidays(spec.holidays))
            ex[:, :len(names), :] = np.moveaxis(features.holiday_matrix(fut, days), 0, 1)
        key = (sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff)
        r = fc.predict_components(spec, theta, rec['y_scale'], pk.grid_from_records(rec), fut,
                                  floor=models['floor'].to_numpy(np.float64)[idx],
                                  cap=models['cap'].to_numpy(np.float64)[idx], extra_future=ex,
                                  intervals=bool(fcfg.get('intervals')), series_key=key,
                                  uncertainty_samples=fcfg.get('uncertainty_samples', 1000), seed=fcfg.get('seed', 0))
        for j, i in enumerate(idx):
            out[(int(sids[i]), int(dids[i]))] = (r, j)
    return out


def test_scorer_components(env):
    fc, _lib = env
    from time_series_spark_amd.jobs import prophet_scorer as ps
    H = 30
    models = _two_bucket_models(fc)
    base = {'forecast': {'periods': H, 'frequency': 'D'}}
    plain = ps.forecast_panel(base)(models)
    for intervals in (False, True):
        fcfg = dict(base['forecast'], components=True, intervals=intervals, uncertainty_samples=300, seed=1)
        got = ps.forecast_panel({'forecast': fcfg})(models)
        assert np.array_equal(got['yhat'].values, plain['yhat'].values) and got['yhat'].dtype == plain['yhat'].dtype
        assert np.array_equal(got['ds'].values, plain['ds'].values)
        hand = _by_hand(fc, models, H, fcfg)
        names = sorted(set().union(*[r.names for r, _ in hand.values()]))
        assert {'holidays', 'a', 'b', 'weekly', 'yearly', 'additive_terms', 'multiplicative_terms'} <= set(names)
        want_cols = (['series_id', 'dim_id', 'ds', 'yhat'] + (['yhat_lower', 'yhat_upper'] if intervals else [])
                     + ['trend'] + (['trend_lower', 'trend_upper'] if intervals else []) + names)
        assert list(got.columns) == want_cols
        for col in want_cols[4:]:
            assert got[col].dtype == np.float64
        absent = 0
        for (sid, did), (r, j) in hand.items():
            rows = got[(got['series_id'] == sid) & (got['dim_id'] == did)]
            assert len(rows) == H
            assert np.array_equal(rows['trend'].values, r.trend[j])
            for name in names:
                if name in r.terms:
                    assert np.array_equal(rows[name].values, r.terms[name][j]), name
                else:
                    assert (rows[name].values == 0.0).all(), name
                    absent += 1
            if intervals:
                for k in ('yhat_lower', 'yhat_upper', 'trend_lower', 'trend_upper'):
                    assert np.array_equal(rows[k].values, getattr(r, k)[j]), k
        assert absent > 0
    # with intervals alone the frame is what it was
    fi = ps.forecast_panel({'forecast': dict(base['forecast'], intervals=True)})(models)
    assert list(fi.columns) == ['series_id', 'dim_id', 'ds', 'yhat', 'yhat_lower', 'yhat_upper']


def test_abi_components_plain_c(env, tmp_path):
    """tests/c/abi_components.c drives tsf_predict_components from plain C99 and writes what it returns"""
    fc, _lib = env
    c = fcs.make('iv129')
    d = str(tmp_path)
    np.ascontiguousarray(c.theta).tofile(d + '/theta.f64')
    np.ascontiguousarray(c.y_scale).tofile(d + '/ys.f64')
    np.ascontiguousarray(c.grid).tofile(d + '/grid.bin')
    np.ascontiguousarray(c.fut, dtype=np.int64).tofile(d + '/fut.i64')
    np.ascontiguousarray(c.extra).tofile(d + '/extra.f64')
    exe = d + '/abi_components'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_components.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(c.N), str(c.H), d])
    got = np.fromfile(d + '/out.f64')
    cols = fc.component_columns(c.spec)
    r = fc.predict_components(c.spec, c.theta, c.y_scale, c.grid, c.fut, extra_future=c.extra,
                              intervals=True, uncertainty_samples=200, seed=5)
    assert [n for n, _, _ in cols][:3] == ['additive_terms', 'extra_regressors_additive', 'extra_regressors_multiplicative']
    want = np.concatenate([r.yhat.ravel(), r.trend.ravel(), r.comp[:, :3, :].ravel(), r.yhat_lower.ravel(),
                           r.yhat_upper.ravel(), r.trend_lower.ravel(), r.trend_upper.ravel()])
    assert helpers.n_bit_diff(got, want) == 0
