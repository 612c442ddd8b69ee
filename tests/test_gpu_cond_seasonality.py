"""GPU tests of conditional seasonalities (fbprophet's add_seasonality(condition_name=...); include/tsf.h "conditional
seasonalities"): run with `-m gpu` on an MI355X.  The columns enter at one place -- tsf_cond_columns, through
fc.conditional_extra -- as explicit design columns; every fit and forecast entry then reads `extra`.  So: the columns
are the canonical oracle's unconditional columns bit for bit where the condition holds and +0.0 elsewhere, in every
layout; fits and forecasts on them are the oracle's on the same columns; the model does what the argument promises;
components, cross-validation, the jobs and a plain C caller follow.  Parity is with the restated oracle, not with
fbprophet itself (unpinned: include/tsf.h).  The CPU side: tests/test_cond_spec.py."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
# at collection, before anything loads libtsf_amd.so (as in bench.py): a torch wheel carries a HIP runtime of its own,
# and the library binds to the runtime that is loaded first
import torch

from tests import cond_ref, helpers

pytestmark = pytest.mark.gpu
DAY = 86400 * 10 ** 9
HOUR = 3600 * 10 ** 9
REL_TOL = 1e-4          # BASELINE.json north_star (tests/test_gpu_parity.py)
FIT_KEYS = ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval')
W7 = {'name': 'w_in', 'period': 7, 'fourier_order': 3, 'condition_name': 'a'}
D1 = {'name': 'd_b', 'period': 1, 'fourier_order': 4, 'condition_name': 'b'}
WEEKLY_IN = {'name': 'weekly_in', 'period': 7, 'fourier_order': 3, 'condition_name': 'in_season'}
WEEKLY_OFF = {'name': 'weekly_off', 'period': 7, 'fourier_order': 3, 'condition_name': 'off_season'}


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU tests cannot run (product has no CPU fallback)')
    return forecaster, _lib


def stamps(rows, step):
    """rows ascending timestamps `step` apart from 2019-03-01 05:00, the first one replaced by a stamp before 1970"""
    ds = np.datetime64('2019-03-01T05:00', 'ns').astype(np.int64) + step * np.arange(rows, dtype=np.int64)
    ds[0] = -(400 * DAY + 7 * HOUR + 1234567)
    return ds


def masks(rows):
    i = np.arange(rows)
    return (i // 5) % 2 == 0, (i * 7) % 3 != 0


def expected_columns(ds, a, b):
    return np.concatenate([cond_ref.canonical_columns(ds, 7, 3, a), cond_ref.canonical_columns(ds, 1, 4, b)])


def same_bits(x, w):
    return x.shape == w.shape and helpers.n_bit_diff(x, w) == 0


def cond_struct(_lib):
    cs = _lib.TsfCondSeas()
    cs.n = 2
    cs.period[0], cs.order[0], cs.cond[0] = 7.0, 3, 0
    cs.period[1], cs.order[1], cs.cond[1] = 1.0, 4, 1
    return cs


# ---- 1. the columns, bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize('step', [HOUR, DAY], ids=['hourly', 'daily'])
@pytest.mark.parametrize('rows', [1, 63, 65, 257, 730])
def test_columns_are_the_oracles_where_the_condition_holds(env, rows, step):
    """Two conditional seasonalities (period 7 order 3, period 1 order 4) on two different masks: the canonical oracle's
    unconditional columns where the mask is true, +0.0 (sign bit clear) where it is false; a sub-range of ds gives the
    sub-range of the columns (nothing depends on the panel's start or on `rows`); a stride above the rows leaves what
    lies behind the rows untouched."""
    fc, _lib = env
    spec = fc.ModelSpec(seasonalities=[dict(W7), dict(D1)])
    ds = stamps(rows, step)
    a, b = masks(rows)
    want = expected_columns(ds, a, b)
    got = fc.conditional_extra(spec, ds, conditions={'a': a, 'b': b})
    assert got.shape == (14, rows) and same_bits(got, want)
    off = np.concatenate([np.repeat(~a[None, :], 6, axis=0), np.repeat(~b[None, :], 8, axis=0)])
    assert (got[off] == 0).all() and not np.signbit(got[off]).any()
    if rows > 2:
        assert np.abs(got[~off]).max() > 0.5
        lo, hi = rows // 3, rows - 1
        sub = fc.conditional_extra(spec, ds[lo:hi], conditions={'a': a[lo:hi], 'b': b[lo:hi]})
        assert same_bits(sub, got[:, lo:hi])
    # written into a larger block at its stride: two leading rows and 5 doubles behind every row keep their marker
    stride = rows + 5
    block = np.full((16, stride), -12345.0)
    cond = np.ascontiguousarray(np.stack([a, b]).astype(np.uint8))
    ctx = fc.get_context()
    cs = cond_struct(_lib)
    ctx.check(_lib.load().tsf_cond_columns(ctx.handle, ctypes.byref(cs), rows, ds.ctypes.data, 2, cond.ctypes.data,
                                           block[2:].ctypes.data, stride))
    assert same_bits(block[2:, :rows], want)
    assert (block[:2] == -12345.0).all() and (block[:, rows:] == -12345.0).all()


def test_host_and_device_entries_agree(env):
    """tsf_cond_columns_dev on device tensors, a stream that is not the default one and a stride above the rows: the
    host entry's bits, the padding untouched; the refused calls return < 0 with a text and leave the context usable"""
    fc, _lib = env
    L, ctx = _lib.load(), fc.get_context()
    rows, stride = 257, 264
    ds = stamps(rows, HOUR)
    a, b = masks(rows)
    cond = np.ascontiguousarray(np.stack([a, b]).astype(np.uint8))
    cs = cond_struct(_lib)
    host = np.zeros((14, rows))
    ctx.check(L.tsf_cond_columns(ctx.handle, ctypes.byref(cs), rows, ds.ctypes.data, 2, cond.ctypes.data, host.ctypes.data, rows))
    d_ds, d_cond = torch.from_numpy(ds).cuda(), torch.from_numpy(cond).cuda()
    d_out = torch.full((14, stride), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    ctx.check(L.tsf_cond_columns_dev(ctx.handle, ctypes.byref(cs), rows, d_ds.data_ptr(), 2, d_cond.data_ptr(),
                                     d_out.data_ptr(), stride, ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    dev = d_out.cpu().numpy()
    assert same_bits(np.ascontiguousarray(dev[:, :rows]), host) and np.isnan(dev[:, rows:]).all()
    assert same_bits(host, expected_columns(ds, a, b))
    # misuse: before any launch, with a message; then the context still works
    def refused(text, cs_=cs, rows_=rows, n_cond=2, stride_=rows):
        rc = L.tsf_cond_columns(ctx.handle, ctypes.byref(cs_), rows_, ds.ctypes.data, n_cond, cond.ctypes.data,
                                host.ctypes.data, stride_)
        assert rc < 0 and text in L.tsf_last_error(ctx.handle).decode(), (text, rc, L.tsf_last_error(ctx.handle))
    refused('col_stride', stride_=rows - 1)
    for field, value, text in (('n', 0, 'tsf_cond_seas.n'), ('n', 9, 'tsf_cond_seas.n')):
        bad = cond_struct(_lib)
        setattr(bad, field, value)
        refused(text, cs_=bad)
    for field, i, value, text in (('period', 0, float('inf'), 'period[0]'), ('period', 1, -1.0, 'period[1]'),
                                  ('order', 1, 0, 'order[1]'), ('cond', 0, 2, 'cond[0]'), ('cond', 1, -1, 'cond[1]')):
        bad = cond_struct(_lib)
        getattr(bad, field)[i] = value
        refused(text, cs_=bad)
    bad = cond_struct(_lib)
    bad.order[0], bad.order[1] = 20, 13
    refused('TSF_MAX_EXTRA', cs_=bad)
    again = np.zeros((14, rows))
    ctx.check(L.tsf_cond_columns(ctx.handle, ctypes.byref(cs), 0, None, 2, None, None, 0))           # rows = 0: a no-op
    ctx.check(L.tsf_cond_columns(ctx.handle, ctypes.byref(cs), rows, ds.ctypes.data, 2, cond.ctypes.data, again.ctypes.data, rows))
    assert same_bits(again, host)


def test_ragged_and_per_series_layouts_equal_the_flat_call(env):
    """The caller's columns in front, the conditional ones behind, in the three layouts the entry points take"""
    fc, _lib = env
    spec = fc.ModelSpec(seasonalities=[dict(helpers.WEEKLY), dict(W7), dict(D1)], extra=[{'name': 'u0'}, {'name': 'u1'}])
    assert spec.n_user_extra == 2 and len(spec.extra) == 16
    N, H = 3, 65
    ds = np.stack([stamps(H, HOUR) + n * 13 * HOUR for n in range(N)])
    a = np.stack([np.roll(masks(H)[0], n) for n in range(N)])
    b = np.stack([np.roll(masks(H)[1], 2 * n) for n in range(N)])
    user = np.arange(N * 2 * H, dtype=np.float64).reshape(N, 2, H)
    flat = fc.conditional_extra(spec, ds.reshape(-1), conditions={'a': a.reshape(-1), 'b': b.reshape(-1)},
                                extra=np.ascontiguousarray(user.transpose(1, 0, 2)).reshape(2, N * H))
    assert flat.shape == (16, N * H)
    assert same_bits(flat[2:], expected_columns(ds.reshape(-1), a.reshape(-1), b.reshape(-1)))
    assert np.array_equal(flat[:2].reshape(2, N, H).transpose(1, 0, 2), user)
    off = np.arange(N + 1, dtype=np.int64) * H
    ragged = fc.conditional_extra(spec, ds.reshape(-1), conditions={'a': a.reshape(-1), 'b': b.reshape(-1)},
                                  extra=flat[:2], offsets=off)
    assert same_bits(ragged, flat)
    per = fc.conditional_extra(spec, ds, conditions={'a': a, 'b': b}, extra=user)
    assert per.shape == (N, 16, H) and same_bits(per, np.ascontiguousarray(flat.reshape(16, N, H).transpose(1, 0, 2)))
    with pytest.raises(ValueError):
        fc.conditional_extra(spec, ds.reshape(-1), conditions={'a': a.reshape(-1), 'b': b.reshape(-1)}, extra=flat[:2],
                             offsets=off[:-1])
    with pytest.raises(ValueError):
        fc.conditional_extra(spec, ds, conditions={'a': a, 'b': b}, extra=flat[:2])


# ---- 2. fit and forecast through the existing oracle ----------------------------------------------------------------

def season_rules(ds, in_season):
    """the in-season blocks of cond_ref.season_flip_panel as a `ranges` rule, and its negation"""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], in_season.astype(np.int8), [0]])))
    ranges = [[str(np.datetime64(int(ds[0]) + int(s) * DAY, 'ns')), str(np.datetime64(int(ds[0]) + int(e) * DAY, 'ns'))]
              for s, e in zip(edges[::2], edges[1::2])]
    return {'in_season': {'ranges': ranges}, 'off_season': {'ranges': ranges, 'negate': True}}


@pytest.mark.parametrize('growth,mode', [('linear', 'additive'), ('logistic', 'multiplicative')])
def test_fit_and_forecast_against_the_oracle(env, growth, mode):
    """N = 3, T = 210: linear growth with an additive in / off-season weekly pair (the quadratic form) and logistic
    growth with multiplicative columns (the residual form).  fit_aligned + predict with `extra` from conditional_extra
    against the live canonical oracle on the same columns: theta, status, n_iter, n_eval and fval without one differing
    bit, yhat within the north-star tolerance -- the comparison test_fit_predict_against_oracle_and_golden makes."""
    fc, _lib = env
    from oracle import canon_lib as cl
    ds, y, in_season = cond_ref.season_flip_panel(3, 210)
    N, T, H = 3, 210, 30
    spec = fc.ModelSpec(growth=growth, seasonality_mode=mode, seasonalities=[dict(WEEKLY_IN), dict(WEEKLY_OFF)],
                        conditions=season_rules(ds, in_season))
    assert helpers.uses_quadratic_form(spec) == (growth == 'linear')
    floor, cap = np.zeros(N), y.max(axis=1) * 1.1
    fut = ds[-1] + DAY * np.arange(1, H + 1)
    # the arrays win where given; the rules say the same on these dates
    ex = fc.conditional_extra(spec, ds, conditions={'in_season': in_season, 'off_season': ~in_season})
    assert same_bits(ex, fc.conditional_extra(spec, ds))
    assert same_bits(ex, np.concatenate([cond_ref.canonical_columns(ds, 7, 3, in_season),
                                         cond_ref.canonical_columns(ds, 7, 3, ~in_season)]))
    exf = fc.conditional_extra(spec, fut)
    assert exf.shape == (12, H) and (exf[:6] == 0).all() and np.abs(exf[6:]).max() > 0.5      # (the rule's ranges end with the history)
    r = fc.fit_aligned(spec, ds, y, floor=floor, cap=cap, extra=ex)
    yhat = fc.predict(spec, r.theta, r.y_scale, r.grid, fut, floor=floor, cap=cap, extra_future=exf)
    assert (r.status > 0).all()
    csp = helpers.oracle_spec(spec)
    for n in range(N):
        o = cl.fit(csp, ds, y[n], floor[n], cap[n], ex)
        yo, _ = cl.predict(csp, o, fut, floor[n], cap[n], exf)
        assert (r.status[n], r.n_iter[n], r.n_eval[n]) == (o['status'], o['n_iter'], o['n_eval']), n
        assert helpers.n_bit_diff(r.theta[n][:len(o['theta'])], o['theta']) == 0, n
        assert helpers.n_bit_diff(r.fval[n], o['f']) == 0, n
        assert np.max(np.abs(yhat[n] - yo) / np.abs(yo)) <= REL_TOL, n


# ---- 3. it models what it says --------------------------------------------------------------------------------------

def test_the_pair_fits_a_pattern_that_flips_with_the_season(env):
    """Series whose weekly pattern flips sign between season and off-season: for every series the in-sample SSE of the
    in / off-season pair is strictly below that of one weekly seasonality of the same order (the oracle alone shows the
    same on these inputs: tests/test_cond_spec.py)."""
    fc, _lib = env
    ds, y, in_season = cond_ref.season_flip_panel(3, 210)
    pair = fc.ModelSpec(growth='linear', seasonalities=[dict(WEEKLY_IN), dict(WEEKLY_OFF)])
    plain = fc.ModelSpec(growth='linear', seasonalities=[dict(helpers.WEEKLY)])
    ex = fc.conditional_extra(pair, ds, conditions={'in_season': in_season, 'off_season': ~in_season})
    rp = fc.fit_aligned(pair, ds, y, extra=ex)
    rw = fc.fit_aligned(plain, ds, y)
    assert (rp.status > 0).all() and (rw.status > 0).all()
    sse_p = ((fc.predict(pair, rp.theta, rp.y_scale, rp.grid, ds, extra_future=ex) - y) ** 2).sum(axis=1)
    sse_w = ((fc.predict(plain, rw.theta, rw.y_scale, rw.grid, ds) - y) ** 2).sum(axis=1)
    print('SSE pair', sse_p, 'SSE plain weekly', sse_w)
    assert (sse_p < sse_w).all()


# ---- 4. components --------------------------------------------------------------------------------------------------

def test_components_name_the_conditional_seasonality(env):
    fc, _lib = env
    ds, y, in_season = cond_ref.season_flip_panel(3, 210)
    spec = fc.ModelSpec(growth='linear', seasonalities=[dict(WEEKLY_IN), dict(WEEKLY_OFF)],
                        conditions=season_rules(ds, in_season))
    ex = fc.conditional_extra(spec, ds)
    r = fc.fit_aligned(spec, ds, y, extra=ex)
    # history rows and future rows in one forecast: both conditions occur
    at = np.concatenate([ds[20:90], ds[-1] + DAY * np.arange(1, 31)])
    on = np.concatenate([in_season[20:90], np.zeros(30, dtype=bool)])
    exf = fc.conditional_extra(spec, at)
    c = fc.predict_components(spec, r.theta, r.y_scale, r.grid, at, extra_future=exf)
    assert c.names == ['additive_terms', 'weekly_in', 'weekly_off', 'multiplicative_terms']
    assert on.any() and not on.all()
    win, woff = c.terms['weekly_in'], c.terms['weekly_off']
    assert (win[:, ~on] == 0.0).all() and (woff[:, on] == 0.0).all()
    assert np.abs(win[:, on]).max() > 1.0 and np.abs(woff[:, ~on]).max() > 1.0
    assert helpers.n_bit_diff(c.yhat, fc.predict(spec, r.theta, r.y_scale, r.grid, at, extra_future=exf)) == 0
    # additive_terms carries both (the same products summed in another order: a few ulp of the largest term)
    tol = 64 * 2.220446049250313e-16 * max(np.abs(win).max(), np.abs(woff).max())
    assert np.abs(c.terms['additive_terms'] - (win + woff)).max() <= tol
    assert (c.terms['multiplicative_terms'] == 0).all()
    cols = list(c.frame(0, at).columns)
    assert 'weekly_in' in cols and 'weekly_off_upper' in cols and not any(k.startswith('extra_regressors') for k in cols)
    assert not any('_delim_' in k for k in cols)


# ---- 5. cross-validation follows -------------------------------------------------------------------------------------

def test_cross_validation_folds_are_fits_on_the_cut_prefix(env):
    """Fold c of cross_validate with the helper's columns = fit_ragged on the explicitly cut prefix with columns built
    for the prefix's ds alone, bit for bit; and its holdout forecast = predict with columns built for the holdout rows."""
    fc, _lib = env
    ds, y, in_season = cond_ref.season_flip_panel(3, 210)
    spec = fc.ModelSpec(growth='linear', seasonalities=[dict(WEEKLY_IN), dict(WEEKLY_OFF)],
                        conditions=season_rules(ds, in_season))
    ex = fc.conditional_extra(spec, ds)
    cv = fc.cross_validate(spec, ds, y, 30 * DAY, extra=ex)
    F = len(cv.cutoff)
    assert list(cv.n_folds) == [F // 3] * 3 and F >= 9 and (cv.status == 0).all()
    hist = cv.hist_rows.astype(np.int64)
    off = np.concatenate([[0], np.cumsum(hist)]).astype(np.int64)
    ds_r = np.concatenate([ds[:h] for h in hist])
    y_r = np.concatenate([y[int(n)][:h] for n, h in zip(cv.fold_series, hist)])
    ex_r = fc.conditional_extra(spec, ds_r, offsets=off)                   # built from the prefixes' own timestamps
    assert same_bits(ex_r, np.concatenate([ex[:, :h] for h in hist], axis=1))
    r = fc.fit_ragged(spec, off, ds_r, y_r, extra=ex_r)
    for k in FIT_KEYS:
        x, w = getattr(cv.fit, k), getattr(r, k)
        assert (helpers.n_bit_diff(x, w) == 0) if x.dtype.kind == 'f' else np.array_equal(x, w), k
    assert cv.fit.grid.tobytes() == r.grid.tobytes()
    ro = np.concatenate([[0], np.cumsum(cv.hold_rows)]).astype(np.int64)
    for f in range(F):
        h, hd = int(hist[f]), int(cv.hold_rows[f])
        fut = ds[h:h + hd]
        yh = fc.predict(spec, r.theta[f:f + 1], r.y_scale[f:f + 1], r.grid[f:f + 1], fut,
                        extra_future=fc.conditional_extra(spec, fut))
        assert helpers.n_bit_diff(cv.yhat[ro[f]:ro[f + 1]], yh[0]) == 0, f


# ---- 6. jobs ----------------------------------------------------------------------------------------------------------

def _write_input(tmp_path, ds, y):
    text = pd.DatetimeIndex(ds.astype('datetime64[ns]')).strftime('%Y-%m-%d %H:%M:%S').values
    for n in range(len(y)):
        d = tmp_path / 'in' / ('series_id=%d' % (7 + n))
        d.mkdir(parents=True)
        (d / 'part-0.csv').write_text('\n'.join('1,%s,%d' % (s, v) for s, v in zip(text, y[n])) + '\n')


def test_modeler_and_scorer_with_a_conditions_rule(env, tmp_path):
    """Modeler -> blob -> scorer with a conditional pair under model.prophet.seasonalities and date rules under
    model.prophet.conditions: the blob carries the original form and the rules; the models are fit_aligned's on the
    helper's columns; the forecast is predict's with helper-built future columns.  The in-season seasonality is called
    'weekly': it switches the automatic weekly off, as any user seasonality of that name does.  The same configuration
    without condition_name: the blobs of the plain model, byte for byte, and no new key in them."""
    fc, _lib = env
    from time_series_spark_amd import panel as pk
    from time_series_spark_amd.jobs import prophet_modeler as pm, prophet_scorer as ps
    N, T, H = 4, 210, 30
    ds, y, in_season = cond_ref.season_flip_panel(N, T)
    y = np.trunc(y)
    _write_input(tmp_path, ds, y)
    rules = season_rules(ds, in_season)
    seas = [dict(WEEKLY_IN, name='weekly'), dict(WEEKLY_OFF)]
    prophet = {'growth': 'linear', 'seasonality_mode': 'additive', 'seasonalities': seas, 'conditions': rules}
    mcfg = {'io': {'input': str(tmp_path / 'in'), 'models': str(tmp_path / 'models')},
            'model': {'floor': 0, 'cap_multiplier': 1.1, 'prophet': prophet}}
    frame = pm.ProphetModeler.model(None, mcfg).sort_values(['series_id', 'dim_id']).reset_index(drop=True)
    assert len(frame) == N
    (sd, pos, rec), = pk.load_models(list(frame['model']))
    assert sd['seasonalities'] == seas and sd['extra'] == [] and sd['conditions'] == rules
    spec = fc.ModelSpec.from_dict(sd)
    assert spec.seasonalities == [] and [e['seasonality'] for e in spec.extra] == ['weekly'] * 6 + ['weekly_off'] * 6
    ex = fc.conditional_extra(spec, ds)
    assert same_bits(ex, np.concatenate([cond_ref.canonical_columns(ds, 7, 3, in_season),
                                         cond_ref.canonical_columns(ds, 7, 3, ~in_season)]))
    lb = fc.ModelSpec.from_dict(dict(sd, lbfgs=dict(sd['lbfgs'], algorithm=_lib.ALGO_LBFGS)))
    r = fc.fit_aligned(lb, ds, y, floor=np.zeros(N), extra=ex)
    assert (r.status > 0).all()                                           # (no Newton retry to follow by hand)
    assert helpers.n_bit_diff(rec['theta'][np.argsort(pos)], r.theta) == 0
    ps.ProphetScorer.score(None, {'io': {'models': mcfg['io']['models'], 'forecasts': str(tmp_path / 'fc')},
                                  'forecast': {'periods': H, 'frequency': 'D'}})
    back = pd.concat([pd.read_csv(f) for f in glob.glob(str(tmp_path / 'fc' / '*.csv'))])
    back = back.sort_values(['series_id', 'dim_id', 'forecast_timestamp'], kind='stable')
    fut = ds[-1] + DAY * np.arange(1, H + 1)
    cap = (y.max(axis=1) * 1.1).astype(np.float32).astype(np.float64)
    yhat, yint = fc.predict(spec, r.theta, r.y_scale, r.grid, fut, floor=np.zeros(N), cap=cap,
                            extra_future=fc.conditional_extra(spec, fut), want_int=True)
    assert np.array_equal(back['forecast_quantity'].to_numpy().reshape(N, H), yint)
    # a condition_name without a rule: refused when the configuration is read, before any fit
    with pytest.raises(ValueError) as e:
        pm.ProphetModeler.model(None, dict(mcfg, model=dict(mcfg['model'], prophet=dict(prophet, conditions={}))))
    assert 'has no rule under model.prophet.conditions' in str(e.value)
    # without condition_name: two plain seasonalities, the blobs those of the plain model
    plain = [{k: v for k, v in s.items() if k != 'condition_name'} for s in seas]
    pcfg = dict(mcfg, io=dict(mcfg['io'], models=str(tmp_path / 'plain')),
                model=dict(mcfg['model'], prophet={'growth': 'linear', 'seasonality_mode': 'additive', 'seasonalities': plain}))
    pframe = pm.ProphetModeler.model(None, pcfg).sort_values(['series_id', 'dim_id']).reset_index(drop=True)
    (psd, ppos, prec), = pk.load_models(list(pframe['model']))
    assert set(psd) == {'growth', 'seasonality_mode', 'n_changepoints', 'changepoint_range', 'changepoint_prior_scale',
                        'seasonality_prior_scale', 'holidays_prior_scale', 'seasonalities', 'extra', 'lbfgs'}
    assert psd['seasonalities'] == plain and psd['extra'] == []
    pspec = fc.ModelSpec(growth='linear', seasonality_mode='additive', seasonalities=plain)
    rp = fc.fit_aligned(fc.ModelSpec(growth='linear', seasonality_mode='additive', seasonalities=plain,
                                     algorithm=_lib.ALGO_LBFGS), ds, y, floor=np.zeros(N))
    assert (rp.status > 0).all()
    want = pk.dump_models_buffer(pspec.to_dict(), rp.theta, rp.y_scale, rp.grid, np.full(N, ds[-1]), rp.status, rp.n_iter)
    assert [bytes(b) for b in pframe['model']] == [want[n].tobytes() for n in range(N)]


# ---- 7. C ABI -----------------------------------------------------------------------------------------------------

def test_c_program_matches_the_python_binding(env, tmp_path):
    """A plain C99 program (tests/c/abi_cond.c) builds the 14 columns into a larger block at its stride: the bytes of
    the ctypes binding's call, the rest of the block untouched; every misuse is refused with a text."""
    fc, _lib = env
    exe = str(tmp_path / 'abi_cond')
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror',
                           '-I', os.path.join(helpers.ROOT, 'include'),
                           os.path.join(helpers.ROOT, 'tests', 'c', 'abi_cond.c'),
                           '-o', exe, '-L', libdir, '-ltsf_amd', '-Wl,-rpath,' + libdir])
    rows = 257
    ds = stamps(rows, HOUR)
    a, b = masks(rows)
    ds.astype('<i8').tofile(tmp_path / 'ds.i64')
    np.stack([a, b]).astype(np.uint8).tofile(tmp_path / 'cond.u8')
    msg = subprocess.check_output([exe, str(rows), str(tmp_path)]).decode()
    for what in ('stride', 'count0', 'count9', 'period', 'order', 'columns', 'index'):
        assert ('%s: rc=-' % what) in msg, msg
    block = np.fromfile(tmp_path / 'out.f64', dtype='<f8').reshape(16, rows + 5)
    spec = fc.ModelSpec(seasonalities=[dict(W7), dict(D1)])
    got = fc.conditional_extra(spec, ds, conditions={'a': a, 'b': b})
    assert np.ascontiguousarray(block[2:, :rows]).tobytes() == got.tobytes()
    assert (block[:2] == -12345.0).all() and (block[:, rows:] == -12345.0).all()
