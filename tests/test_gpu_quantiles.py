"""GPU tests of the forecast quantiles, cumulative quantiles and predictive samples (tsf_predict_quantiles:
interval_sample_kernel's running-sum output, quantile_kernel, the chunk-by-chunk copy of the raw draws).

What pins them (include/tsf.h, the contract of the quantile section):
  the raw draws against oracle cn_predict_intervals -- with 2^k + 1 samples and width 1 - 2j / 2^k its lower / upper are
  the order statistics v[j] / v[2^k - j] with no interpolation, so 33 oracle calls reconstruct a row's 65 sorted values,
  and its calls with 1, 2 and 3 samples give samples 0, 1 and 2 themselves;
  the quantiles against the numpy evaluation of the contract's expression on the returned draws, bit for bit (sorting
  is exact, the expression is three roundings in a fixed order);
  the levels (1 -+ w) / 2 against tsf_predict_intervals / tsf_predict_components, bit for bit."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import forecast_cases as fcs, helpers

pytestmark = pytest.mark.gpu

SEED = 17
LEVELS = np.array([0, 0.1, 0.25, 0.5, 0.9, 0.975, 1])


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU quantile tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _keys(c):
    return np.arange(c.N, dtype=np.int64) * 7919 + 3


def _kw(c, keys=None, **kw):
    return dict(floor=c.floor, cap=c.cap, extra_future=c.extra, series_key=_keys(c) if keys is None else keys, seed=SEED,
                **kw)


def _args(c):
    return c.spec, c.theta, c.y_scale, c.grid, c.fut


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _contract(v, levels):
    """the header's expression on draws v [..., S] -> [..., Q]: ascending sort, pos = p (S - 1), lo = floor(pos),
    hi = min(lo + 1, S - 1), v[lo] + (v[hi] - v[lo]) * (pos - lo)"""
    v = np.sort(v, axis=-1)
    S = v.shape[-1]
    out = []
    for p in levels:
        pos = np.float64(p) * np.float64(S - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, S - 1)
        out.append(v[..., lo] + (v[..., hi] - v[..., lo]) * (pos - np.float64(lo)))
    return np.stack(out, axis=-1)


def _beta0(c):
    """the case with every beta 0 and sigma = exp(-800) = 0: every yhat draw is its trend draw"""
    import copy
    b = copy.copy(c)
    b.theta = c.theta.copy()
    b.theta[:, 3 + c.spec.n_changepoints:] = 0.0
    b.theta[:, 2] = -800.0
    return b


# ---- 1. the interval entries' bits -----------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['iv65', 'iv129'])
@pytest.mark.parametrize('n_samples,w', [(2, 0.01), (3, 0.99), (1000, 0.8), (4096, 0.99)])
def test_levels_of_an_interval_are_the_interval(env, name, n_samples, w):
    fc, _lib = env
    c = fcs.make(name)
    pair = [(1.0 - w) / 2.0, (1.0 + w) / 2.0]
    r = fc.predict_quantiles(*_args(c), pair, trend=True, **_kw(c, uncertainty_samples=n_samples))
    yhat, lo, hi = fc.predict_intervals(*_args(c), interval_width=w, **_kw(c, uncertainty_samples=n_samples))
    assert r.q.shape == (c.N, 2, c.H) and r.cum_q is None
    assert _bits(r.q[:, 0], lo) and _bits(r.q[:, 1], hi)
    comp = fc.predict_components(*_args(c), intervals=True, interval_width=w, columns=[],
                                 **_kw(c, uncertainty_samples=n_samples))
    assert _bits(r.trend_q[:, 0], comp.trend_lower) and _bits(r.trend_q[:, 1], comp.trend_upper)
    point = fc.predict(*_args(c), floor=c.floor, cap=c.cap, extra_future=c.extra)
    assert _bits(r.yhat, point) and _bits(yhat, point)
    # seven levels that include the two: the same two rows
    seven = [0.5, pair[1], 0.0, 0.33, pair[0], 1.0, 0.7]
    r7 = fc.predict_quantiles(*_args(c), seven, trend=True, **_kw(c, uncertainty_samples=n_samples))
    assert _bits(r7.q[:, 4], lo) and _bits(r7.q[:, 1], hi)
    assert _bits(r7.trend_q[:, 4], comp.trend_lower) and _bits(r7.trend_q[:, 1], comp.trend_upper)
    assert _bits(r7.yhat, point)


# ---- 2. the raw draws against the oracle --------------------------------------------------------------------------

def _oracle_rows(cl, c, n_samples, width):
    """(lower, upper) [N][H] of oracle cn_predict_intervals"""
    csp = fcs.oracle_spec(c)
    keys = _keys(c)
    lo, hi = np.zeros((c.N, c.H)), np.zeros((c.N, c.H))
    for n in range(c.N):
        fitres, fut, fl, cp, ex = fcs.series_args(c, n)
        lo[n], hi[n] = cl.predict_intervals(csp, fitres, fut, fl, cp, ex, n_samples=n_samples, interval_width=width,
                                            seed=SEED, series_key=int(keys[n]))
    return lo, hi


def _oracle_sorted65(cl, c):
    """[N][H][65]: every row's order statistics from 33 oracle calls (width 1 - 2 j / 64: v[j] and v[64 - j] exactly)"""
    v = np.zeros((c.N, c.H, 65))
    for j in range(33):
        v[:, :, j], v[:, :, 64 - j] = _oracle_rows(cl, c, 65, 1.0 - 2.0 * j / 64.0)
    return v


def _oracle_first3(cl, c):
    """[N][H][3]: samples 0, 1, 2 -- the 1-sample call, then the value new among 2 (min / max) and among 3 (min /
    median / max) samples"""
    s0, _ = _oracle_rows(cl, c, 1, 0.5)
    mn2, mx2 = _oracle_rows(cl, c, 2, 1.0)
    assert ((mn2 == s0) | (mx2 == s0)).all()
    s1 = np.where(mn2 == s0, mx2, mn2)
    mn3, mx3 = _oracle_rows(cl, c, 3, 1.0)
    md3, md3b = _oracle_rows(cl, c, 3, 0.0)
    assert np.array_equal(md3, md3b)
    three = np.sort(np.stack([mn3, md3, mx3], axis=-1), axis=-1)
    two = np.sort(np.stack([s0, s1], axis=-1), axis=-1)
    s2 = np.zeros_like(s0)
    for idx in np.ndindex(s0.shape):       # the multiset difference {3 samples} - {2 samples}
        rest = list(three[idx])
        for x in two[idx]:
            rest.remove(x)
        s2[idx] = rest[0]
    return np.stack([s0, s1, s2], axis=-1)


@pytest.fixture(scope='module')
def drawn(env):
    """per case: the case, the 65-sample call's draws, and the oracle's order statistics and first three samples of the
    yhat draws and (the beta = 0, sigma = 0 model) of the trend draws -- computed once, read by the tests below"""
    from oracle import canon_lib as cl
    fc, _lib = env
    out = {}
    for name in ('iv65', 'iv129'):
        c = fcs.make(name)
        ps = fc.predictive_samples(*_args(c), **_kw(c, uncertainty_samples=65))
        b = _beta0(c)
        out[name] = dict(c=c, ps=ps, sorted=_oracle_sorted65(cl, c), first3=_oracle_first3(cl, c),
                         tsorted=_oracle_sorted65(cl, b), tfirst3=_oracle_first3(cl, b))
        for v in out[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


@pytest.mark.parametrize('name', ['iv65', 'iv129'])
def test_samples_against_the_oracle(env, drawn, name):
    fc, _lib = env
    d = drawn[name]
    c, ps = d['c'], d['ps']
    assert ps['yhat'].shape == ps['trend'].shape == (c.N, c.H, 65)
    # every row's 65 values are distinct in the oracle, so the reconstruction has no ambiguity
    assert (np.diff(d['sorted'], axis=-1) > 0).all()
    assert np.array_equal(np.sort(ps['yhat'], axis=-1), d['sorted'])
    assert np.array_equal(ps['yhat'][:, :, :3], d['first3'])
    # the trend draws: the oracle on the model with beta = 0 and no observation noise (values: +-0 alike) ...
    assert np.array_equal(np.sort(ps['trend'], axis=-1), d['tsorted'])
    assert np.array_equal(ps['trend'][:, :, :3], d['tfirst3'])
    # ... and the library's own yhat draws of that model
    b = _beta0(c)
    pb = fc.predictive_samples(*_args(b), **_kw(b, uncertainty_samples=65))
    assert np.array_equal(ps['trend'], pb['yhat']) and np.array_equal(pb['trend'], pb['yhat'])


@pytest.mark.parametrize('name', ['iv65', 'iv129'])
def test_prefix_property(env, drawn, name):
    """sample s does not depend on n_samples"""
    fc, _lib = env
    d = drawn[name]
    c = d['c']
    for m in (2, 3, 17):
        pm = fc.predictive_samples(*_args(c), **_kw(c, uncertainty_samples=m))
        assert pm['yhat'].shape == (c.N, c.H, m)
        assert _bits(pm['yhat'], d['ps']['yhat'][:, :, :m]) and _bits(pm['trend'], d['ps']['trend'][:, :, :m]), m


# ---- 3. the quantiles from the draws -------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['iv65', 'iv129'])
@pytest.mark.parametrize('n_samples', [2, 65, 1000])
def test_quantiles_are_the_contract_on_the_samples(env, name, n_samples):
    fc, _lib = env
    c = fcs.make(name)
    r = fc.predict_quantiles(*_args(c), LEVELS, cumulative=True, trend=True, **_kw(c, uncertainty_samples=n_samples))
    ps = fc.predictive_samples(*_args(c), **_kw(c, uncertainty_samples=n_samples))
    assert np.array_equal(r.quantiles, LEVELS)
    for got, draws in ((r.q, ps['yhat']), (r.cum_q, np.cumsum(ps['yhat'], axis=1)), (r.trend_q, ps['trend'])):
        want = np.moveaxis(_contract(draws, LEVELS), -1, 1)          # [N][H][Q] -> [N][Q][H]
        assert got.shape == want.shape == (c.N, len(LEVELS), c.H)
        assert _bits(got, want)
    assert _bits(r.cum_q[:, :, 0], r.q[:, :, 0])
    for a in (r.q, r.cum_q, r.trend_q):                               # monotone in the level
        assert (np.diff(a, axis=1) >= 0).all()
    assert _bits(r.q[:, 0], ps['yhat'].min(axis=-1)) and _bits(r.q[:, -1], ps['yhat'].max(axis=-1))
    f = r.frame(1, c.fut if c.shared else c.fut[1])
    assert list(f.columns) == (['ds', 'yhat'] + fc.quantile_columns(LEVELS) + fc.quantile_columns(LEVELS, 'yhat_cum_q')
                               + fc.quantile_columns(LEVELS, 'trend_q'))
    assert np.array_equal(f['yhat_cum_q97.5'].values, r.cum_q[1, 5])


def test_one_row(env):
    """H = 1: the running sum is the sample"""
    fc, _lib = env
    c = fcs.make('h1')
    r = fc.predict_quantiles(*_args(c), LEVELS, cumulative=True, trend=True, **_kw(c, uncertainty_samples=65))
    ps = fc.predictive_samples(*_args(c), **_kw(c, uncertainty_samples=65))
    assert r.q.shape == (c.N, len(LEVELS), 1)
    assert _bits(r.q, np.moveaxis(_contract(ps['yhat'], LEVELS), -1, 1)) and _bits(r.cum_q, r.q)
    assert _bits(r.trend_q, np.moveaxis(_contract(ps['trend'], LEVELS), -1, 1))


# ---- 4. independence -----------------------------------------------------------------------------------------------

ALL = ('q', 'cum_q', 'trend_q', 'samples', 'trend_samples')


def _call(fc, c, want, n_samples, levels=LEVELS, sl=slice(None), keys=None):
    """the binding's one call (forecaster._predict_quantiles_call) on series `sl` of the case with any set of outputs"""
    keys = _keys(c) if keys is None else keys
    return fc._predict_quantiles_call(c.spec, c.theta[sl], c.y_scale[sl], c.grid if len(c.grid) == 1 else c.grid[sl],
                                      c.fut if c.shared else c.fut[sl], c.floor[sl], None if c.cap is None else c.cap[sl],
                                      c.extra if (c.extra is None or c.shared) else c.extra[sl], keys[sl], n_samples, SEED,
                                      levels, want, None)


@pytest.mark.parametrize('name', ['iv65', 'iv129'])
def test_any_subset_of_the_outputs(env, name):
    fc, _lib = env
    c = fcs.make(name)
    full = _call(fc, c, ALL, 65)
    subsets = [(k,) for k in ALL] + [('q', 'cum_q'), ('cum_q', 'trend_samples'), ('trend_q', 'samples'),
                                     ('q', 'samples', 'trend_samples'), ('cum_q', 'trend_q')]
    for want in subsets:
        r = _call(fc, c, want, 65)
        assert set(r) == set(want) | {'yhat'}
        for k in r:
            assert _bits(r[k], full[k]), (want, k)
    # no levels at all: the samples alone
    r = _call(fc, c, ('samples',), 65, levels=[])
    assert _bits(r['samples'], full['samples'])


@pytest.mark.parametrize('name', ['iv65', 'iv129'])
def test_sub_batch_with_the_same_keys(env, name):
    fc, _lib = env
    c = fcs.make(name)
    full = _call(fc, c, ALL, 65)
    sl = slice(1, c.N)
    part = _call(fc, c, ALL, 65, sl=sl)
    for k in part:
        assert _bits(part[k], full[k][sl]), k
    # the default key is the index in the call
    r0 = fc.predict_quantiles(*_args(c), LEVELS, floor=c.floor, cap=c.cap, extra_future=c.extra, seed=SEED,
                              uncertainty_samples=65, cumulative=True)
    r1 = fc.predict_quantiles(*_args(c), LEVELS, cumulative=True,
                              **_kw(c, keys=np.arange(c.N, dtype=np.int64), uncertainty_samples=65))
    assert _bits(r0.q, r1.q) and _bits(r0.cum_q, r1.cum_q)


def test_quantiles_over_several_chunks(env):
    """300 series x 960 steps x 1000 samples with the running sums: 16 MB of scratch per series, so the call runs 9
    chunks (34 series each); series 130 .. 170 (chunks 3, 4 and 5) against a call on them alone, which runs one"""
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
    keys = np.arange(c.N, dtype=np.int64) ^ 0x5555
    lv = [(1.0 - 0.8) / 2.0, 0.5, (1.0 + 0.8) / 2.0]
    r = fc.predict_quantiles(*_args(c), lv, cumulative=True, **_kw(c, keys=keys, uncertainty_samples=1000))
    sl = slice(130, 170)
    p = _call(fc, c, ('q', 'cum_q'), 1000, levels=lv, sl=sl, keys=keys)
    assert _bits(r.yhat[sl], p['yhat']) and _bits(r.q[sl], p['q']) and _bits(r.cum_q[sl], p['cum_q'])
    _, lo, hi = fc.predict_intervals(*_args(c), interval_width=0.8, **_kw(c, keys=keys, uncertainty_samples=1000))
    assert _bits(r.q[:, 0], lo) and _bits(r.q[:, 2], hi)
    assert _bits(r.cum_q[:, :, 0], r.q[:, :, 0]) and (np.diff(r.cum_q, axis=1) >= 0).all()


def test_samples_over_several_chunks(env):
    """the raw draws leave the scratch chunk by chunk: 36 series x 960 steps x 1000 samples with the running sums (two
    sample buffers: 34 series per chunk) run 2 chunks; series 30 .. 36 (both chunks) against a call on them alone"""
    fc, _lib = env
    c = fcs.make('h960')
    rep = 12
    c.N = c.N * rep
    c.theta = np.tile(c.theta, (rep, 1))
    c.theta[:, 2] += np.linspace(-0.5, 0.5, c.N)
    c.y_scale = np.tile(c.y_scale, rep)
    c.floor = np.tile(c.floor, rep)
    assert c.N == 36
    lv = [0.5]
    full = _call(fc, c, ('samples', 'cum_q'), 1000, levels=lv)
    sl = slice(30, 36)
    part = _call(fc, c, ('samples', 'cum_q'), 1000, levels=lv, sl=sl)
    for k in ('yhat', 'samples', 'cum_q'):
        assert _bits(full[k][sl], part[k]), k
    want = np.moveaxis(_contract(np.cumsum(part['samples'], axis=1), lv), -1, 1)
    assert _bits(part['cum_q'], want)


# ---- 5. argument checks --------------------------------------------------------------------------------------------

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
    bufs = {k: np.zeros((N, 65, H)) for k in ('q', 'cum_q', 'trend_q')}
    bufs.update(yhat=np.zeros((N, H)), samples=np.zeros((N, H, 4097)), trend_samples=np.zeros((N, H, 4097)))

    def call(levels, n_samples=10, want=('q',), grid=c.grid, n_q=None, yhat=True):
        levels = np.ascontiguousarray(levels, dtype=np.float64)
        grid = np.ascontiguousarray(grid)
        out = _lib.TsfQuantileOut(**{k: bufs[k].ctypes.data for k in want + (('yhat',) if yhat else ())})
        return L.tsf_predict_quantiles(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, ys.ctypes.data,
                                       grid.ctypes.data, len(grid), fut.ctypes.data, 1, None, None, None, None, n_samples,
                                       0, len(levels) if n_q is None else n_q, levels.ctypes.data, ctypes.byref(out))

    ok = [0.1, 0.9]
    assert call(ok) == 0 and call(ok, want=ALL) == 0 and call([], want=('samples',)) == 0
    assert call(np.linspace(0, 1, 64), want=('q', 'cum_q', 'trend_q')) == 0
    bad_grid = c.grid.copy()
    bad_grid['S'][1] = -1
    for kw, why in ((dict(levels=np.linspace(0, 1, 65)), 'n_q'),
                    (dict(levels=ok, n_q=-1), 'n_q'),
                    (dict(levels=[0.5, -0.1]), r'quantiles\[1\]'),
                    (dict(levels=[1.5]), r'quantiles\[0\]'),
                    (dict(levels=[0.1, 0.2, float('nan')]), r'quantiles\[2\]'),
                    (dict(levels=ok, n_samples=1), 'n_samples'),
                    (dict(levels=ok, n_samples=4097), 'n_samples'),
                    (dict(levels=ok, n_samples=1, want=('samples',)), 'n_samples'),
                    (dict(levels=ok, want=()), 'nothing requested'),
                    (dict(levels=[], want=()), 'nothing requested'),
                    (dict(levels=[], want=('q',)), 'n_q = 0'),
                    (dict(levels=[], want=('cum_q', 'samples')), 'n_q = 0'),
                    (dict(levels=ok, yhat=False), 'yhat'),
                    # a bad grid is refused first: before the levels, the sample count and the outputs are looked at
                    (dict(levels=ok, grid=bad_grid), r'grid\[1\]'),
                    (dict(levels=[1.5], n_samples=1, want=(), grid=bad_grid), r'grid\[1\]')):
        rc = call(**kw)
        assert rc < 0, why
        assert re.search(why, L.tsf_last_error(ctx.handle).decode()), (why, L.tsf_last_error(ctx.handle))
    with pytest.raises(_lib.TsfError, match='quantiles'):
        fc.predict_quantiles(*_args(c), [0.5, 2.0], floor=c.floor)
    with pytest.raises(_lib.TsfError, match='n_samples'):
        fc.predict_quantiles(*_args(c), [0.5], floor=c.floor, uncertainty_samples=4097)
    with pytest.raises(ValueError, match='uncertainty_samples'):
        fc.predictive_samples(*_args(c), floor=c.floor, uncertainty_samples=1)
    # the context is usable: the same call as before the refusals, the same bits
    r = fc.predict_quantiles(*_args(c), ok, floor=c.floor, uncertainty_samples=10)
    assert call(ok) == 0 and _bits(r.q, bufs['q'].reshape(-1)[:N * 2 * H].reshape(N, 2, H))
    assert _bits(r.yhat, fc.predict(*_args(c), floor=c.floor))


# ---- 6. plain C ----------------------------------------------------------------------------------------------------

def test_abi_quantiles_plain_c(env, tmp_path):
    """tests/c/abi_quantiles.c drives tsf_predict_quantiles from plain C99 and writes what it returns"""
    fc, _lib = env
    c = fcs.make('iv129')
    d = str(tmp_path)
    np.ascontiguousarray(c.theta).tofile(d + '/theta.f64')
    np.ascontiguousarray(c.y_scale).tofile(d + '/ys.f64')
    np.ascontiguousarray(c.grid).tofile(d + '/grid.bin')
    np.ascontiguousarray(c.fut, dtype=np.int64).tofile(d + '/fut.i64')
    np.ascontiguousarray(c.extra).tofile(d + '/extra.f64')
    exe = d + '/abi_quantiles'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_quantiles.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(c.N), str(c.H), d])
    got = np.fromfile(d + '/out.f64')
    lv = [0.1, 0.5, 0.9]
    r = fc.predict_quantiles(*_args(c), lv, extra_future=c.extra, uncertainty_samples=50, seed=5, cumulative=True,
                             trend=True)
    ps = fc.predictive_samples(*_args(c), extra_future=c.extra, uncertainty_samples=50, seed=5)
    want = np.concatenate([r.yhat.ravel(), r.q.ravel(), r.cum_q.ravel(), r.trend_q.ravel(), ps['yhat'].ravel(),
                           ps['trend'].ravel()])
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0


# ---- 7. the scorer ------------------------------------------------------------------------------------------------

def test_scorer_quantiles(env):
    fc, _lib = env
    from time_series_spark_amd import panel as pk, synth
    from time_series_spark_amd.jobs import prophet_modeler as pm, prophet_scorer as ps
    H = 14
    ds, y = synth.make_panel(3, 400, 'linear', seed=4)
    df = pd.concat([pd.DataFrame({'series_id': 8 + n // 2, 'dim_id': n, 'ds': pd.to_datetime(ds), 'y': y[n]})
                    for n in range(3)], ignore_index=True)
    models = pm.model_panel({'model': {'floor': 0, 'cap_multiplier': 1.1,
                                       'prophet': {'growth': 'linear', 'seasonality_mode': 'additive'}}})(df)
    base = {'periods': H, 'frequency': 'D'}
    plain = ps.forecast_panel({'forecast': base})(models)
    assert list(plain.columns) == ['series_id', 'dim_id', 'ds', 'yhat']
    lv = [0.1, 0.5, 0.9]
    opts = dict(base, uncertainty_samples=300, seed=1)
    got = ps.forecast_panel({'forecast': dict(opts, quantiles=lv, cumulative=True)})(models)
    names = ['yhat_q10', 'yhat_q50', 'yhat_q90', 'yhat_cum_q10', 'yhat_cum_q50', 'yhat_cum_q90']
    assert list(got.columns) == list(plain.columns) + names
    assert got[list(plain.columns)].equals(plain) and all(got[n].dtype == np.float64 for n in names)
    noc = ps.forecast_panel({'forecast': dict(opts, quantiles=lv)})(models)
    assert list(noc.columns) == list(plain.columns) + names[:3] and noc.equals(got[list(noc.columns)])
    # fc.predict_quantiles on the model blobs, as a user would call it
    sids, dids = models['series_id'].to_numpy(), models['dim_id'].to_numpy()
    (spec_dict, idx, rec), = list(pk.load_models(models['model'].tolist()))
    spec = fc.ModelSpec.from_dict(spec_dict)
    theta = np.zeros((len(idx), spec.theta_stride))
    theta[:, :rec['theta'].shape[1]] = rec['theta']
    key = (sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff)
    r = fc.predict_quantiles(spec, theta, rec['y_scale'], pk.grid_from_records(rec),
                             pk.future_dates(rec['last_ds_ns'], H, 'D'), lv,
                             floor=models['floor'].to_numpy(np.float64)[idx], cap=models['cap'].to_numpy(np.float64)[idx],
                             series_key=key, uncertainty_samples=300, seed=1, cumulative=True)
    for j, i in enumerate(idx):
        rows = got[(got['series_id'] == sids[i]) & (got['dim_id'] == dids[i])]
        assert len(rows) == H
        for k, name in enumerate(names[:3]):
            assert _bits(rows[name].values, r.q[j, k]) and _bits(rows[names[3 + k]].values, r.cum_q[j, k])
    # with the intervals at width 0.8: consistent draws.  The interval's levels are (1 - 0.8) / 2 and (1 + 0.8) / 2 formed in
    # double (include/tsf.h); both are named yhat_q10 / yhat_q90 and give yhat_lower / yhat_upper bit for bit.  The literal
    # 0.9 is that upper level; the literal 0.1 is one ulp above the lower one (0.09999999999999998), so its column
    # differs from yhat_lower in the rounding of the interpolation weight and is not compared here.
    w = 0.8
    lw = [(1.0 - w) / 2.0, 0.5, (1.0 + w) / 2.0]
    both = ps.forecast_panel({'forecast': dict(opts, quantiles=lw, cumulative=True, intervals=True)})(models)
    assert list(both.columns) == list(plain.columns) + ['yhat_lower', 'yhat_upper'] + names
    assert _bits(both['yhat_q10'].values, both['yhat_lower'].values)
    assert _bits(both['yhat_q90'].values, both['yhat_upper'].values)
    lit = ps.forecast_panel({'forecast': dict(opts, quantiles=lv, cumulative=True, intervals=True)})(models)
    assert list(lit.columns) == list(both.columns) and lit[names].equals(got[names])
    assert _bits(lit['yhat_q90'].values, lit['yhat_upper'].values) and lit['yhat_lower'].equals(both['yhat_lower'])
    assert both[names[1:3] + names[4:]].equals(got[names[1:3] + names[4:]])
    # a series gets the same quantiles whatever frame it arrives in
    one = ps.forecast_panel({'forecast': dict(opts, quantiles=lv, cumulative=True)})(models.iloc[[2]])
    sel = got[(got['series_id'] == sids[2]) & (got['dim_id'] == dids[2])].reset_index(drop=True)
    assert one.reset_index(drop=True).equals(sel)
    with pytest.raises(ValueError):
        ps.forecast_panel({'forecast': dict(opts, quantiles=[0.1, 1.2])})(models)
