"""GPU tests of the group roll-ups (tsf_rollup_create / _add / _quantiles / _free: rollup_add_kernel and
rollup_cumsum_kernel behind the draw loop tsf_predict_quantiles runs, quantile_kernel on the accumulators).

The reference in every test is numpy on fc.predictive_samples of the same members, keys, seed and sample count (the
contract of include/tsf.h, "group roll-ups"): zeros, then an explicit Python loop of acc = acc + x over the members in the
contract's order (add calls in call order, within a call ascending index); np.cumsum along the rows for the running
sums (sequential along that axis); the contract's quantile expression restated below.  Every comparison is bit for bit
on the int64 view, except the scorer's, whose bound is derived in that test.

The members.  tests/forecast_cases.py's interval cases are two series of 129 rows (iv129) and three of 65 rows (iv65).
The roll-up tests need many series on few rows -- 129 series on 2 rows, 65 on 3 -- so the cases are tiled here the way
test_quantiles_over_several_chunks tiles h960: the case's models repeated, theta and y_scale perturbed per series by a
seeded generator, the calendar the case's first rows (iv129: its shared hourly grid; iv65: the first rows of series 0,
which every member is then forecast on).  No fixture changes.  A sample does not depend on the sample count (pinned by
test_gpu_quantiles.test_prefix_property), so the reference draws are taken once at 4096 samples and cut."""
import ctypes
import os
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
        pytest.fail('no GPU visible: GPU roll-up tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


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


class Members(object):
    """N series of one spec to add: spec, theta, y_scale, grid [N], floor, cap (or None), keys"""

    def take(self, sl):
        m = Members()
        m.spec, m.N = self.spec, len(self.theta[sl])
        m.theta, m.y_scale, m.grid, m.floor, m.keys = self.theta[sl], self.y_scale[sl], self.grid[sl], self.floor[sl], self.keys[sl]
        m.cap = None if self.cap is None else self.cap[sl]
        return m


def _tiled(name, N, seed, key0=3):
    """case `name` repeated to N series, theta's seasonal block, sigma and y_scale perturbed per series -> (Members, case)"""
    c = fcs.make(name)
    rng = np.random.default_rng(seed)
    rep = -(-N // c.N)
    ncp = c.spec.n_changepoints
    m = Members()
    m.spec, m.N = c.spec, N
    m.theta = np.tile(c.theta, (rep, 1))[:N].copy()
    m.theta[:, 3 + ncp:] *= rng.uniform(0.5, 1.5, (N, 1))
    m.theta[:, 2] += rng.normal(0, 0.3, N)
    m.y_scale = np.tile(c.y_scale, rep)[:N] * rng.uniform(0.5, 2.0, N)
    m.grid = c.grid[np.arange(N) % len(c.grid)].copy()
    m.floor = np.tile(c.floor, rep)[:N].copy()
    m.cap = None if c.cap is None else np.tile(c.cap, rep)[:N].copy()
    m.keys = np.arange(N, dtype=np.int64) * 7919 + key0
    return m, c


def _draws(fc, m, cal, extra, S):
    """(draws [N][H][S], yhat [N][H]) of the members on the calendar: fc.predictive_samples and fc.predict"""
    args = (m.spec, m.theta, m.y_scale, m.grid, cal)
    ps = fc.predictive_samples(*args, floor=m.floor, cap=m.cap, extra_future=extra, series_key=m.keys,
                               uncertainty_samples=S, seed=SEED)
    return ps['yhat'], fc.predict(*args, floor=m.floor, cap=m.cap, extra_future=extra)


def _numpy_rollup(G, adds):
    """the contract in numpy.  adds: (group [n], draws [n][H][S], yhat [n][H]) per add call, in call order ->
    (acc [G][H][S], ysum [G][H], count [G])"""
    _, H, S = adds[0][1].shape
    acc, ysum, count = np.zeros((G, H, S)), np.zeros((G, H)), np.zeros(G, dtype=np.int64)
    for group, x, y in adds:
        for n in range(len(group)):          # ascending index in the call: a group's members in ascending order
            g = int(group[n])
            acc[g] = acc[g] + x[n]
            ysum[g] = ysum[g] + y[n]
            count[g] += 1
    return acc, ysum, count


def _expect_q(acc):
    """(q, cum_q) [G][Q][H] of accumulators [G][H][S]"""
    return (np.moveaxis(_contract(acc, LEVELS), -1, 1), np.moveaxis(_contract(np.cumsum(acc, axis=1), LEVELS), -1, 1))


def _check(roll, acc, ysum, count, groups=slice(None)):
    """the roll-up's samples, yhat, count, q and cum_q against the numpy accumulators"""
    r = roll.quantiles(LEVELS, cumulative=True)
    q, cq = _expect_q(acc)
    assert r.q.shape == (roll.G, len(LEVELS), roll.H)
    assert _bits(roll.samples()[groups], acc[groups])
    assert _bits(r.yhat[groups], ysum[groups]) and np.array_equal(r.count[groups], count[groups])
    assert _bits(r.q[groups], q[groups]) and _bits(r.cum_q[groups], cq[groups])
    assert _bits(r.cum_q[:, :, 0], r.q[:, :, 0])
    return r


def _add(roll, m, group, extra=None):
    roll.add(m.spec, m.theta, m.y_scale, m.grid, group, m.keys, floor=m.floor, cap=m.cap, extra_future=extra)


@pytest.fixture(scope='module')
def iv129(env):
    """129 series of iv129's model on its first 2 hourly rows (shared, 2 extra columns, mixed modes); groups n % 5 with
    series 128 alone in group 5 and group 6 empty; the reference draws at 4096 samples"""
    fc, _lib = env
    m, c = _tiled('iv129', 129, seed=11)
    d = dict(m=m, cal=np.ascontiguousarray(c.fut[:2]), extra=np.ascontiguousarray(c.extra[:, :2]), G=7)
    d['group'] = np.arange(129, dtype=np.int64) % 5
    d['group'][128] = 5
    d['draws'], d['yhat'] = _draws(fc, m, d['cal'], d['extra'], 4096)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@pytest.fixture(scope='module')
def iv65(env):
    """65 series of iv65's model (logistic, floor, cap) on the first three future rows of its series 0"""
    fc, _lib = env
    m, c = _tiled('iv65', 65, seed=12, key0=10 ** 7)
    assert m.spec.growth == 'logistic' and m.cap is not None and (m.floor != 0).any() and not c.shared
    return dict(m=m, cal=np.ascontiguousarray(c.fut[0, :3]))


# ---- 1. summed draws and quantiles are the contract ----------------------------------------------------------------

@pytest.mark.parametrize('n_samples', [2, 3, 65, 1000, 4096])
def test_sums_and_quantiles_are_the_contract(env, iv129, n_samples):
    fc, _lib = env
    d = iv129
    acc, ysum, count = _numpy_rollup(d['G'], [(d['group'], d['draws'][:, :, :n_samples], d['yhat'])])
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=n_samples, seed=SEED) as roll:
        _add(roll, d['m'], d['group'], d['extra'])
        r = _check(roll, acc, ysum, count)
    assert list(count) == [26, 26, 26, 25, 25, 1, 0]
    # the empty group: zeros (+0.0 bit for bit) and count 0
    assert r.count[6] == 0 and _bits(r.q[6], np.zeros((len(LEVELS), 2))) and _bits(r.cum_q[6], np.zeros((len(LEVELS), 2)))
    assert _bits(r.yhat[6], np.zeros(2))
    for a in (r.q, r.cum_q):                               # monotone in the level
        assert (np.diff(a, axis=1) >= 0).all()
    f = r.frame(1, d['cal'])
    assert list(f.columns) == ['ds', 'yhat'] + fc.quantile_columns(LEVELS) + fc.quantile_columns(LEVELS, 'yhat_cum_q')
    assert np.array_equal(f['yhat_cum_q97.5'].values, r.cum_q[1, 5])


def test_per_series_extra_columns(env, iv129):
    """extra_future [N][n_extra][H]: every member on its own columns, forecast as tsf_predict does per-series futures"""
    fc, _lib = env
    d = iv129
    m = d['m']
    extra = np.random.default_rng(5).normal(0, 1, (m.N, 2, 2))
    x, y = _draws(fc, m, np.tile(d['cal'], (m.N, 1)), extra, 65)
    acc, ysum, count = _numpy_rollup(d['G'], [(d['group'], x, y)])
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=65, seed=SEED) as roll:
        _add(roll, m, d['group'], extra)
        _check(roll, acc, ysum, count)


def test_predict_rollup(env, iv129):
    """the one-spec convenience on labels that are not dense"""
    fc, _lib = env
    d = iv129
    m = d['m']
    labels = 751 - 3 * d['group']                              # descending in the group index
    uniq, r = fc.predict_rollup(m.spec, m.theta, m.y_scale, m.grid, d['cal'], labels, LEVELS, m.keys, floor=m.floor,
                                extra_future=d['extra'], uncertainty_samples=65, seed=SEED, cumulative=True)
    assert list(uniq) == [736, 739, 742, 745, 748, 751]
    acc, ysum, count = _numpy_rollup(6, [(5 - d['group'], d['draws'][:, :, :65], d['yhat'])])
    q, cq = _expect_q(acc)
    assert _bits(r.q, q) and _bits(r.cum_q, cq) and _bits(r.yhat, ysum) and np.array_equal(r.count, count)


# ---- 2. a group of one is the series ---------------------------------------------------------------------------------

def test_a_group_of_one_is_the_series(env, iv129):
    """0.0 + x is x for every x the draws produce, so the group that holds series 128 alone has its quantiles"""
    fc, _lib = env
    d = iv129
    one = d['m'].take(slice(128, 129))
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=1000, seed=SEED) as roll:
        _add(roll, d['m'], d['group'], d['extra'])
        r = roll.quantiles(LEVELS, cumulative=True)
    p = fc.predict_quantiles(one.spec, one.theta, one.y_scale, one.grid, d['cal'], LEVELS, floor=one.floor,
                             extra_future=d['extra'], series_key=one.keys, uncertainty_samples=1000, seed=SEED,
                             cumulative=True)
    assert r.count[5] == 1
    assert _bits(r.q[5], p.q[0]) and _bits(r.cum_q[5], p.cum_q[0]) and _bits(r.yhat[5], p.yhat[0])


# ---- 3. logistic members on the roll-up's own rows -----------------------------------------------------------------

def test_logistic_members_on_the_rollups_rows(env, iv65):
    fc, _lib = env
    m, cal = iv65['m'], iv65['cal']
    group = np.arange(m.N, dtype=np.int64) % 4                 # interleaved
    x, y = _draws(fc, m, cal, None, 300)
    assert x.shape == (65, 3, 300)
    acc, ysum, count = _numpy_rollup(4, [(group, x, y)])
    with fc.Rollup(cal, 4, uncertainty_samples=300, seed=SEED) as roll:
        _add(roll, m, group)
        _check(roll, acc, ysum, count)


# ---- 4. two specs in one roll-up -------------------------------------------------------------------------------------

def test_two_specs_in_one_rollup(env, iv129, iv65):
    """iv129's and iv65's members in the same groups, two add calls on one calendar (iv65's first two rows of series 0);
    the sum follows the call order, whichever it is"""
    fc, _lib = env
    a, b = iv129['m'], iv65['m']
    cal = np.ascontiguousarray(iv65['cal'][:2])
    ga, gb = iv129['group'], np.arange(b.N, dtype=np.int64) % 5
    assert not set(a.keys) & set(b.keys)
    xa, ya = _draws(fc, a, cal, iv129['extra'], 65)
    xb, yb = _draws(fc, b, cal, None, 65)
    got = []
    for first_a in (True, False):
        adds = [(ga, xa, ya), (gb, xb, yb)]
        with fc.Rollup(cal, 7, uncertainty_samples=65, seed=SEED) as roll:
            for which in ((0, 1) if first_a else (1, 0)):
                if which == 0:
                    _add(roll, a, ga, iv129['extra'])
                else:
                    _add(roll, b, gb)
            acc, ysum, count = _numpy_rollup(7, adds if first_a else adds[::-1])
            r = _check(roll, acc, ysum, count)
            got.append(roll.samples())
        assert list(r.count) == [39, 39, 39, 38, 38, 1, 0]
    # (the two orders are two different sums: they agree to rounding, not necessarily in bits)
    assert np.allclose(got[0], got[1], rtol=0, atol=1e-12 * np.abs(got[0]).max())


# ---- 5. order and batching -------------------------------------------------------------------------------------------

def test_order_and_batching(env, iv129):
    fc, _lib = env
    d = iv129
    m, group, S = d['m'], d['group'], 1000
    x, y = d['draws'][:, :, :S], d['yhat']
    full = _numpy_rollup(d['G'], [(group, x, y)])
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=S, seed=SEED) as roll:
        _add(roll, m, group, d['extra'])
        one = (roll.samples(), roll.quantiles(LEVELS, cumulative=True))
    assert _bits(one[0], full[0])
    # two adds of [0, 64) and [64, 129); quantiles between them (the partial result) and after, twice
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=S, seed=SEED) as roll:
        _add(roll, m.take(slice(0, 64)), group[:64], d['extra'])
        _check(roll, *_numpy_rollup(d['G'], [(group[:64], x[:64], y[:64])]))
        _add(roll, m.take(slice(64, 129)), group[64:], d['extra'])
        r1 = _check(roll, *full)
        r2 = roll.quantiles(LEVELS, cumulative=True)
        assert _bits(roll.samples(), one[0])
    for r in (r1, r2):
        assert _bits(r.q, one[1].q) and _bits(r.cum_q, one[1].cum_q) and _bits(r.yhat, one[1].yhat)
        assert np.array_equal(r.count, one[1].count)
    # 40 unrelated series of the same spec in the same call, mapped to the spare group 6
    other, _ = _tiled('iv129', 40, seed=99, key0=5 * 10 ** 6)
    both = Members()
    both.spec, both.N, both.cap = m.spec, m.N + other.N, None
    for k in ('theta', 'y_scale', 'grid', 'floor', 'keys'):
        setattr(both, k, np.concatenate([getattr(m, k), getattr(other, k)]))
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=S, seed=SEED) as roll:
        _add(roll, both, np.concatenate([group, np.full(40, 6, dtype=np.int64)]), d['extra'])
        r = roll.quantiles(LEVELS, cumulative=True)
        assert _bits(roll.samples()[:6], one[0][:6])
    assert _bits(r.q[:6], one[1].q[:6]) and _bits(r.cum_q[:6], one[1].cum_q[:6]) and _bits(r.yhat[:6], one[1].yhat[:6])
    assert list(r.count) == list(one[1].count[:6]) + [40]


# ---- 6. groups across scratch chunks ---------------------------------------------------------------------------------

def test_groups_across_scratch_chunks(env):
    """90 series x 960 steps x 1000 samples: 8 * 960 * 1003 bytes of scratch per series, 69 series per chunk, so the call
    runs 2 chunks (69 + 21).  Groups n % 3, and group 3 = series 60 .. 71, which straddle the chunk boundary: against
    numpy on those 12 series' draws; every group against the same members added in two calls of 45 (one chunk each)"""
    fc, _lib = env
    m, c = _tiled('h960', 90, seed=9)
    m.keys = np.arange(90, dtype=np.int64) ^ 0x5555
    assert c.H == 960 and (512 << 20) // (8 * 960 * 1003) == 69
    group = np.arange(90, dtype=np.int64) % 3
    group[60:72] = 3
    with fc.Rollup(c.fut, 4, uncertainty_samples=1000, seed=SEED) as roll:
        _add(roll, m, group)
        acc = roll.samples()
        r = roll.quantiles(LEVELS, cumulative=True)
    x, y = _draws(fc, m.take(slice(60, 72)), c.fut, None, 1000)
    want, ysum, _ = _numpy_rollup(1, [(np.zeros(12, dtype=np.int64), x, y)])
    del x
    assert _bits(acc[3], want[0]) and _bits(r.yhat[3], ysum[0]) and r.count[3] == 12
    q, cq = _expect_q(want)
    assert _bits(r.q[3], q[0]) and _bits(r.cum_q[3], cq[0])
    with fc.Rollup(c.fut, 4, uncertainty_samples=1000, seed=SEED) as roll:
        _add(roll, m.take(slice(0, 45)), group[:45])
        _add(roll, m.take(slice(45, 90)), group[45:])
        assert _bits(roll.samples(), acc)
        r2 = roll.quantiles(LEVELS, cumulative=True)
    assert _bits(r2.q, r.q) and _bits(r2.cum_q, r.cum_q) and _bits(r2.yhat, r.yhat) and np.array_equal(r2.count, r.count)
    assert list(r.count) == [26, 26, 26, 12]


# ---- 7. argument checks ----------------------------------------------------------------------------------------------

def test_argument_checks(env, iv129, iv65):
    """every refusal of the contract: < 0 with a message, before anything is launched -- the roll-up's samples are bit
    for bit what they were, and the context fits and predicts as before"""
    fc, _lib = env
    from time_series_spark_amd import synth
    L = _lib.load()
    ctx = fc.get_context()
    d = iv129
    m, G, H = d['m'], d['G'], 2
    vp = ctypes.c_void_p

    def message():
        return L.tsf_last_error(ctx.handle).decode()

    ds, yy = synth.make_panel(2, 120, 'linear', seed=3)
    fspec = fc.ModelSpec(growth='linear', n_changepoints=5,
                         seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3, 'mode': 'additive'}])
    fit0 = fc.fit_aligned(fspec, ds, yy)
    pred0 = fc.predict(m.spec, m.theta, m.y_scale, m.grid, d['cal'], floor=m.floor, extra_future=d['extra'])

    # create
    cal = np.ascontiguousarray(d['cal'])
    for kw, why in ((dict(G=0), 'G'), (dict(G=-3), 'G'), (dict(H=0), 'H'), (dict(S=1), 'n_samples'), (dict(S=4097), 'n_samples'),
                    (dict(ds=None), 'ds_future')):
        a = dict(dict(G=G, H=H, S=10, ds=cal.ctypes.data), **kw)
        h = vp()
        rc = L.tsf_rollup_create(ctx.handle, a['G'], a['H'], a['ds'], a['S'], SEED, ctypes.byref(h))
        assert rc < 0 and not h.value, why
        assert why in message(), (why, message())

    roll = fc.Rollup(cal, G, uncertainty_samples=10, seed=SEED)
    _add(roll, m, d['group'], d['extra'])
    before = roll.samples()
    assert np.abs(before[:6]).min() > 0
    cs = m.spec.to_c()
    keys, group = np.ascontiguousarray(m.keys), np.ascontiguousarray(d['group'])
    theta, ys, grid, extra = (np.ascontiguousarray(v) for v in (m.theta, m.y_scale, m.grid, d['extra']))
    lg = iv65['m']                                      # logistic members: cap is required
    lcs = lg.spec.to_c()
    ltheta, lys, lgrid = (np.ascontiguousarray(v) for v in (lg.theta, lg.y_scale, lg.grid))
    lkeys, lgroup = np.ascontiguousarray(lg.keys), np.zeros(lg.N, dtype=np.int64)

    def add(N=m.N, group=group, keys=keys, grid=grid, n_grids=None, extra=extra, logistic=False):
        p = lambda v: None if v is None else v.ctypes.data     # noqa: E731
        if logistic:
            return L.tsf_rollup_add(roll._h, ctypes.byref(lcs), lg.N, p(ltheta), p(lys), p(lgrid), lg.N, None, None, None,
                                    1, p(lkeys), p(lgroup))
        return L.tsf_rollup_add(roll._h, ctypes.byref(cs), N, p(theta), p(ys), p(grid), len(grid) if n_grids is None else n_grids,
                                None, None, p(extra), 1, p(keys), p(group))

    hi, neg = group.copy(), group.copy()
    hi[100], neg[7] = G, -1
    bad_grid = grid.copy()
    bad_grid['S'][1] = -1
    for kw, why in ((dict(group=hi), r'group[100]'), (dict(group=neg), r'group[7]'), (dict(keys=None), 'series_key'),
                    (dict(grid=bad_grid), 'grid[1]'), (dict(extra=None), 'extra_future'), (dict(logistic=True), 'cap'),
                    (dict(n_grids=2), 'n_grids'), (dict(N=-1), 'N')):
        rc = add(**kw)
        assert rc < 0, why
        assert why in message(), (why, message())
        assert _bits(roll.samples(), before), why
    assert add(N=0) == 0 and _bits(roll.samples(), before)             # a legal no-op
    assert np.array_equal(roll.quantiles([0.5]).count, [26, 26, 26, 25, 25, 1, 0])

    # quantiles
    bufs = dict(yhat=np.zeros((G, H)), count=np.zeros(G, dtype=np.int64), q=np.zeros((G, 65, H)),
                cum_q=np.zeros((G, 65, H)), samples=np.zeros((G, H, 10)))

    def quant(levels, want=('yhat', 'count', 'q'), n_q=None):
        levels = np.ascontiguousarray(levels, dtype=np.float64)
        out = _lib.TsfRollupOut(**{k: bufs[k].ctypes.data for k in want})
        return L.tsf_rollup_quantiles(roll._h, len(levels) if n_q is None else n_q, levels.ctypes.data, ctypes.byref(out))

    ok = [0.1, 0.9]
    assert quant(ok) == 0 and quant(ok, want=tuple(bufs)) == 0 and quant([], want=('yhat', 'samples')) == 0
    assert quant(np.linspace(0, 1, 64), want=('yhat', 'q', 'cum_q')) == 0
    for kw, why in ((dict(levels=np.linspace(0, 1, 65)), 'n_q'), (dict(levels=ok, n_q=-1), 'n_q'),
                    (dict(levels=[0.5, -0.1]), 'quantiles[1]'), (dict(levels=[1.5]), 'quantiles[0]'),
                    (dict(levels=[0.1, 0.2, float('nan')]), 'quantiles[2]'),
                    (dict(levels=ok, want=('yhat', 'count')), 'nothing requested'),
                    (dict(levels=[], want=('yhat', 'q')), 'n_q = 0'), (dict(levels=[], want=('yhat',)), 'nothing requested'),
                    (dict(levels=ok, want=('q',)), 'yhat')):
        rc = quant(**kw)
        assert rc < 0, why
        assert why in message(), (why, message())
    assert _bits(roll.samples(), before)
    # the Python layer: TsfError from the library's refusals, ValueError from its own
    with pytest.raises(_lib.TsfError, match='grid'):
        roll.add(m.spec, m.theta, m.y_scale, bad_grid, d['group'], m.keys, extra_future=d['extra'])
    with pytest.raises(ValueError, match='series_key'):
        roll.add(m.spec, m.theta, m.y_scale, m.grid, d['group'], None, extra_future=d['extra'])
    with pytest.raises(ValueError, match='group'):
        roll.add(m.spec, m.theta, m.y_scale, m.grid, hi, m.keys, extra_future=d['extra'])
    with pytest.raises(ValueError):
        roll.quantiles([0.5, 2.0])
    assert _bits(roll.samples(), before)
    roll.close()
    roll.close()                                               # (closing twice is harmless)
    for call in (roll.samples, lambda: roll.quantiles([0.5]), lambda: _add(roll, m, d['group'], d['extra'])):
        with pytest.raises(ValueError, match='closed'):
            call()
    # the context is usable: the same fit and the same forecast as before the refusals
    fit1 = fc.fit_aligned(fspec, ds, yy)
    assert _bits(fit1.theta, fit0.theta) and np.array_equal(fit1.status, fit0.status)
    assert _bits(fc.predict(m.spec, m.theta, m.y_scale, m.grid, d['cal'], floor=m.floor, extra_future=d['extra']), pred0)


# ---- 8. plain C --------------------------------------------------------------------------------------------------------

def test_abi_rollup_plain_c(env, iv129, tmp_path):
    """tests/c/abi_rollup.c drives create / add twice / quantiles / free from plain C99 and writes what it returns"""
    fc, _lib = env
    d = iv129
    m = d['m']
    p = str(tmp_path)
    for name, v in (('theta.f64', m.theta), ('ys.f64', m.y_scale), ('grid.bin', m.grid), ('extra.f64', d['extra']),
                    ('fut.i64', d['cal']), ('key.i64', m.keys), ('group.i64', d['group'])):
        np.ascontiguousarray(v).tofile(os.path.join(p, name))
    exe = p + '/abi_rollup'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_rollup.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(m.N), '2', str(d['G']), p])
    got = np.fromfile(p + '/out.f64')
    lv = [0.1, 0.5, 0.9]
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=50, seed=5) as roll:
        _add(roll, m.take(slice(0, 64)), d['group'][:64], d['extra'])
        _add(roll, m.take(slice(64, 129)), d['group'][64:], d['extra'])
        r = roll.quantiles(lv, cumulative=True)
        want = np.concatenate([r.yhat.ravel(), r.q.ravel(), r.cum_q.ravel(), roll.samples().ravel()])
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0
    assert np.array_equal(np.fromfile(p + '/count.i64', dtype=np.int64), r.count)


# ---- 9. the scorer -----------------------------------------------------------------------------------------------------

def test_scorer_rollup(env, tmp_path):
    fc, _lib = env
    from time_series_spark_amd import panel as pk, synth
    from time_series_spark_amd.jobs import prophet_modeler as pm, prophet_scorer as ps
    H, S = 14, 300
    ds, y = synth.make_panel(6, 800, 'linear', seed=4)
    # series_id 8 and 9 with three dim_ids each; three series of 400 daily rows (the last 400 dates), three of 800
    frames = [pd.DataFrame({'series_id': 8 + n // 3, 'dim_id': n, 'ds': pd.to_datetime(ds[-T:]), 'y': y[n, -T:]})
              for n, T in enumerate([400, 800, 400, 800, 400, 800])]
    mcfg = {'model': {'floor': 0, 'cap_multiplier': 1.1, 'prophet': {'growth': 'linear', 'seasonality_mode': 'additive'}}}
    models = pm.model_panel(mcfg)(pd.concat(frames, ignore_index=True))
    buckets = list(pk.load_models(models['model'].tolist()))
    assert len(buckets) == 2                                   # the auto-seasonalities differ with the span
    lv = [0.1, 0.5, 0.9]
    cfg = {'forecast': {'periods': H, 'frequency': 'D', 'uncertainty_samples': S, 'seed': 1,
                        'rollup': {'by': 'series_id', 'quantiles': lv, 'cumulative': True}}}
    got = ps.rollup_panel(cfg)(models)
    names = ['yhat_q10', 'yhat_q50', 'yhat_q90', 'yhat_cum_q10', 'yhat_cum_q50', 'yhat_cum_q90']
    assert list(got.columns) == ['series_id', 'ds', 'yhat', 'count'] + names
    assert got['series_id'].dtype == np.int32 and got['count'].dtype == np.int64 and got['yhat'].dtype == np.float64
    assert got['ds'].dtype == np.dtype('datetime64[ns]') and all(got[n].dtype == np.float64 for n in names)
    assert list(got['series_id']) == [8] * H + [9] * H and (got['count'] == 3).all()
    fut = pk.future_dates(np.array([ds[-1]]), H, 'D')[0]
    assert np.array_equal(got['ds'].values.astype(np.int64), np.tile(fut, 2))
    # numpy sums of fc.predictive_samples per bucket.  The job does not promise the bucket order; two orders of a 3-term
    # double sum differ by at most a few ulp of (sum over members of max |draw|), and sorting and the interpolation
    # (weights in [0, 1]) pass a perturbation on with a factor of at most 1 (the running sum of 14 rows with at most 14 of
    # them): atol = 1e-12 * that scale is a derived bound (an ulp is 2.2e-16 of it), not a measured one.
    sids, dids = models['series_id'].to_numpy(), models['dim_id'].to_numpy()
    acc, ysum, scale = np.zeros((2, H, S)), np.zeros((2, H)), np.zeros(2)
    for spec_dict, idx, rec in buckets:
        spec = fc.ModelSpec.from_dict(spec_dict)
        theta = np.zeros((len(idx), spec.theta_stride))
        theta[:, :rec['theta'].shape[1]] = rec['theta']
        args = (spec, theta, rec['y_scale'], pk.grid_from_records(rec), fut)
        kw = dict(floor=models['floor'].to_numpy(np.float64)[idx], cap=models['cap'].to_numpy(np.float64)[idx])
        key = (sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff)
        x = fc.predictive_samples(*args, series_key=key, uncertainty_samples=S, seed=1, **kw)['yhat']
        yh = fc.predict(*args, **kw)
        for j, i in enumerate(idx):
            g = int(sids[i]) - 8
            acc[g] = acc[g] + x[j]
            ysum[g] = ysum[g] + yh[j]
            scale[g] += np.abs(x[j]).max()
    q = np.moveaxis(_contract(acc, lv), -1, 1)
    cq = np.moveaxis(_contract(np.cumsum(acc, axis=1), lv), -1, 1)
    for g in range(2):
        rows = got[got['series_id'] == 8 + g]
        atol = 1e-12 * scale[g]
        assert np.allclose(rows['yhat'].values, ysum[g], rtol=0, atol=atol)
        for k in range(3):
            assert np.allclose(rows[names[k]].values, q[g, k], rtol=0, atol=atol)
            assert np.allclose(rows[names[3 + k]].values, cq[g, k], rtol=0, atol=atol)
    # ProphetScorer.score writes the frame after the forecasts when io.rollup_forecasts is set
    mdir, fdir, rdir = (str(tmp_path / k) for k in ('models', 'forecasts', 'rollup'))
    pm.ProphetModeler({'io': {'models': mdir}}).persist_models(models)
    ps.ProphetScorer.score(None, dict(cfg, io={'models': mdir, 'forecasts': fdir, 'rollup_forecasts': rdir}))
    back = pd.read_csv(os.path.join(rdir, 'part-00000.csv'), float_precision='round_trip')
    assert list(back.columns) == list(got.columns) and len(back) == 2 * H
    assert _bits(back[names].to_numpy(np.float64), got[names].to_numpy(np.float64))
    assert os.path.exists(os.path.join(fdir, 'part-00000.csv'))
    # a frame whose series end on two different dates: refused, naming the dates
    frames[1] = frames[1].iloc[:-3]
    late = pm.model_panel(mcfg)(pd.concat(frames, ignore_index=True))
    with pytest.raises(ValueError, match='forecast.rollup needs one forecast calendar'):
        ps.rollup_panel(cfg)(late)
    with pytest.raises(ValueError):
        ps.rollup_panel({'forecast': dict(cfg['forecast'], rollup={'quantiles': [0.1, 1.2]})})(models)
