"""GPU tests of the predictive sampler's draws (interval_sample_kernel) against their distribution laws.

Every other test of the draws compares them with oracle cn_predict_intervals, which is the same scheme written twice.
Here fc.predictive_samples is held against the laws of what the scheme claims to draw (tests/sampler_ref.py: the
battery, run on the CPU by tests/test_sampler_ref.py on the restated scheme, on an independent numpy sampler and on
seven mutants that it rejects), on every case of tests/sampler_cases.py and every key family: 64 series with identical
parameters and different keys, 4 096 samples, 32 rows.  The deterministic trend and the additive and multiplicative
terms that the draws are decomposed with are the library's own (predict_components).

Thresholds (tests/sampler_ref.py; derived, not measured): every z-score within 5.5, every p-value at least 1e-7; the
module has 1 874 statistics, so a scheme that follows the laws fails it with probability below 1e-4.  Seeds and
keys are fixed in the case file."""
import numpy as np
import pytest
from scipy import stats

from tests import sampler_cases as sc, sampler_ref as sr

pytestmark = pytest.mark.gpu

REF_SEED = 7


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU sampler tests cannot run (product has no CPU fallback)')
    return fc


@pytest.fixture(scope='module')
def logistic_ref():
    d = sr.independent_draws(sc.make('logistic_s3').sampler, sc.N, sc.NS, REF_SEED)
    for v in d.values():
        v.setflags(write=False)
    return d


def _args(c):
    return c.spec, c.theta, c.y_scale, c.grid, c.fut


def _draw(fc, c, family):
    """the library's draws with the rows in increasing order"""
    keys, seed = sc.keys_of(family)
    ps = fc.predictive_samples(*_args(c), floor=c.floor, cap=c.cap, extra_future=c.extra, series_key=keys,
                               uncertainty_samples=sc.NS, seed=seed)
    assert ps['yhat'].shape == ps['trend'].shape == (sc.N, sc.H, sc.NS)
    inv = np.argsort(c.perm)
    return {k: v[:, inv, :] for k, v in ps.items()}


def _terms(fc, c):
    """(deterministic trend, additive term, 1 + multiplicative term) [N][H] as the library reports them, rows in
    increasing order"""
    comp = fc.predict_components(*_args(c), floor=c.floor, cap=c.cap, extra_future=c.extra)
    inv = np.argsort(c.perm)
    return comp.trend[:, inv], comp.terms['additive_terms'][:, inv], 1.0 + comp.terms['multiplicative_terms'][:, inv]


def _report(tag, results):
    z, p = sr.extremes(results)
    print('%s: %d statistics, largest |z| %.3f, smallest p %.3g' % (tag, len(results), z, p))
    for name, kind, value in results:
        print('    %-78s %s %.6g' % (name, kind, value))


@pytest.mark.parametrize('family', sc.FAMILIES)
@pytest.mark.parametrize('name', list(sc.CASES))
def test_draws_follow_their_laws(env, logistic_ref, name, family):
    fc = env
    c = sc.make(name)
    det, xa, opm = _terms(fc, c)
    # the library's terms are the hand-made model's (so the laws are those of the model that was written down)
    m = c.sampler
    assert np.allclose(det, m.det_trend()[None, :], rtol=1e-12, atol=1e-12 * m.y_scale)
    assert np.allclose(xa, m.xa[None, :], rtol=1e-12, atol=1e-12 * m.y_scale)
    assert np.allclose(opm, m.opm[None, :], rtol=1e-12)
    d = _draw(fc, c, family)
    res = sr.battery(d, m, c.fine, det_trend=det, xa=xa, opm=opm,
                     ref=logistic_ref if m.growth == 'logistic' else None, ks_rows=sc.LOGISTIC_KS_ROWS)
    _report('%s / %s' % (name, family), res)
    assert len(res) == (42 if m.growth == 'linear' else 41)        # no case leaves a statistic out
    assert not sr.failures(res)
    if name == 'rate0':             # no new changepoint: every trend draw is the deterministic trend
        assert np.max(np.abs(d['trend'] - det[:, :, None]) / np.abs(det[:, :, None])) <= 1e-12


@pytest.mark.parametrize('name', list(sc.CASES))
def test_two_seeds_at_the_same_keys_are_independent(env, name):
    fc = env
    c = sc.make(name)
    res = sr.cross_stats(_draw(fc, c, 'index'), _draw(fc, c, 'next_seed'), c.sampler, 'seed against seed + 1')
    _report(name, res)
    assert res and not sr.failures(res)


def test_key_families_are_independent_of_each_other(env):
    """the same series under two key families: different streams"""
    fc = env
    c = sc.make('lin_add_s16')
    a = _draw(fc, c, 'index')
    res = []
    for family in ('high_word', 'low_word', 'stride'):
        res += sr.cross_stats(a, _draw(fc, c, family), c.sampler, 'index keys against %s' % family)
    _report('families', res)
    assert len(res) == 6 and not sr.failures(res)


def test_unsorted_rows_replay_the_stream(env):
    """the trend draws of a permuted row order are the permutation of the sorted order's, bit for bit"""
    fc = env
    u, s = sc.make('unsorted_s16'), sc.make('lin_add_s16')
    assert not np.array_equal(u.perm, np.arange(sc.H)) and np.array_equal(u.theta, s.theta)
    for family in ('index', 'stride'):
        du, ds = _draw(fc, u, family), _draw(fc, s, family)
        assert np.array_equal(du['trend'].view(np.int64), ds['trend'].view(np.int64))
        assert not np.array_equal(du['yhat'], ds['yhat'])          # the noise is counted by the caller's row index


def test_cumulative_quantiles_follow_the_sum_law(env):
    """no_cp: noise only (the trend deviation is of the order of lam = 1e-8 of y_scale), so the running sum of a
    sample at row h is N(sum of yhat over rows 0 .. h, (h + 1) sigma^2 y_scale^2).  With F that law's distribution
    function, F(the level-p quantile of n draws) -- the contract's interpolation between two order statistics -- has
    mean p + (1 - 2 p) / (n + 1) and variance p (1 - p) / (n + 2) (the uniform order statistics'; the curvature of F
    over one spacing is O(1 / n^2)); the mean over the 64 series is compared with it."""
    fc = env
    c = sc.make('no_cp')
    m = c.sampler
    levels = [0.1, 0.5, 0.9]
    r = fc.predict_quantiles(*_args(c), levels, floor=c.floor, cap=c.cap, extra_future=c.extra, cumulative=True,
                             uncertainty_samples=sc.NS, seed=sc.SEED)
    assert r.cum_q.shape == (sc.N, 3, sc.H)
    center = np.cumsum(r.yhat, axis=1)
    sd = m.sigma * m.y_scale * np.sqrt(np.arange(1, sc.H + 1))
    res = []
    for h in (0, 1, 15, 31):
        for i, p in enumerate(levels):
            F = stats.norm.cdf((r.cum_q[:, i, h] - center[:, h]) / sd[h])
            mean, var = p + (1.0 - 2.0 * p) / (sc.NS + 1), p * (1.0 - p) / (sc.NS + 2)
            res.append(sr.mean_stat('cumulative q%g at row %d' % (100 * p, h), F, mean, var))
    _report('sum law', res)
    assert len(res) == 12 and not sr.failures(res)
