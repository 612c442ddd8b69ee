"""CPU tests of the predictive sampler's reference (tests/sampler_ref.py) on the cases of tests/sampler_cases.py.

The kernel's draws are pinned bit for bit to oracle cn_predict_intervals, but the oracle is the same scheme written
twice.  Here the scheme itself is held against the laws of what it claims to draw (fbprophet's sample_predictive_trend
and sample_model): the restated stream scheme and an independent numpy sampler both pass the battery at the full sample
count (64 keys x 4 096 samples), seven subtly wrong variants of the scheme are each rejected at the same thresholds, and
the restatement is tied to the oracle on samples 0, 1 and 2.  tests/test_gpu_sampler.py runs the same battery on the
device."""
import math

import numpy as np
import pytest

from oracle import canon_lib as cl
from tests import sampler_cases as sc, sampler_ref as sr

IND_SEED = 99           # the independent sampler under test
REF_SEED = 7            # the independent sampler as the two-sample reference of the logistic case
MUTANT_CASE = 'lin_add_s25'         # a full piece of the Poisson draw and a remainder


def _report(tag, results):
    z, p = sr.extremes(results)
    print('%s: %d statistics, largest |z| %.3f, smallest p %.3g' % (tag, len(results), z, p))
    for name, kind, value in results:
        print('    %-78s %s %.6g' % (name, kind, value))


@pytest.fixture(scope='module')
def logistic_ref():
    d = sr.independent_draws(sc.make('logistic_s3').sampler, sc.N, sc.NS, REF_SEED)
    for v in d.values():
        v.setflags(write=False)
    return d


def _battery(c, draws, logistic_ref):
    ref = logistic_ref if c.sampler.growth == 'logistic' else None
    return sr.battery(draws, c.sampler, c.fine, ref=ref, ks_rows=sc.LOGISTIC_KS_ROWS)


def _restated(c, mutant=None, **kw):
    return sr.restated_draws(c.sampler, np.arange(sc.N), sc.NS, sc.SEED, mutant=mutant, noise_index=np.argsort(c.perm),
                             **kw)


# ---- the thresholds' premises ------------------------------------------------------------------------------------

def test_kink_threshold_misses_a_real_kink_with_probability_below_1e_7():
    p = sr.kink_miss_probability()
    x0 = sr.KINK_X0
    assert abs(p - x0 * (1.0 - np.euler_gamma - math.log(x0))) <= 1e-3 * p
    assert p < 1e-7


def test_windows_hold_three_kinks_with_probability_below_1e_4():
    assert sr.neglected_mass(sr.WINDOW_MU_MAX) < sr.NEGLECTED_MAX
    for name in sc.CASES:
        c = sc.make(name)
        tf = c.sampler.t[c.fine[0]:c.fine[1]]
        dt = np.diff(tf)
        assert np.allclose(dt, dt[0], rtol=1e-9, atol=0)          # (t is the rounded quotient of exact integers)
        assert c.sampler.S_cp * 2.0 * dt[0] <= sr.WINDOW_MU_MAX * (1 + 1e-9)
        assert c.sampler.t[-1] == (1.0 if name == 'rate0' else 1.5)
    rates = [sc.make(n).sampler.rate for n in ('lin_add_s1', 'lin_add_s16', 'lin_add_s25', 'lin_add_s60')]
    assert rates == [0.5, 8.0, 12.5, 30.0]


def test_statistics_merge_small_cells_and_switch_to_the_exact_law():
    """chi-square cells that expect fewer than 10 are merged into a neighbour, never dropped (the first cell into the
    one after it); a count goes by the normal approximation only where events and non-events both expect 1 000"""
    name, kind, p = sr.chi2_stat('x', [0, 1, 50, 40, 2, 0], [0.5, 2.0, 48.0, 40.0, 2.0, 0.5])
    want = sr.stats.chi2.sf(0.5 ** 2 / 50.5 + 0.5 ** 2 / 42.5, 1)          # the cells (0, 1, 2) and (3, 4, 5)
    assert kind == 'p' and abs(p - want) <= 1e-12
    assert sr.count_stat('c', 1100, 10 ** 6, 1e-3)[1] == 'z' and sr.count_stat('c', 900, 10 ** 6, 0.9e-3)[1] == 'p'
    name, kind, p = sr.count_stat('c', 43, 10 ** 6, 4.3e-5)
    assert kind == 'p' and 0.9 <= p <= 1.0
    assert sr.count_stat('c', 0, 100, 0.0)[2] == 1.0 and sr.count_stat('c', 1, 100, 0.0)[2] == 0.0


def test_laws_against_a_direct_simulation():
    """the closed forms of the compound-Poisson moments against numpy's own draws of the definition (small, fast): the
    variance, the fourth moment, the covariance and the variance of the product at two rows"""
    rng = np.random.default_rng(1)
    S_cp, lam, Tm, a, b, P = 5, 0.4, 1.5, 1.2, 1.45, 400000
    laws = sr.Laws(S_cp, lam, Tm)
    n = rng.poisson(laws.rate, P)
    J = n.max()
    tau = np.where(np.arange(J)[None, :] < n[:, None], rng.uniform(1.0, Tm, (P, J)), np.inf)
    d = rng.laplace(0.0, lam, (P, J))
    Da, Db = [(d * np.clip(x - tau, 0.0, None)).sum(axis=1) for x in (a, b)]
    for got, want, var in ((Da ** 2, laws.var(a), laws.moment4(a) - laws.var(a) ** 2),
                           (Db ** 4, laws.moment4(b), laws.moment8(b) - laws.moment4(b) ** 2),
                           (Da * Db, laws.cov(a, b), laws.var_of_product(a, b))):
        assert abs(got.mean() - want) <= 4.5 * math.sqrt(var / P), (got.mean(), want)
        assert abs(got.var() / var - 1.0) <= 0.25           # (the variance of a heavy-tailed variable: loosely)


# ---- the generator's map to a double --------------------------------------------------------------------------------

def test_u01_reaches_one_and_every_consumer_stays_finite_there():
    """((x >> 11) + 0.5) 2^-53 is documented as lying in (0, 1), but 2^53 - 1 + 0.5 is not representable (ties to
    even: 2^53), so the top 53-bit value gives exactly 1.0, with probability 2^-53.  Each consumer of that value:
    the Laplace inversion takes dm_log(2 (1 - u)) = dm_log(0) = -1023 ln 2 (a slope change of 709 lam, finite), the
    order-statistic recurrence dm_log(u) / rem = 0 (the time repeats the one before), Box-Muller sqrt(-2 dm_log(1)) = 0
    (z = 0), the Poisson product a factor of 1."""
    assert float(2 ** 53 - 1) + 0.5 == 2.0 ** 53
    top = np.array([2 ** 64 - 1, (2 ** 53 - 1) << 11, ((2 ** 53 - 2) << 11) | 0x7ff, 0, 0x7ff, 1 << 11], dtype=np.uint64)
    u = sr.u01_from_bits(top)
    assert u[0] == 1.0 and u[1] == 1.0
    # (above 2^52 every + 0.5 is a tie: an even 53-bit value keeps its own, 2^53 - 2 -> 1 - 2^-52)
    assert u[2] == 1.0 - 2.0 ** -52 and u[3] == u[4] == 2.0 ** -54 and u[5] == 1.5 * 2.0 ** -53
    assert ((u > 0.0) & (u <= 1.0)).all()
    L = cl.lib()
    log0 = L.cn_det_log(2.0 * (1.0 - u[0]))
    assert math.isfinite(log0) and abs(log0 + 1023.0 * math.log(2.0)) <= 1e-9
    lam = 0.3
    assert math.isfinite(-(lam * log0)) and -(lam * log0) > 0
    assert L.cn_det_log(u[0]) == 0.0 and L.cn_det_exp(L.cn_det_log(u[0]) / 3.0) == 1.0
    z = math.sqrt(-2.0 * L.cn_det_log(u[0])) * 0.7
    assert z == 0.0
    # the smallest value: every logarithm is of a normal number
    assert math.isfinite(L.cn_det_log(u[3])) and math.isfinite(L.cn_det_log(2.0 * u[3]))


def test_key_schedule_separates_every_argument():
    k = sr.stream_key(5, np.arange(4), 0, 0)
    assert len(set(k.tolist())) == 4
    assert sr.stream_key(5, 1, 2, 0) != sr.stream_key(5, 2, 1, 0) and sr.stream_key(5, 1, 2, 0) != sr.stream_key(5, 1, 2, 1)
    signed, unsigned = np.array([-3], dtype=np.int64), np.array([2 ** 64 - 3], dtype=np.uint64)
    assert sr.stream_key(5, signed, 2, 0) == sr.stream_key(5, unsigned, 2, 0)


# ---- the restatement is the oracle's scheme ------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(sc.CASES))
def test_restated_scheme_gives_the_oracles_first_three_samples(name):
    """samples 0, 1 and 2 of three series against oracle cn_predict_intervals (reconstructed as
    tests/test_gpu_quantiles._oracle_first3 does), within 1e-12 of max(|value|, sigma y_scale): libm and the
    deterministic transcendentals differ in the last places"""
    from tests import test_gpu_quantiles as tq
    c = sc.make(name)
    c.N = 3
    c.theta, c.y_scale, c.floor = c.theta[:3], c.y_scale[:3], c.floor[:3]
    c.cap = None if c.cap is None else c.cap[:3]
    want = tq._oracle_first3(cl, c)[:, np.argsort(c.perm), :]
    got = sr.restated_draws(c.sampler, tq._keys(c), 3, tq.SEED, noise_index=np.argsort(c.perm))['yhat']
    assert got.shape == want.shape == (3, sc.H, 3)
    tol = 1e-12 * np.maximum(np.abs(want), c.sampler.sigma * c.sampler.y_scale)
    assert (np.abs(got - want) <= tol).all(), np.max(np.abs(got - want) / tol)


# ---- the battery ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(sc.CASES))
def test_restated_scheme_passes_the_battery(name, logistic_ref):
    c = sc.make(name)
    d = _restated(c, want_counts=True)
    res = _battery(c, d, logistic_ref)
    # the count itself, which only the restatement shows: chi-square against Poisson(rate)
    rate = c.sampler.rate
    cnt = d['n_new'].ravel()
    if rate > 0.0:
        top = int(cnt.max()) + 1
        pmf = np.diff(np.concatenate([[0.0], sr.stats.poisson.cdf(np.arange(top), rate), [1.0]]))
        res.append(sr.chi2_stat('count of new changepoints against Poisson(%g)' % rate,
                                np.bincount(cnt, minlength=top + 1), pmf * cnt.size))
    else:
        res.append(('count of new changepoints[exact]', 'p', 1.0 if not cnt.any() else 0.0))
    _report('restated %s' % name, res)
    assert not sr.failures(res)
    if name == 'rate0':
        assert np.array_equal(d['trend'], np.broadcast_to(c.sampler.det_trend()[None, :, None], d['trend'].shape))


@pytest.mark.parametrize('name', list(sc.CASES))
def test_independent_sampler_passes_the_battery(name, logistic_ref):
    c = sc.make(name)
    res = _battery(c, sr.independent_draws(c.sampler, sc.N, sc.NS, IND_SEED), logistic_ref)
    _report('independent %s' % name, res)
    assert not sr.failures(res)


@pytest.mark.parametrize('mutant', sr.MUTANTS)
def test_battery_rejects_a_subtly_wrong_scheme(mutant, logistic_ref):
    """each mutant of the restated scheme fails at least one statistic at the thresholds the device is held to"""
    c = sc.make(MUTANT_CASE)
    res = _battery(c, _restated(c, mutant), logistic_ref)
    bad = sr.failures(res)
    print('%s: rejected by %s' % (mutant, '; '.join('%s (%s %.3g)' % b for b in bad)))
    assert bad, mutant


def test_two_seeds_and_two_key_families_are_independent_streams():
    c = sc.make('lin_add_s16')
    a = sr.restated_draws(c.sampler, np.arange(sc.N), sc.NS, sc.SEED)
    res = []
    for family in ('next_seed', 'high_word'):
        keys, seed = sc.keys_of(family)
        b = sr.restated_draws(c.sampler, np.arange(sc.N) if keys is None else keys, sc.NS, seed)
        res += sr.cross_stats(a, b, c.sampler, 'index keys against %s' % family)
    _report('cross', res)
    assert len(res) == 4 and not sr.failures(res)
