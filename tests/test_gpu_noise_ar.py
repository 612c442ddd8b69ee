"""GPU tests of the serially correlated observation noise (include/tsf.h "serially correlated observation noise"):
tsf_residual_autocorr / _dev (ar_series_kernel) bit for bit against tests/ar_ref.py, and tsf_set_noise_ar's draw (the
AR instance of interval_sample_kernel) against the independent draw's own normals bit for bit, against the restated
streams, against the chain's laws, and through every consumer of the draws.

Thresholds of the statistics: tests/sampler_ref.py's Z_MAX = 5.5 and P_MIN = 1e-7 (derived there, not measured).  Seeds,
keys and autocorrelations are fixed here; they are not to be tuned after a look at a result."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

from tests import ar_ref as ar, helpers, sampler_cases as sc, sampler_ref as sr, score_ref, window_ref

pytestmark = pytest.mark.gpu

SEED = 20241020


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU noise tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _same(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _report(tag, results):
    z, p = sr.extremes(results)
    print('%s: %d statistics, largest |z| %.3f, smallest p %.3g' % (tag, len(results), z, p))
    for name, kind, value in results:
        print('    %-78s %s %.6g' % (name, kind, value))


# ---- 1. the estimator, bit for bit -------------------------------------------------------------------------------------

EST_FIELDS = ('phi', 'phi_raw', 'n_pairs', 'scale', 'status')
N_EST = 12


def _estimator_panel(T, dtype, seed=23):
    """12 series of T rows with planted autocorrelations 0 .. 0.9 (one negative); series 3 has NaN rows in fitted (and in
    y where the dtype has a NaN), series 5 a zero residual, series 7 a constant residual -> (y, fitted)"""
    rng = np.random.default_rng(seed)
    phi = np.array([0.0, 0.3, 0.6, 0.9, -0.5, 0.2, 0.8, 0.1, 0.5, 0.7, 0.4, 0.95])
    e = np.stack([ar.chain(rng.standard_normal(T), p) for p in phi]) * rng.uniform(1.0, 30.0, (N_EST, 1))
    fitted = 100.0 + 10.0 * rng.standard_normal((N_EST, T))
    y = fitted + e
    y = np.rint(y).astype(np.int32) if dtype == np.int32 else y.astype(dtype)
    fitted[3, T // 3:T // 2 + 1] = np.nan
    if T > 4:
        fitted[3, -3] = np.nan
    if dtype != np.int32:
        y[3, -1] = np.nan
    fitted[5] = y[5].astype(np.float64)
    fitted[7] = y[7].astype(np.float64) - 2.0
    return y, fitted


def _check_estimate(got, want):
    for k in EST_FIELDS:
        assert _same(getattr(got, k), want[k]), (k, getattr(got, k), want[k])


@pytest.mark.parametrize('T', [1, 2, 64, 65, 129])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32], ids=['f64', 'f32', 'i32'])
def test_estimator_bit_for_bit_aligned(env, dtype, T):
    fc, _lib = env
    y, fitted = _estimator_panel(T, dtype)
    for kw in (dict(), dict(phi_max=0.4, min_pairs=1)):
        got = fc.residual_autocorrelation(y, fitted, **kw)
        _check_estimate(got, ar.autocorr(y, fitted, **kw))
    assert _lib.AR_NO_PAIRS == -51 and got.status[5] == _lib.AR_NO_PAIRS and np.isnan(got.scale[5])
    if T >= 2:
        assert got.status[7] == _lib.AR_OK and got.phi_raw[7] == 1.0 and got.phi[7] == 0.4 and got.scale[7] == 2.0
    if T >= 64:
        full = fc.residual_autocorrelation(y, fitted)
        assert (np.delete(full.status, 5) == _lib.AR_OK).all() and full.phi[4] == 0.0 and full.phi_raw[4] < 0.0
        assert full.phi[3] > 0.5 and full.n_pairs[3] < T - 1 and full.n_pairs[0] == T - 1
    assert list(got.frame().columns) == ['series', 'phi', 'phi_raw', 'n_pairs', 'scale', 'status']


@pytest.mark.parametrize('dtype', [np.float64, np.int32], ids=['f64', 'i32'])
def test_estimator_bit_for_bit_ragged(env, dtype):
    """lengths at the lane and butterfly edges, an empty series and a one-row series among them"""
    fc, _lib = env
    lens = [129, 0, 1, 200, 65, 2, 63, 128, 9, 130, 8, 64]
    y2, f2 = _estimator_panel(200, dtype)
    y = np.concatenate([y2[i, :n] for i, n in enumerate(lens)])
    fitted = np.concatenate([f2[i, :n] for i, n in enumerate(lens)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for kw in (dict(), dict(phi_max=0.5, min_pairs=2)):
        got = fc.residual_autocorrelation(y, fitted, offsets=offsets, **kw)
        _check_estimate(got, ar.autocorr(y, fitted, offsets, **kw))
    assert list(got.n_pairs[[1, 2, 5]]) == [0, 0, 1] and np.isnan(got.scale[1]) and not np.isnan(got.scale[2])
    assert (got.status[[1, 2, 5]] == _lib.AR_NO_PAIRS).all()
    # all series empty: nothing is read
    none = fc.residual_autocorrelation(np.zeros(0), np.zeros(0), offsets=np.zeros(4, np.int64))
    assert (none.status == _lib.AR_NO_PAIRS).all() and np.isnan(none.scale).all() and not none.phi.any()


def test_estimator_without_series(env):
    fc, _lib = env
    got = fc.residual_autocorrelation(np.zeros((0, 40)), np.zeros((0, 40)))
    assert got.phi.shape == got.status.shape == (0,)
    got = fc.residual_autocorrelation(np.zeros(0), np.zeros(0), offsets=np.zeros(1, np.int64))
    assert got.phi.shape == (0,)


def test_estimator_dev_variant_agrees(env):
    """tsf_residual_autocorr_dev on device pointers (plain hipMalloc blocks; offsets on the host) == the host variant"""
    fc, _lib = env
    from tests.test_gpu_screen import _hip_runtime
    hip = _hip_runtime()
    lens = [129, 0, 1, 200, 65, 2, 63, 128, 9, 130, 8, 64]
    y2, f2 = _estimator_panel(200, np.float64)
    yr = np.concatenate([y2[i, :n] for i, n in enumerate(lens)])
    fr = np.concatenate([f2[i, :n] for i, n in enumerate(lens)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bufs = []

    def dev(a_):
        a_ = np.ascontiguousarray(a_)
        p_ = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p_), max(a_.nbytes, 8)) == 0
        bufs.append(p_)
        assert hip.hipMemcpy(p_, a_.ctypes.data, a_.nbytes, 1) == 0             # hipMemcpyHostToDevice
        return p_
    ctx = fc.get_context()
    try:
        for y, fitted, off, T in ((y2, f2, None, 200), (yr, fr, offsets, 0)):
            want = fc.residual_autocorrelation(y, fitted, offsets=off)
            host = dict(phi=np.full(N_EST, 7.0), phi_raw=np.zeros(N_EST), n_pairs=np.zeros(N_EST, np.int64),
                        scale=np.zeros(N_EST), status=np.full(N_EST, 7, np.int32))
            d_y, d_f = dev(y), dev(fitted)
            o = {k: dev(v) for k, v in host.items()}
            out = _lib.TsfArOut(*[o[k] for k in EST_FIELDS])
            ctx.check(_lib.load().tsf_residual_autocorr_dev(ctx.handle, N_EST, T, None if off is None else off.ctypes.data,
                                                            d_y, _lib.Y_F64, d_f, None, ctypes.byref(out), None))
            assert hip.hipDeviceSynchronize() == 0
            for k, v in host.items():
                assert hip.hipMemcpy(v.ctypes.data, o[k], v.nbytes, 2) == 0         # hipMemcpyDeviceToHost
            for k in EST_FIELDS:
                assert _same(host[k], getattr(want, k)), k
    finally:
        for p_ in bufs:
            hip.hipFree(p_)


# ---- the models of the draw tests ----------------------------------------------------------------------------------------

class _M(object):
    """N series of one spec: spec, theta, y_scale, grid, fut, floor, cap, extra, keys"""

    def args(self):
        return self.spec, self.theta, self.y_scale, self.grid, self.fut

    def kw(self, keys=True):
        return dict(floor=self.floor, cap=self.cap, extra_future=self.extra, series_key=self.keys if keys else None)


def _unit_model(N, H):
    """sampler_cases' noise-only shape ('no_cp') with every parameter zero: k = m = 0, beta = 0, log sigma = 0, y_scale 1,
    floor 0, on rows at t <= 1 (its 'history' calendar), where no new changepoint can fall: the sampled trend is +0.0 and
    the draw is 0 * 1 + 0 + (z * 1) * 1 = z itself, provided the library's exp(0) is 1.0"""
    c = sc.make('no_cp')
    m = _M()
    m.spec, m.grid, m.cap = c.spec, c.grid, None
    m.theta = np.zeros((N, c.spec.theta_stride))
    m.y_scale, m.floor = np.ones(N), np.zeros(N)
    m.fut = np.ascontiguousarray(sc.START_NS + sc.row_offsets_ns(1, 'history')[:H])
    m.extra = np.ascontiguousarray(c.extra[:, :H])
    m.keys = 7919 * np.arange(N, dtype=np.int64) + 3
    return m


def _case_model(name, N, phi_seed=None):
    """the first N series of a sampler case (identical parameters, different keys) on its own 32 rows"""
    c = sc.make(name)
    m = _M()
    m.spec, m.grid, m.fut, m.extra = c.spec, c.grid, c.fut, c.extra
    m.theta, m.y_scale, m.floor = c.theta[:N], c.y_scale[:N], c.floor[:N]
    m.cap = None if c.cap is None else c.cap[:N]
    m.keys = 7919 * np.arange(N, dtype=np.int64) + 3
    m.sampler = c.sampler
    return m


def _samples(fc, m, S, seed=SEED, noise_ar=None, keys=True):
    return fc.predictive_samples(*m.args(), uncertainty_samples=S, seed=seed, noise_ar=noise_ar, **m.kw(keys))


# ---- 2. the chain, bit for bit, on a unit model ---------------------------------------------------------------------------

UNIT_PHI = np.array([0.0, 0.3, 0.6, 0.95, -0.5])


def test_chain_bit_for_bit_on_the_unit_model(env):
    """300 samples (a full block of 256 and a partial one), 9 rows, five series: with noise_ar row h of every sample is
    numpy's fl(fl(phi e) + fl(c z)) of the independent call's own values"""
    fc, _lib = env
    assert fc.selftest_math(2, np.zeros(1))[0] == 1.0           # the library's exp(0): sigma = 1 exactly
    m = _unit_model(5, 9)
    indep = _samples(fc, m, 300)
    assert not indep['trend'].any() and not np.signbit(indep['trend']).any()
    z = indep['yhat']
    assert abs(z.mean()) < 0.1 and abs(z.std() - 1.0) < 0.1        # (they are the normals)
    got = _samples(fc, m, 300, noise_ar=UNIT_PHI)
    assert _same(got['trend'], indep['trend'])
    for n, phi in enumerate(UNIT_PHI):
        assert _same(got['yhat'][n], ar.chain(z[n], phi, axis=0)), phi
    assert _same(got['yhat'][0], z[0])                             # phi = 0: the independent call's bits
    assert _same(got['yhat'][:, 0], z[:, 0])                       # row 0 of every series likewise
    assert (got['yhat'][1:, 1:] != z[1:, 1:]).mean() > 0.99
    # a NoiseAR is taken for its phi
    est = fc.NoiseAR(UNIT_PHI, None, None, None, None)
    assert _same(_samples(fc, m, 300, noise_ar=est)['yhat'], got['yhat'])


def test_one_row_is_the_independent_call(env):
    fc, _lib = env
    m = _unit_model(5, 1)
    assert _same(_samples(fc, m, 300, noise_ar=UNIT_PHI)['yhat'], _samples(fc, m, 300)['yhat'])


# ---- 3. a general model against the restated streams ----------------------------------------------------------------------

@pytest.mark.parametrize('name', ['lin_mul_s16', 'logistic_s3'])
def test_draw_against_the_restatement(env, name):
    """yhat_ar - yhat_indep against ((e - z) sigma) y_scale with z restated from sampler_ref's streams (numpy's log and
    cos) and e its chain, within 1e-12 * sigma * y_scale: the tolerance with which test_sampler_ref.py ties those
    streams to the deterministic recipes of the device.  The sampled trend is bit-identical with and without."""
    fc, _lib = env
    N, S = 6, 300
    m = _case_model(name, N)
    phi = np.array([0.0, 0.3, 0.6, 0.9, -0.5, 0.6])
    indep, got = _samples(fc, m, S), _samples(fc, m, S, noise_ar=phi)
    assert _same(got['trend'], indep['trend'])
    H = len(m.fut)
    knz = sr.stream_key(SEED, np.repeat(m.keys, S), np.tile(np.arange(S, dtype=np.int64), N), 1).reshape(N, 1, S)
    h2 = (2 * np.arange(H, dtype=np.uint64)).reshape(1, H, 1)
    z = sr.box_muller(sr.u01(knz, h2), sr.u01(knz, h2 + np.uint64(1)))
    e = np.stack([ar.chain(z[n], phi[n], axis=0) for n in range(N)])
    sig, ys = m.sampler.sigma, m.sampler.y_scale
    want = ((e - z) * sig) * ys
    err = np.abs((got['yhat'] - indep['yhat']) - want).max()
    tol = 1e-12 * sig * ys
    print('%s: largest deviation %.3g, tolerance %.3g, largest term %.3g' % (name, err, tol, np.abs(want).max()))
    assert np.abs(want).max() > sig * ys
    assert err <= tol
    assert _same(got['yhat'][0], indep['yhat'][0])


# ---- 4. laws on the device ----------------------------------------------------------------------------------------------

LAW_PHI = np.where(np.arange(sc.N) < sc.N // 2, 0.6, 0.3)
LAW_HALVES = ((0.6, slice(0, sc.N // 2)), (0.3, slice(sc.N // 2, sc.N)))
LEVELS = [0.1, 0.5, 0.9]


@pytest.fixture(scope='module')
def law_noise(env):
    """per seed (SEED, SEED + 1): the standardised noise [N][H][S] of the noise-only case ('no_cp': its sampled trend is
    the deviation itself at lam = 1e-8, nine orders below the noise) drawn with LAW_PHI: 64 series, 32 rows, 4 096 samples"""
    fc, _lib = env
    m = _case_model('no_cp', sc.N)
    out = []
    for seed in (SEED, SEED + 1):
        d = _samples(fc, m, sc.NS, seed=seed, noise_ar=LAW_PHI)
        s = m.sampler
        e = (d['yhat'] - d['trend'] * s.opm[None, :, None] - s.xa[None, :, None]) / (s.sigma * s.y_scale)
        e.setflags(write=False)
        out.append(e)
    return out


@pytest.mark.parametrize('seed_i', [0, 1])
def test_chained_noise_follows_its_laws(law_noise, seed_i):
    res = []
    for phi, half in LAW_HALVES:
        e = law_noise[seed_i][half]                             # [32][H][S]
        rows = np.ascontiguousarray(e.transpose(1, 0, 2)).reshape(sc.H, -1)
        res += [('phi %g: %s' % (phi, n), k, v) for n, k, v in ar.chain_law_stats(rows, phi)]
        for h in (0, 16, 31):
            res.append(('phi %g: row %d, KS against N(0,1)' % (phi, h), 'p', sr.ks_normal(rows[h])))
        last = (e[:, -1, :] - 0.0)
        res.append(sr.corr_stat('phi %g: neighbouring samples at the last row' % phi, last[:, :-1], last[:, 1:]))
        res.append(sr.corr_stat('phi %g: neighbouring keys at the last row' % phi, last[:-1], last[1:]))
    _report('seed %d' % seed_i, res)
    assert len(res) == 2 * (12 + 3 + 2) and not sr.failures(res)


def test_two_seeds_are_independent(law_noise):
    res = [sr.corr_stat('seed against seed + 1 at row %d' % h, law_noise[0][:, h, :], law_noise[1][:, h, :]) for h in (0, 31)]
    _report('seeds', res)
    assert not sr.failures(res)


def _sum_law_stats(fc, noise_ar):
    """the cumulative quantiles of the noise-only case against the normal law of the CHAINED running sum, pooled over the
    series of each half as test_gpu_sampler pools them: F(the level-p quantile of n draws) has mean p + (1 - 2 p) / (n + 1)
    and variance p (1 - p) / (n + 2)"""
    m = _case_model('no_cp', sc.N)
    r = fc.predict_quantiles(*m.args(), LEVELS, cumulative=True, uncertainty_samples=sc.NS, seed=SEED, noise_ar=noise_ar,
                             **m.kw())
    center = np.cumsum(r.yhat, axis=1)
    s = m.sampler
    res = []
    for phi, half in LAW_HALVES:
        for h in (1, 7, 31):
            sd = s.sigma * s.y_scale * math.sqrt(ar.sum_variance(h, phi))
            for i, p in enumerate(LEVELS):
                F = stats.norm.cdf((r.cum_q[half, i, h] - center[half, h]) / sd)
                mean, var = p + (1.0 - 2.0 * p) / (sc.NS + 1), p * (1.0 - p) / (sc.NS + 2)
                res.append(sr.mean_stat('phi %g: cumulative q%g at row %d' % (phi, 100 * p, h), F, mean, var))
    return res


def test_cumulative_quantiles_follow_the_chained_sum_law(env):
    fc, _lib = env
    res = _sum_law_stats(fc, LAW_PHI)
    _report('sum law', res)
    assert len(res) == 18 and not sr.failures(res)


def test_the_independent_draw_fails_the_chained_sum_law(env):
    """the companion: without noise_ar the same statistics reject, at the same thresholds -- the totals' spread is too
    narrow (the medians alone do not tell)"""
    fc, _lib = env
    bad = sr.failures(_sum_law_stats(fc, None))
    _report('independent', bad)
    assert len(bad) >= 12 and all('q50' not in name for name, _, _ in bad)


# ---- 5. consumers -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def general(env):
    """6 series of the multiplicative case on its 32 rows with mixed phi, 300 samples: the AR draws and the independent ones"""
    fc, _lib = env
    m = _case_model('lin_mul_s16', 6)
    phi = np.array([0.6, 0.0, 0.3, 0.9, -0.5, 0.6])
    return m, phi, _samples(fc, m, 300, noise_ar=phi)['yhat'], _samples(fc, m, 300)['yhat']


def test_quantiles_and_intervals_read_the_chained_draws(env, general):
    fc, _lib = env
    m, phi, draws, indep = general
    lv = [(1.0 - 0.8) / 2.0, 0.5, (1.0 + 0.8) / 2.0]           # (the levels predict_intervals forms at width 0.8)
    r = fc.predict_quantiles(*m.args(), lv, cumulative=True, uncertainty_samples=300, seed=SEED, noise_ar=phi, **m.kw())
    v = np.sort(draws, axis=-1)
    assert _same(r.q, np.stack([score_ref.quantile(v, p) for p in lv], axis=1))
    c = np.sort(window_ref.window_sums(draws, np.zeros(32, int), np.arange(1, 33)), axis=-1)
    assert _same(r.cum_q, np.stack([score_ref.quantile(c, p) for p in lv], axis=1))
    yhat, lo, hi = fc.predict_intervals(*m.args(), uncertainty_samples=300, interval_width=0.8, seed=SEED, noise_ar=phi, **m.kw())
    assert _same(lo, r.q[:, 0]) and _same(hi, r.q[:, 2]) and _same(yhat, r.yhat)


def test_windows_sum_the_chained_draws(env, general):
    fc, _lib = env
    m, phi, draws, indep = general
    start, end = np.array([0, 3, 7, 25, 0], np.int32), np.array([7, 4, 21, 32, 32], np.int32)
    w = fc.Windows(start, end)
    lv = [0.1, 0.5, 0.9]
    got = fc.predict_windows(*m.args(), w, lv, uncertainty_samples=300, seed=SEED, noise_ar=phi, **m.kw())
    assert _same(got.q, window_ref.score(draws, None, lv, start, end)['q'])
    assert not _same(got.q, window_ref.score(indep, None, lv, start, end)['q'])


def test_scores_rank_against_the_chained_draws(env, general):
    fc, _lib = env
    m, phi, draws, indep = general
    y_obs = np.ascontiguousarray(np.median(indep, axis=-1) + 3.0 * np.cos(np.arange(32))[None, :])
    y_obs[2, 5] = np.nan
    got = fc.score_actuals(*m.args(), y_obs, quantiles=[0.1, 0.9], uncertainty_samples=300, seed=SEED, noise_ar=phi, **m.kw())
    want = score_ref.score(draws, y_obs, [0.1, 0.9])
    assert score_ref.same(got.pit, want['pit']) and score_ref.same(got.q, want['q'])
    lt = (draws < y_obs[:, :, None]).sum(-1)
    eq = (draws == y_obs[:, :, None]).sum(-1)
    ok = ~np.isnan(y_obs)
    assert np.array_equal(got.pit[ok], ((lt + 0.5 * eq) / 300.0)[ok])
    assert not score_ref.same(got.pit, score_ref.score(indep, y_obs, [0.1, 0.9])['pit'])


def test_rollup_adds_the_chained_draws(env, general):
    """acc = +0.0 + the members' AR samples in list order, over two add calls (the second without a setting)"""
    fc, _lib = env
    m, phi, draws, indep = general
    group = np.array([0, 1, 0, 1, 0, 2], dtype=np.int64)
    with fc.Rollup(m.fut, 3, uncertainty_samples=300, seed=SEED) as roll:
        first = slice(0, 4)
        roll.add(m.spec, m.theta[first], m.y_scale[first], m.grid, group[first], m.keys[first], floor=m.floor[first],
                 extra_future=m.extra, noise_ar=phi[first])
        roll.add(m.spec, m.theta[4:], m.y_scale[4:], m.grid, group[4:], m.keys[4:], floor=m.floor[4:], extra_future=m.extra)
        got = roll.samples()
    want = np.zeros((3, 32, 300))
    for n in range(6):
        want[group[n]] = want[group[n]] + (draws[n] if n < 4 else indep[n])
    assert _same(got, want)
    uniq, r = fc.predict_rollup(m.spec, m.theta, m.y_scale, m.grid, m.fut, group, [0.5], m.keys, floor=m.floor,
                                extra_future=m.extra, uncertainty_samples=300, seed=SEED, noise_ar=phi)
    want = np.zeros((3, 32, 300))
    for n in range(6):
        want[group[n]] = want[group[n]] + draws[n]
    assert _same(r.q[:, 0], score_ref.quantile(np.sort(want, axis=-1), 0.5))


def test_batch_and_sample_count_independence(env):
    """a series drawn alone, in a batch of 64 and at 300 against 4 096 samples: the same first 300 samples"""
    fc, _lib = env
    m = _case_model('lin_mul_s16', 64)
    phi = np.linspace(-0.5, 0.9, 64)
    big = _samples(fc, m, 4096, noise_ar=phi)['yhat']
    small = _samples(fc, m, 300, noise_ar=phi)['yhat']
    assert _same(big[:, :, :300], small)
    one = _M()
    n = 37
    one.spec, one.grid, one.fut, one.extra, one.cap = m.spec, m.grid, m.fut, m.extra, None
    one.theta, one.y_scale, one.floor, one.keys = m.theta[n:n + 1], m.y_scale[n:n + 1], m.floor[n:n + 1], m.keys[n:n + 1]
    assert _same(_samples(fc, one, 300, noise_ar=phi[n:n + 1])['yhat'][0], small[n])


# ---- 6. the one-shot rule and refusals -------------------------------------------------------------------------------------

def test_one_shot_rule_and_refusals(env, general):
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    m, phi, draws, indep = general
    N = len(phi)

    def message():
        return L.tsf_last_error(ctx.handle).decode()

    def arm(p=phi, n=None):
        p = np.ascontiguousarray(p, dtype=np.float64)
        return L.tsf_set_noise_ar(ctx.handle, p.ctypes.data, len(p) if n is None else n)

    def draw():
        return _samples(fc, m, 300)['yhat']

    # consumed by the next drawing entry; the call after it is the independent one
    assert arm() == 0
    assert _same(draw(), draws) and _same(draw(), indep)
    # NULL or n == 0 clears
    assert arm() == 0 and L.tsf_set_noise_ar(ctx.handle, None, 0) == 0 and _same(draw(), indep)
    assert arm() == 0 and arm(n=0) == 0 and _same(draw(), indep)
    # entries that do not draw leave it alone
    assert arm() == 0
    fc.predict(*m.args(), floor=m.floor, extra_future=m.extra)
    fc.predict_components(*m.args(), floor=m.floor, extra_future=m.extra)
    assert _same(draw(), draws)
    # N != n fails with a message and clears
    assert arm(phi[:-1]) == 0
    with pytest.raises(_lib.TsfError, match='tsf_set_noise_ar was given 5 series'):
        draw()
    assert _same(draw(), indep)
    # a bad value is refused, and nothing is pending afterwards
    for bad, why in (([0.1, 1.0], 'phi[1]'), ([-1.0], 'phi[0]'), ([0.2, 0.3, np.nan], 'phi[2]'), ([np.inf], 'phi[0]'),
                     ([0.5, -1.5], 'phi[1]')):
        assert arm() == 0
        assert arm(bad) < 0 and why in message(), (why, message())
        assert _same(draw(), indep)
    with pytest.raises(ValueError, match='noise_ar'):
        _samples(fc, m, 300, noise_ar=np.full(N, 1.0))
    with pytest.raises(ValueError, match='noise_ar'):
        _samples(fc, m, 300, noise_ar=phi[:-1])
    # a failed taking call consumes it too
    assert arm() == 0
    with pytest.raises(_lib.TsfError, match='n_samples'):
        fc.predict_quantiles(*m.args(), [0.5], uncertainty_samples=1, seed=SEED, **m.kw())
    assert _same(draw(), indep)

    # every other entry that draws refuses while a setting is pending, clears it, and the context stays usable
    from time_series_spark_amd import synth
    T = 120
    ds = synth.daily_grid(T)
    y = 50.0 + np.random.default_rng(4).standard_normal((N, T))
    day = synth.DAY_NS
    spec_cv = fc.ModelSpec(growth='linear', n_changepoints=2, seasonalities=[])
    group = np.array([0, 1, 0, 1, 0, 2], dtype=np.int64)
    add_args = (m.spec, m.theta, m.y_scale, m.grid, group, m.keys)
    add_kw = dict(floor=m.floor, extra_future=m.extra)
    with fc.Rollup(m.fut, 3, uncertainty_samples=300, seed=SEED) as plain, \
            fc.Rollup(m.fut, 3, uncertainty_samples=300, seed=SEED, noise_corr=[0.5, 0.5, 0.5]) as corr:
        plain.add(*add_args, **add_kw)
        before = plain.samples()
        tkeys = 10 ** 9 + np.arange(3, dtype=np.int64)
        refusing = (
            lambda: fc.predict_components(*m.args(), floor=m.floor, extra_future=m.extra, series_key=m.keys, intervals=True,
                                          uncertainty_samples=300, seed=SEED),
            lambda: fc.cross_validate(spec_cv, ds, y, 14 * day, intervals=True, uncertainty_samples=50),
            lambda: fc.calibrate(spec_cv, ds, y, 14 * day, [0.8], mode='cqr', uncertainty_samples=50, interval_width=0.8),
            lambda: plain.set_totals(m.spec, m.theta[:3], m.y_scale[:3], m.grid, np.arange(3), tkeys, floor=m.floor[:3],
                                     extra_future=m.extra),
            lambda: plain.reconcile(*add_args, np.full(N, 0.5), quantiles=[0.5], **add_kw),
            lambda: corr.add(*add_args, **add_kw),
        )
        for i, call in enumerate(refusing):
            assert arm() == 0
            with pytest.raises(_lib.TsfError, match='pending'):
                call()
            assert _same(draw(), indep), i                         # cleared
        assert _same(plain.samples(), before)
        # the refused handles go on: the correlated add lands, a wrong count leaves the plain handle usable
        corr.add(*add_args, **add_kw)
        assert arm(phi[:-1]) == 0
        with pytest.raises(_lib.TsfError, match='tsf_set_noise_ar was given'):
            plain.add(*add_args, **add_kw)
        assert _same(plain.samples(), before)
        plain.add(*add_args, **add_kw)
        want = before.copy()
        for n in range(N):                                         # (the members land one at a time, in list order)
            want[group[n]] = want[group[n]] + indep[n]
        assert _same(plain.samples(), want)
        # the host layer's own refusals
        with pytest.raises(ValueError, match='noise_corr'):
            corr.add(*add_args, noise_ar=phi, **add_kw)
    with pytest.raises(ValueError, match='noise_corr'):
        fc.predict_rollup(m.spec, m.theta, m.y_scale, m.grid, m.fut, group, [0.5], m.keys, noise_corr=[0.5] * 3, noise_ar=phi,
                          **add_kw)
    unsorted = m.fut.copy()
    unsorted[[3, 4]] = unsorted[[4, 3]]
    tied = m.fut.copy()
    tied[4] = tied[3]
    for fut in (unsorted, tied, np.tile(unsorted, (N, 1))):
        with pytest.raises(ValueError, match='strictly increasing'):
            fc.predictive_samples(m.spec, m.theta, m.y_scale, m.grid, fut, uncertainty_samples=300, noise_ar=phi,
                                  floor=m.floor, extra_future=m.extra if fut.ndim == 1 else np.tile(m.extra, (N, 1, 1)))
    assert _same(draw(), indep)

    # the estimator's refusals: before any launch, nothing written, the context usable
    y2, f2 = _estimator_panel(70, np.float64)
    est0 = fc.residual_autocorrelation(y2, f2)
    p = lambda v: None if v is None else v.ctypes.data     # noqa: E731
    bufs = dict(phi=np.full(N_EST, 7.0), phi_raw=np.zeros(N_EST), n_pairs=np.zeros(N_EST, np.int64), scale=np.zeros(N_EST),
                status=np.full(N_EST, 7, np.int32))
    dec = np.array([0, 70, 60] + [70 * i for i in range(3, N_EST + 1)], dtype=np.int64)
    off1 = np.arange(N_EST + 1, dtype=np.int64) * 70 + 1

    def est(N=N_EST, T=70, offsets=None, y=y2, dtype=_lib.Y_F64, fitted=f2, phi_max=0.95, min_pairs=8, want=EST_FIELDS, out=True):
        a = _lib.TsfArArgs(phi_max, min_pairs, 0)
        o = _lib.TsfArOut(**{k: bufs[k].ctypes.data for k in want})
        return L.tsf_residual_autocorr(ctx.handle, N, T, p(offsets), p(y), dtype, p(fitted), ctypes.byref(a),
                                       ctypes.byref(o) if out else None)

    for kw, why in ((dict(out=False), 'NULL'), (dict(want=('phi_raw', 'status')), 'phi'), (dict(want=('phi',)), 'status'),
                    (dict(y=None), 'NULL'), (dict(fitted=None), 'NULL'), (dict(dtype=3), 'y_dtype'), (dict(dtype=-1), 'y_dtype'),
                    (dict(phi_max=1.0), 'phi_max'), (dict(phi_max=-0.1), 'phi_max'), (dict(phi_max=float('nan')), 'phi_max'),
                    (dict(min_pairs=0), 'min_pairs'), (dict(T=0), 'T'), (dict(offsets=dec), 'offsets'),
                    (dict(offsets=off1), 'offsets'), (dict(N=-1), 'N')):
        rc = est(**kw)
        assert rc < 0, why
        assert why in message(), (why, message())
    assert (bufs['phi'] == 7.0).all() and (bufs['status'] == 7).all()          # nothing was written
    assert est(N=0, y=None, fitted=None) == 0                                  # a legal no-op
    assert (bufs['phi'] == 7.0).all()
    assert est(want=('phi', 'status')) == 0 and _same(bufs['phi'], est0.phi)
    with pytest.raises(ValueError, match='phi_max'):
        fc.residual_autocorrelation(y2, f2, phi_max=1.0)
    with pytest.raises(ValueError, match='min_pairs'):
        fc.residual_autocorrelation(y2, f2, min_pairs=0)
    with pytest.raises(ValueError, match='fitted'):
        fc.residual_autocorrelation(y2, f2[:, :-1])
    _check_estimate(fc.residual_autocorrelation(y2, f2), {k: getattr(est0, k) for k in EST_FIELDS})


# ---- 7. plain C ----------------------------------------------------------------------------------------------------------

def test_abi_noise_ar_plain_c(env, tmp_path):
    """tests/c/abi_noise_ar.c drives tsf_residual_autocorr / tsf_set_noise_ar / tsf_predict_quantiles from plain C99 and
    writes what they return"""
    fc, _lib = env
    N, Hc, T = 7, 5, 40
    c = sc.make('no_cp')
    theta, ys = np.ascontiguousarray(c.theta[:N]), np.where(np.arange(N) % 2 == 0, 250.0, 60.0)
    grid = np.repeat(c.grid, N)
    fut, extra = np.ascontiguousarray(c.fut[:Hc]), np.ascontiguousarray(c.extra[:, :Hc])
    keys = 7919 * np.arange(N, dtype=np.int64) + 3
    rng = np.random.default_rng(9)
    fitted = 50.0 + rng.normal(0, 5, (N, T))
    y = fitted + np.stack([ar.chain(rng.standard_normal(T), p_) for p_ in np.linspace(0.2, 0.9, N)])
    p = str(tmp_path)
    for name, v in (('theta.f64', theta), ('ys.f64', ys), ('grid.bin', grid), ('extra.f64', extra), ('fut.i64', fut),
                    ('key.i64', keys), ('y.f64', y), ('fitted.f64', fitted)):
        np.ascontiguousarray(v).tofile(os.path.join(p, name))
    exe = p + '/abi_noise_ar'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_noise_ar.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(N), str(Hc), str(T), p])
    got = np.fromfile(p + '/out.f64')
    est = fc.residual_autocorrelation(y, fitted)
    assert (est.status == _lib.AR_OK).all() and est.phi.max() > 0.3
    lv = [0.1, 0.5, 0.9]
    want = [est.phi, est.phi_raw, est.scale]
    for noise_ar in (est, None):
        r = fc._predict_quantiles_call(c.spec, theta, ys, grid, fut, None, None, extra, keys, 50, 5, lv,
                                       ['q', 'cum_q', 'samples'], None, noise_ar=noise_ar)
        want += [r['yhat'].ravel(), r['q'].ravel(), r['cum_q'].ravel(), r['samples'].ravel()]
    want = np.concatenate(want)
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0
    per_call = N * Hc * (1 + 6 + 50)
    assert not np.array_equal(got[3 * N:3 * N + per_call], got[3 * N + per_call:])
    assert np.array_equal(np.fromfile(p + '/ints.i64', dtype=np.int64), np.concatenate([est.n_pairs, est.status]))


# ---- 8. end to end through forecaster ------------------------------------------------------------------------------------

def test_end_to_end(env):
    """64 series x 400 days with AR(1) residuals planted at 0.6 and 28 held-back days: fit_aligned ->
    fit_residual_autocorrelation -> predict_windows(y_obs=, noise_ar=) over four weeks.

    The band of the estimate.  In sample the fit removes p = 13 directions from the residuals (k, m, 5 changepoints, 6
    weekly columns), the low-frequency ones among them, where an AR(1) of phi = 0.6 has up to (1 + phi) / (1 - phi) = 4
    times its average variance: at most the share s = 4 p / T = 0.13 of ss, and of C no more than that share of ss, so
    E[phi_raw] >= (phi - s) / (1 - s) - 2 phi / T = 0.457.  A series' own estimate has standard error
    sqrt((1 - phi^2) / T) = 0.04 and the mean over n series that over sqrt(n); both bands are Z_MAX of them wide.  From
    above the planted value bounds the mean (the fit can only remove).  The direction of the intervals: every weekly
    total's P10-P90 is wider than the independent one's for every series with phi > 0; no coverage number is asserted."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N, T, Hf, PHI = 64, 400, 28, 0.6
    rng = np.random.default_rng(41)
    ds_all = synth.daily_grid(T + Hf)
    t = np.arange(T + Hf)
    resid = ar.synth_ar1(rng, N, T + Hf, PHI, sd=3.0)
    y_all = (100.0 + rng.uniform(0.0, 0.1, (N, 1)) * t + 5.0 * np.sin(2 * np.pi * t / 7.0 + rng.uniform(0, 6, (N, 1))) + resid)
    ds, y, fut, y_obs = ds_all[:T], np.ascontiguousarray(y_all[:, :T]), ds_all[T:], np.ascontiguousarray(y_all[:, T:])
    spec = fc.ModelSpec(growth='linear', n_changepoints=5,
                        seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3, 'mode': 'additive'}])
    res = fc.fit_aligned(spec, ds, y)
    # a series whose fit failed (line-search failures on residuals this persistent: Prophet would raise) takes no part, as
    # a caller would treat it; the bands below are as wide as the number that remain makes them
    ok = res.status > 0
    n_ok = int(ok.sum())
    print('fitted', n_ok, 'of', N)
    assert n_ok >= N // 4
    est = fc.fit_residual_autocorrelation(spec, res, ds, y)
    raw = est.phi_raw[ok]
    se = math.sqrt((1.0 - PHI * PHI) / T)
    s = 4.0 * 13 / T
    low = (PHI - s) / (1.0 - s) - 2.0 * PHI / T
    print('phi_raw: mean %.4f, min %.4f, max %.4f; band of the mean [%.4f, %.4f)' %
          (raw.mean(), raw.min(), raw.max(), low - sr.Z_MAX * se / math.sqrt(n_ok), PHI))
    assert (est.status[ok] == _lib.AR_OK).all() and (est.n_pairs[ok] == T - 1).all()
    assert low - sr.Z_MAX * se / math.sqrt(n_ok) <= raw.mean() < PHI
    assert (raw >= low - sr.Z_MAX * se).all() and (raw <= PHI + sr.Z_MAX * se).all()
    assert _same(est.phi[ok], np.clip(raw, 0.0, 0.95))
    w = fc.row_windows(Hf, 7)
    keys = np.arange(N, dtype=np.int64) + 1000
    width = []
    for noise_ar in (None, est.phi[ok]):
        r = fc.predict_windows(spec, res.theta[ok], res.y_scale[ok], res.grid, fut, w, [0.1, 0.9], y_obs=y_obs[ok],
                               series_key=keys[ok], uncertainty_samples=1000, seed=3, noise_ar=noise_ar)
        assert r.q.shape == (n_ok, 2, 4) and np.isfinite(r.pit).all()
        width.append(r.q[:, 1] - r.q[:, 0])
    pos = est.phi[ok] > 0
    assert pos.all() and (width[1][pos] > width[0][pos]).all()
    print('width ratio: mean %.3f, min %.3f' % ((width[1] / width[0]).mean(), (width[1] / width[0]).min()))
