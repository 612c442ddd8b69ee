"""GPU tests of the conditioned start of the AR(1) noise chain (include/tsf.h "the conditioned start"):
tsf_residual_last / _dev (ar_last_kernel) bit for bit against tests/ar_start_ref.py, the conditioned draw
(ar_start_shift_kernel and the third instance of interval_sample_kernel) bit for bit on a unit model, against the
restated streams on general models, against its laws, and through every consumer of the draws; the order and one-shot
rules with every refusal; a C99 caller; the corrected point forecast end to end.

Thresholds of the statistics: tests/sampler_ref.py's Z_MAX = 5.5 and P_MIN = 1e-7 (derived there, not measured).  Seeds,
keys, autocorrelations, residuals and step counts are fixed here; they are not to be tuned after a look at a result."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ar_ref as ar, ar_start_ref as ars, helpers, sampler_cases as sc, sampler_ref as sr, score_ref, window_ref

pytestmark = pytest.mark.gpu

SEED = 20241021


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


# ---- 1. tsf_residual_last, bit for bit -----------------------------------------------------------------------------------

LAST_FIELDS = ('last_resid', 'last_gap', 'status')
N_LAST = 12


def _last_panel(T, dtype, seed=31):
    """12 series of T rows.  Absent rows are NaN in fitted (every dtype has them there) and, in series 4, in y where the
    dtype has a NaN: series 1 the last row, 2 the last 65 rows (all of a shorter series), 3 every row, 4 the last row
    through y, 5 the last 64 rows, 6 every row but the first, 7 the last but one row (the final row is present)"""
    rng = np.random.default_rng(seed)
    fitted = 100.0 + 10.0 * rng.standard_normal((N_LAST, T))
    y = fitted + rng.standard_normal((N_LAST, T)) * rng.uniform(1.0, 30.0, (N_LAST, 1))
    y = np.rint(y).astype(np.int32) if dtype == np.int32 else y.astype(dtype)
    fitted[1, -1:] = np.nan
    fitted[2, -65:] = np.nan
    fitted[3, :] = np.nan
    if dtype != np.int32:
        y[4, -1] = np.nan
    else:
        fitted[4, -1] = np.inf
    fitted[5, -64:] = np.nan
    fitted[6, 1:] = np.nan
    if T > 1:
        fitted[7, -2] = np.nan
    return y, fitted


def _check_last(got, want):
    for k, g in zip(LAST_FIELDS, got):
        assert _same(g, want[k]), (k, g, want[k])


@pytest.mark.parametrize('T', [1, 2, 64, 65, 129])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32], ids=['f64', 'f32', 'i32'])
def test_residual_last_bit_for_bit_aligned(env, dtype, T):
    fc, _lib = env
    y, fitted = _last_panel(T, dtype)
    got = fc.residual_last(y, fitted)
    want = ars.residual_last(y, fitted)
    _check_last(got, want)
    resid, gap, status = got
    assert status[0] == _lib.AR_OK and gap[0] == 0 and resid[0] == float(y[0, -1]) - fitted[0, -1]
    assert status[3] == _lib.AR_NO_ROW == -52 and gap[3] == T and resid[3] == 0.0 and not np.signbit(resid[3])
    assert gap[1] == min(1, T) and gap[2] == min(65, T) and gap[5] == min(64, T) and gap[6] == T - 1 and gap[7] == 0
    assert status[2] == (_lib.AR_OK if T > 65 else _lib.AR_NO_ROW) and status[5] == (_lib.AR_OK if T > 64 else _lib.AR_NO_ROW)
    # residual_autocorrelation carries the same values
    est = fc.residual_autocorrelation(y, fitted)
    assert _same(est.last_resid, resid) and _same(est.last_gap, gap) and est.last_ds_ns is None
    assert list(est.frame(last=True).columns[-2:]) == ['last_resid', 'last_gap']


@pytest.mark.parametrize('dtype', [np.float64, np.int32], ids=['f64', 'i32'])
def test_residual_last_bit_for_bit_ragged(env, dtype):
    """lengths at the block edges, an empty series and a one-row series among them"""
    fc, _lib = env
    lens = [129, 0, 1, 200, 65, 2, 63, 128, 9, 130, 8, 64]
    y2, f2 = _last_panel(200, dtype)
    y = np.concatenate([y2[i, :n] for i, n in enumerate(lens)])
    fitted = np.concatenate([f2[i, :n] for i, n in enumerate(lens)])
    fitted[129 + 0 + 1 + 200 + 65 - 1] = np.nan                   # (series 4, 65 rows: its last row absent)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    got = fc.residual_last(y, fitted, offsets=offsets)
    _check_last(got, ars.residual_last(y, fitted, offsets))
    assert got[2][1] == _lib.AR_NO_ROW and got[1][1] == 0 and got[2][2] == _lib.AR_OK and got[1][2] == 0 and got[1][4] == 1
    none = fc.residual_last(np.zeros(0), np.zeros(0), offsets=np.zeros(4, np.int64))
    assert (none[2] == _lib.AR_NO_ROW).all() and not none[1].any() and not none[0].any()
    empty = fc.residual_last(np.zeros((0, 40)), np.zeros((0, 40)))
    assert empty[0].shape == (0,)


def test_residual_last_dev_variant_and_refusals(env):
    """tsf_residual_last_dev on device pointers (plain hipMalloc blocks; offsets on the host) == the host variant; the
    refusals come before any launch and write nothing"""
    fc, _lib = env
    from tests.test_gpu_screen import _hip_runtime
    hip = _hip_runtime()
    L = _lib.load()
    lens = [129, 0, 1, 200, 65, 2, 63, 128, 9, 130, 8, 64]
    y2, f2 = _last_panel(200, np.float64)
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
            want = fc.residual_last(y, fitted, offsets=off)
            host = dict(last_resid=np.full(N_LAST, 7.0), last_gap=np.full(N_LAST, 7, np.int32), status=np.full(N_LAST, 7, np.int32))
            d_y, d_f = dev(y), dev(fitted)
            o = {k: dev(v) for k, v in host.items()}
            out = _lib.TsfArLastOut(*[o[k] for k in LAST_FIELDS])
            ctx.check(L.tsf_residual_last_dev(ctx.handle, N_LAST, T, None if off is None else off.ctypes.data, d_y, _lib.Y_F64,
                                              d_f, ctypes.byref(out), None))
            assert hip.hipDeviceSynchronize() == 0
            for k, v in host.items():
                assert hip.hipMemcpy(v.ctypes.data, o[k], v.nbytes, 2) == 0         # hipMemcpyDeviceToHost
            for k, w in zip(LAST_FIELDS, want):
                assert _same(host[k], w), k
    finally:
        for p_ in bufs:
            hip.hipFree(p_)
    # refusals
    p = lambda v: None if v is None else v.ctypes.data     # noqa: E731
    hb = dict(last_resid=np.full(N_LAST, 7.0), last_gap=np.full(N_LAST, 7, np.int32), status=np.full(N_LAST, 7, np.int32))
    dec = np.array([0, 70, 60] + [70 * i for i in range(3, N_LAST + 1)], dtype=np.int64)
    off1 = np.arange(N_LAST + 1, dtype=np.int64) * 70 + 1
    y70, f70 = _last_panel(70, np.float64)

    def last(N=N_LAST, T=70, offsets=None, y=y70, dtype=_lib.Y_F64, fitted=f70, want=LAST_FIELDS, out=True):
        o = _lib.TsfArLastOut(**{k: hb[k].ctypes.data for k in want})
        return L.tsf_residual_last(ctx.handle, N, T, p(offsets), p(y), dtype, p(fitted), ctypes.byref(o) if out else None)

    for kw, why in ((dict(out=False), 'NULL'), (dict(want=('last_gap', 'status')), 'last_resid'),
                    (dict(want=('last_resid', 'status')), 'last_gap'), (dict(want=('last_resid', 'last_gap')), 'status'),
                    (dict(y=None), 'NULL'), (dict(fitted=None), 'NULL'), (dict(dtype=3), 'y_dtype'), (dict(dtype=-1), 'y_dtype'),
                    (dict(T=0), 'T'), (dict(offsets=dec), 'offsets'), (dict(offsets=off1), 'offsets'), (dict(N=-1), 'N')):
        assert last(**kw) < 0, why
        assert why in L.tsf_last_error(ctx.handle).decode(), why
    assert (hb['last_resid'] == 7.0).all() and (hb['status'] == 7).all()      # nothing was written
    assert last(N=0, y=None, fitted=None) == 0 and (hb['last_gap'] == 7).all()   # a legal no-op
    assert last() == 0 and _same(hb['last_resid'], fc.residual_last(y70, f70)[0])
    with pytest.raises(ValueError, match='fitted'):
        fc.residual_last(y70, f70[:, :-1])


# ---- the models of the draw tests (test_gpu_noise_ar.py's, restated) ---------------------------------------------------------

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


def _case_model(name, N):
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


def _yhat(fc, m, S, seed=SEED, noise_ar=None):
    """the yhat of a drawing call (predictive_samples returns the draws; predict_quantiles the point forecast beside them)"""
    return fc.predict_quantiles(*m.args(), [0.5], uncertainty_samples=S, seed=seed, noise_ar=noise_ar, **m.kw()).yhat


# ---- 2. the conditioned chain, bit for bit, on a unit model ----------------------------------------------------------------

UNIT_PHI = np.array([0.0, 0.3, 0.6, 0.95, -0.5])


@pytest.fixture(scope='module')
def unit(env):
    fc, _lib = env
    assert fc.selftest_math(2, np.zeros(1))[0] == 1.0           # the library's exp(0): sigma = 1 exactly
    m = _unit_model(5, 9)
    indep = _samples(fc, m, 300)
    assert not indep['trend'].any() and not np.signbit(indep['trend']).any()
    return m, indep, _yhat(fc, m, 300)


@pytest.mark.parametrize('steps', [1, 4])
@pytest.mark.parametrize('resid', [0.0, 1.5, -2.0])
def test_conditioned_chain_bit_for_bit_on_the_unit_model(env, unit, resid, steps):
    """300 samples (a full block of 256 and a partial one), 9 rows, five series: row h of every sample is numpy's
    (0 + (yhat + m_h)) + e_h of the independent call's own normals, yhat is yhat + m_h"""
    fc, _lib = env
    m, indep, yhat0 = unit
    z = indep['yhat']
    cond = fc.NoiseARStart(UNIT_PHI, np.full(5, resid), np.full(5, steps))
    got = _samples(fc, m, 300, noise_ar=cond)
    yhat = _yhat(fc, m, 300, noise_ar=cond)
    assert _same(got['trend'], indep['trend'])
    for n, phi in enumerate(UNIT_PHI):
        want_yhat, want = ars.draw(z[n], phi, resid, steps, base=yhat0[n])
        assert _same(got['yhat'][n], want), phi
        assert _same(yhat[n], want_yhat), phi
    # phi = 0: the call without any setting, bit for bit, whatever resid is
    assert _same(got['yhat'][0], z[0]) and _same(yhat[0], yhat0[0])
    if resid == 0.0 and steps == 1:
        # against the stationary chain: row 0 differs by exactly the factor c0, and later rows carry it on
        stat = _samples(fc, m, 300, noise_ar=UNIT_PHI)['yhat']
        for n in range(1, 5):
            c0 = float(ar.noise_c(UNIT_PHI[n]))
            assert _same(got['yhat'][n][0], c0 * stat[n][0]) and not _same(got['yhat'][n][1], stat[n][1])
        assert _same(yhat, yhat0)
    # predict(noise_ar=) is the drawing call's yhat
    assert _same(fc.predict(*m.args(), floor=m.floor, extra_future=m.extra, noise_ar=cond), yhat)


def test_conditioned_object(env):
    fc, _lib = env
    est = fc.NoiseAR(UNIT_PHI, None, None, None, None, last_resid=np.arange(5.0), last_gap=np.array([0, 1, 0, 2, 0], np.int32))
    c = est.conditioned()
    assert _same(c.steps, np.array([1, 2, 1, 3, 1], np.int32)) and _same(c.resid, np.arange(5.0)) and c.last_ds_ns is None
    assert _same(est.conditioned(lead=3).steps, np.array([3, 4, 3, 5, 3], np.int32))
    assert _same(est.conditioned(lead=np.array([1, 1, 2, 1, 1])).steps, np.array([1, 2, 2, 3, 1], np.int32))
    for bad in (0, [1, 1], 1.5):
        with pytest.raises(ValueError, match='lead'):
            est.conditioned(lead=bad)
    with pytest.raises(ValueError, match='last_resid'):
        fc.NoiseAR(UNIT_PHI, None, None, None, None).conditioned()
    with pytest.raises(ValueError, match='steps'):
        fc.NoiseARStart(UNIT_PHI, np.zeros(5), np.zeros(5, np.int32))
    with pytest.raises(ValueError, match='resid'):
        fc.NoiseARStart(UNIT_PHI, np.full(5, np.nan), np.ones(5, np.int32))


# ---- 3. general models against the restated streams ------------------------------------------------------------------------

GEN_PHI = np.array([0.0, 0.3, 0.6, 0.9, -0.5, 0.6])
GEN_STEPS = np.array([1, 1, 3, 1, 2, 1], np.int32)
GEN_R = np.array([2.0, 2.0, -2.0, 1.0, 2.0, -2.0])           # the last residual in units of sigma * y_scale
TOL = 1.25e-11


@pytest.mark.parametrize('name', ['lin_mul_s16', 'logistic_s3'])
def test_draw_against_the_restatement(env, name):
    """yhat_cond - yhat_indep against m_h + ((e - z) sigma) y_scale with z restated from sampler_ref's streams (numpy's
    log and cos), e its conditioned chain and m_h the reference's mean rows, within 1.25e-11; the point forecast moves
    by m_h within the same; the sampled trend is bit-identical with and without."""
    fc, _lib = env
    N, S = 6, 300
    m = _case_model(name, N)
    sig, ys = m.sampler.sigma, m.sampler.y_scale
    resid = GEN_R * sig * ys
    cond = fc.NoiseARStart(GEN_PHI, resid, GEN_STEPS)
    indep, got = _samples(fc, m, S), _samples(fc, m, S, noise_ar=cond)
    assert _same(got['trend'], indep['trend'])
    H = len(m.fut)
    knz = sr.stream_key(SEED, np.repeat(m.keys, S), np.tile(np.arange(S, dtype=np.int64), N), 1).reshape(N, 1, S)
    h2 = (2 * np.arange(H, dtype=np.uint64)).reshape(1, H, 1)
    z = sr.box_muller(sr.u01(knz, h2), sr.u01(knz, h2 + np.uint64(1)))
    _, c0, _ = ars.start_constants(GEN_PHI, resid, GEN_STEPS)
    e = np.stack([ars.chain(z[n], GEN_PHI[n], c0[n]) for n in range(N)])
    mean = ars.mean_rows(GEN_PHI, resid, GEN_STEPS, H)
    mean[GEN_PHI == 0.0] = 0.0
    want = mean[:, :, None] + ((e - z) * sig) * ys
    err = np.abs((got['yhat'] - indep['yhat']) - want).max()
    yerr = np.abs((_yhat(fc, m, S, noise_ar=cond) - _yhat(fc, m, S)) - mean).max()
    print('%s: largest deviation of the draws %.3g, of yhat %.3g, tolerance %.3g, largest term %.3g'
          % (name, err, yerr, TOL, np.abs(want).max()))
    assert np.abs(want).max() > sig * ys
    assert err <= TOL and yerr <= TOL
    assert _same(got['yhat'][0], indep['yhat'][0])


# ---- 4. laws on the device ---------------------------------------------------------------------------------------------------

_n = np.arange(sc.N)
LAW_PHI = np.where(_n < sc.N // 2, 0.6, 0.3)
LAW_STEPS = np.where(_n % 2 == 0, 1, 3).astype(np.int32)
LAW_R = np.where(_n % 4 < 2, 2.0, -2.0)
LAW_GROUPS = [(phi, steps, r, np.flatnonzero((LAW_PHI == phi) & (LAW_STEPS == steps) & (LAW_R == r)))
              for phi in (0.6, 0.3) for steps in (1, 3) for r in (2.0, -2.0)]


def _law_draw(fc, seed, noise_ar):
    """(x, center): the draws [N][H][S] of the noise-only case ('no_cp': its sampled trend is the deviation itself at
    lam = 1e-8, nine orders below the noise) less the sampled trend's and the additive piece, and the drawing call's
    yhat less the independent call's, both in units of sigma * y_scale"""
    m = _case_model('no_cp', sc.N)
    s = m.sampler
    d = _samples(fc, m, sc.NS, seed=seed, noise_ar=noise_ar)
    x = (d['yhat'] - d['trend'] * s.opm[None, :, None] - s.xa[None, :, None]) / (s.sigma * s.y_scale)
    center = (_yhat(fc, m, 2, seed=seed, noise_ar=noise_ar) - _yhat(fc, m, 2, seed=seed)) / (s.sigma * s.y_scale)
    return m, x, center


def _law_stats(x, center):
    out = []
    for phi, steps, r, idx in LAW_GROUPS:
        assert len(idx) == 8
        rows = np.ascontiguousarray(x[idx].transpose(1, 0, 2)).reshape(sc.H, -1)
        assert np.abs(center[idx] - center[idx[0]]).max() <= 1e-13
        out.append(((phi, steps, r), ars.start_law_stats(rows, center[idx[0]], phi, r, steps)))
    return out


@pytest.mark.parametrize('seed_i', [0, 1])
def test_conditioned_draws_follow_their_laws(env, seed_i):
    """64 series x 4 096 samples x 32 rows: eight groups of eight series (phi 0.6 / 0.3, steps 1 / 3, the last residual
    at +- 2 sigma y_scale), 18 statistics each"""
    fc, _lib = env
    m = _case_model('no_cp', sc.N)
    cond = fc.NoiseARStart(LAW_PHI, LAW_R * m.sampler.sigma * m.sampler.y_scale, LAW_STEPS)
    _, x, center = _law_draw(fc, SEED + seed_i, cond)
    n_stats = 0
    for tag, res in _law_stats(x, center):
        _report('seed %d, phi %g steps %d r %g' % ((seed_i,) + tag), res)
        assert len(res) == 18 and not sr.failures(res), (tag, sr.failures(res))
        n_stats += len(res)
    assert n_stats == 8 * 18


def test_the_stationary_chain_fails_the_start_laws(env):
    """the companion: with the stationary chain of tsf_set_noise_ar alone the same statistics reject at row 0 -- the mean
    in every group (the least shift, 2 * 0.3^3 = 0.054 at 32 768 samples, is 9.8 standard errors), the point forecast in
    every group, the variance in the groups at steps = 1 (1 against 0.64 and 0.91: 72 and 12.7 standard errors; at
    steps = 3 and phi = 0.3 the variances differ by 7e-4, below what 32 768 samples resolve)"""
    fc, _lib = env
    _, x, center = _law_draw(fc, SEED, LAW_PHI)
    for (phi, steps, r), res in _law_stats(x, center):
        bad = [name for name, _, _ in sr.failures(res)]
        assert 'row 0: mean' in bad and 'row 0: yhat is the law\'s mean' in bad, (phi, steps, r, bad)
        if steps == 1:
            assert 'row 0: variance' in bad, (phi, steps, r, bad)


# ---- 5. consumers -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def general(env):
    """6 series of the multiplicative case on its 32 rows with mixed phi, steps and residuals, 300 samples: the
    conditioned draws, the independent ones, the conditioned object and the conditioned yhat"""
    fc, _lib = env
    m = _case_model('lin_mul_s16', 6)
    cond = fc.NoiseARStart(np.array([0.6, 0.0, 0.3, 0.9, -0.5, 0.6]), GEN_R * m.sampler.sigma * m.sampler.y_scale, GEN_STEPS)
    yhat = fc.predict(*m.args(), floor=m.floor, extra_future=m.extra, noise_ar=cond)
    return m, cond, _samples(fc, m, 300, noise_ar=cond)['yhat'], _samples(fc, m, 300)['yhat'], yhat


def test_quantiles_and_intervals_read_the_conditioned_draws(env, general):
    fc, _lib = env
    m, cond, draws, indep, yhat_c = general
    lv = [(1.0 - 0.8) / 2.0, 0.5, (1.0 + 0.8) / 2.0]           # (the levels predict_intervals forms at width 0.8)
    r = fc.predict_quantiles(*m.args(), lv, cumulative=True, uncertainty_samples=300, seed=SEED, noise_ar=cond, **m.kw())
    v = np.sort(draws, axis=-1)
    assert _same(r.q, np.stack([score_ref.quantile(v, p) for p in lv], axis=1))
    c = np.sort(window_ref.window_sums(draws, np.zeros(32, int), np.arange(1, 33)), axis=-1)
    assert _same(r.cum_q, np.stack([score_ref.quantile(c, p) for p in lv], axis=1))
    assert _same(r.yhat, yhat_c) and not _same(r.yhat[0], fc.predict(*m.args(), floor=m.floor, extra_future=m.extra)[0])
    yhat, lo, hi = fc.predict_intervals(*m.args(), uncertainty_samples=300, interval_width=0.8, seed=SEED, noise_ar=cond, **m.kw())
    assert _same(lo, r.q[:, 0]) and _same(hi, r.q[:, 2]) and _same(yhat, yhat_c)


def test_windows_sum_the_conditioned_draws(env, general):
    fc, _lib = env
    m, cond, draws, indep, yhat_c = general
    start, end = np.array([0, 3, 7, 25, 0], np.int32), np.array([7, 4, 21, 32, 32], np.int32)
    lv = [0.1, 0.5, 0.9]
    got = fc.predict_windows(*m.args(), fc.Windows(start, end), lv, uncertainty_samples=300, seed=SEED, noise_ar=cond, **m.kw())
    assert _same(got.q, window_ref.score(draws, None, lv, start, end)['q'])
    assert not _same(got.q, window_ref.score(indep, None, lv, start, end)['q'])


def test_scores_rank_against_the_conditioned_draws(env, general):
    fc, _lib = env
    m, cond, draws, indep, yhat_c = general
    y_obs = np.ascontiguousarray(np.median(indep, axis=-1) + 3.0 * np.cos(np.arange(32))[None, :])
    y_obs[2, 5] = np.nan
    got = fc.score_actuals(*m.args(), y_obs, quantiles=[0.1, 0.9], uncertainty_samples=300, seed=SEED, noise_ar=cond, **m.kw())
    want = score_ref.score(draws, y_obs, [0.1, 0.9])
    assert score_ref.same(got.pit, want['pit']) and score_ref.same(got.q, want['q'])
    assert not score_ref.same(got.pit, score_ref.score(indep, y_obs, [0.1, 0.9])['pit'])


def test_rollup_adds_the_conditioned_draws(env, general):
    """acc = +0.0 + the members' conditioned samples in list order, over two add calls (the second without a setting);
    ysum accumulates the shifted yhat"""
    fc, _lib = env
    m, cond, draws, indep, yhat_c = general
    group = np.array([0, 1, 0, 1, 0, 2], dtype=np.int64)
    first = slice(0, 4)
    part = fc.NoiseARStart(cond.phi[first], cond.resid[first], cond.steps[first])
    with fc.Rollup(m.fut, 3, uncertainty_samples=300, seed=SEED) as roll:
        roll.add(m.spec, m.theta[first], m.y_scale[first], m.grid, group[first], m.keys[first], floor=m.floor[first],
                 extra_future=m.extra, noise_ar=part)
        roll.add(m.spec, m.theta[4:], m.y_scale[4:], m.grid, group[4:], m.keys[4:], floor=m.floor[4:], extra_future=m.extra)
        got = roll.samples()
        ysum = roll.quantiles([0.5]).yhat
    yhat_i = fc.predict(*m.args(), floor=m.floor, extra_future=m.extra)
    want, want_y = np.zeros((3, 32, 300)), np.zeros((3, 32))
    for n in range(6):
        want[group[n]] = want[group[n]] + (draws[n] if n < 4 else indep[n])
        want_y[group[n]] = want_y[group[n]] + (yhat_c[n] if n < 4 else yhat_i[n])
    assert _same(got, want) and _same(ysum, want_y)
    uniq, r = fc.predict_rollup(m.spec, m.theta, m.y_scale, m.grid, m.fut, group, [0.5], m.keys, floor=m.floor,
                                extra_future=m.extra, uncertainty_samples=300, seed=SEED, noise_ar=cond)
    want, want_y = np.zeros((3, 32, 300)), np.zeros((3, 32))
    for n in range(6):
        want[group[n]] = want[group[n]] + draws[n]
        want_y[group[n]] = want_y[group[n]] + yhat_c[n]
    assert _same(r.q[:, 0], score_ref.quantile(np.sort(want, axis=-1), 0.5)) and _same(r.yhat, want_y)


def test_batch_chunk_and_sample_count_independence(env):
    """a series drawn alone, in a batch of 64 and at 300 against 4 096 samples: the same first 300 samples; 600 series
    at 4 096 samples with running sums (three chunks of the 512 MB scratch) against the same series in calls of 200"""
    fc, _lib = env
    m = _case_model('lin_mul_s16', 64)
    s = m.sampler
    rng = np.random.default_rng(3)
    cond = fc.NoiseARStart(np.linspace(-0.5, 0.9, 64), rng.normal(0, 2, 64) * s.sigma * s.y_scale, rng.integers(1, 5, 64))
    big = _samples(fc, m, 4096, noise_ar=cond)['yhat']
    small = _samples(fc, m, 300, noise_ar=cond)['yhat']
    assert _same(big[:, :, :300], small)
    del big
    one = _M()
    n = 37
    one.spec, one.grid, one.fut, one.extra, one.cap = m.spec, m.grid, m.fut, m.extra, None
    one.theta, one.y_scale, one.floor, one.keys = m.theta[n:n + 1], m.y_scale[n:n + 1], m.floor[n:n + 1], m.keys[n:n + 1]
    c1 = fc.NoiseARStart(cond.phi[n:n + 1], cond.resid[n:n + 1], cond.steps[n:n + 1])
    assert _same(_samples(fc, one, 300, noise_ar=c1)['yhat'][0], small[n])
    N = 600
    wide = _M()
    wide.spec, wide.grid, wide.fut, wide.extra, wide.cap = m.spec, m.grid, m.fut, m.extra, None
    wide.theta, wide.y_scale, wide.floor = np.tile(m.theta[:1], (N, 1)), np.tile(m.y_scale[:1], N), np.tile(m.floor[:1], N)
    wide.keys = 7919 * np.arange(N, dtype=np.int64) + 3
    cw = fc.NoiseARStart(rng.uniform(-0.5, 0.9, N), rng.normal(0, 2, N) * s.sigma * s.y_scale, rng.integers(1, 5, N))

    def quant(lo, hi):
        part = fc.NoiseARStart(cw.phi[lo:hi], cw.resid[lo:hi], cw.steps[lo:hi])
        return fc.predict_quantiles(wide.spec, wide.theta[lo:hi], wide.y_scale[lo:hi], wide.grid, wide.fut, [0.1, 0.9],
                                    cumulative=True, uncertainty_samples=4096, seed=SEED, noise_ar=part, floor=wide.floor[lo:hi],
                                    extra_future=wide.extra, series_key=wide.keys[lo:hi])
    whole = quant(0, N)
    for lo in (0, 200, 400):
        part = quant(lo, lo + 200)
        assert _same(whole.yhat[lo:lo + 200], part.yhat) and _same(whole.q[lo:lo + 200], part.q)
        assert _same(whole.cum_q[lo:lo + 200], part.cum_q)


# ---- 6. the order and one-shot rules, and every refusal -----------------------------------------------------------------------

def test_order_one_shot_rule_and_refusals(env, general):
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    m, cond, draws, indep, yhat_c = general
    N = len(cond.phi)
    stat = _samples(fc, m, 300, noise_ar=cond.phi)['yhat']

    def message():
        return L.tsf_last_error(ctx.handle).decode()

    def arm(p=cond.phi, n=None):
        p = np.ascontiguousarray(p, dtype=np.float64)
        return L.tsf_set_noise_ar(ctx.handle, p.ctypes.data, len(p) if n is None else n)

    def start(resid=cond.resid, steps=cond.steps, n=None):
        resid = np.ascontiguousarray(resid, dtype=np.float64)
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        return L.tsf_set_noise_ar_start(ctx.handle, resid.ctypes.data, steps.ctypes.data, len(resid) if n is None else n)

    def draw():
        return _samples(fc, m, 300)['yhat']

    # both settings are consumed by the next drawing entry; the call after it is the independent one
    assert arm() == 0 and start() == 0
    assert _same(draw(), draws) and _same(draw(), indep)
    # a start without a pending phi is refused
    assert start() < 0 and 'no tsf_set_noise_ar setting is pending' in message()
    assert _same(draw(), indep)
    # n mismatch: refused, and the pending phi is cleared with it
    assert arm() == 0 and start(cond.resid[:-1], cond.steps[:-1]) < 0 and 'was given 5 series' in message()
    assert _same(draw(), indep)
    # steps < 1 and a non-finite resid: refused, both cleared
    for kw, why in ((dict(steps=np.array([1, 1, 0, 1, 1, 1])), 'steps[2]'), (dict(steps=np.array([-3, 1, 1, 1, 1, 1])), 'steps[0]'),
                    (dict(resid=np.array([0, 0, 0, np.nan, 0, 0.0])), 'resid[3]'),
                    (dict(resid=np.array([0, np.inf, 0, 0, 0, 0.0])), 'resid[1]')):
        assert arm() == 0 and start(**kw) < 0 and why in message(), (why, message())
        assert _same(draw(), indep)
    # NULL or n == 0 clears the start only: the stationary chain is drawn
    assert arm() == 0 and start() == 0 and L.tsf_set_noise_ar_start(ctx.handle, None, None, 0) == 0
    assert _same(draw(), stat)
    assert arm() == 0 and start() == 0 and start(n=0) == 0 and _same(draw(), stat)
    # a new phi setting clears the start; clearing phi clears both
    assert arm() == 0 and start() == 0 and arm() == 0 and _same(draw(), stat)
    assert arm() == 0 and start() == 0 and L.tsf_set_noise_ar(ctx.handle, None, 0) == 0 and _same(draw(), indep)
    # entries that do not draw leave both alone
    assert arm() == 0 and start() == 0
    fc.predict(*m.args(), floor=m.floor, extra_future=m.extra)
    fc.predict_components(*m.args(), floor=m.floor, extra_future=m.extra)
    assert _same(draw(), draws)
    # a call with N != n fails and clears both
    five = _M()
    five.spec, five.grid, five.fut, five.extra, five.cap = m.spec, m.grid, m.fut, m.extra, None
    five.theta, five.y_scale, five.floor, five.keys = m.theta[:5], m.y_scale[:5], m.floor[:5], m.keys[:5]
    assert arm() == 0 and start() == 0
    with pytest.raises(_lib.TsfError, match='tsf_set_noise_ar was given 6 series'):
        _samples(fc, five, 300)
    assert _same(draw(), indep)
    # a failed taking call consumes both
    assert arm() == 0 and start() == 0
    with pytest.raises(_lib.TsfError, match='n_samples'):
        fc.predict_quantiles(*m.args(), [0.5], uncertainty_samples=1, seed=SEED, **m.kw())
    assert _same(draw(), indep)
    # an entry that refuses a pending setting clears both, and the context stays usable
    group = np.array([0, 1, 0, 1, 0, 2], dtype=np.int64)
    add_args = (m.spec, m.theta, m.y_scale, m.grid, group, m.keys)
    add_kw = dict(floor=m.floor, extra_future=m.extra)
    with fc.Rollup(m.fut, 3, uncertainty_samples=300, seed=SEED, noise_corr=[0.5, 0.5, 0.5]) as corr:
        refusing = (
            lambda: fc.predict_components(*m.args(), floor=m.floor, extra_future=m.extra, series_key=m.keys, intervals=True,
                                          uncertainty_samples=300, seed=SEED),
            lambda: corr.add(*add_args, **add_kw),
        )
        for i, call in enumerate(refusing):
            assert arm() == 0 and start() == 0
            with pytest.raises(_lib.TsfError, match='pending'):
                call()
            assert _same(draw(), indep), i
        with pytest.raises(ValueError, match='noise_corr'):
            corr.add(*add_args, noise_ar=cond, **add_kw)
    # the host layer: predict_temporal refuses a conditioned object before anything else is looked at
    with pytest.raises(ValueError, match='predict_temporal keeps the stationary start'):
        fc._temporal_phi(cond, N, m.fut, 'noise_ar')
    # future rows not after last_ds_ns
    for last_ds in (np.full(N, m.fut[0]), np.where(np.arange(N) == 4, m.fut[0] + 5, m.fut[0] - 1)):
        late = fc.NoiseARStart(cond.phi, cond.resid, cond.steps, last_ds_ns=last_ds)
        for call in (lambda: _samples(fc, m, 300, noise_ar=late),
                     lambda: fc.predict(*m.args(), floor=m.floor, extra_future=m.extra, noise_ar=late)):
            with pytest.raises(ValueError, match='after the history'):
                call()
    ok = fc.NoiseARStart(cond.phi, cond.resid, cond.steps, last_ds_ns=np.full(N, m.fut[0] - 1))
    assert _same(_samples(fc, m, 300, noise_ar=ok)['yhat'], draws)
    # predict: a phi alone does nothing to a point forecast, and the integer column is not corrected
    with pytest.raises(ValueError, match='conditioned'):
        fc.predict(*m.args(), floor=m.floor, extra_future=m.extra, noise_ar=cond.phi)
    with pytest.raises(ValueError, match='want_int'):
        fc.predict(*m.args(), floor=m.floor, extra_future=m.extra, noise_ar=cond, want_int=True)
    with pytest.raises(ValueError, match='noise_ar'):
        _samples(fc, m, 300, noise_ar=fc.NoiseARStart(cond.phi[:-1], cond.resid[:-1], cond.steps[:-1]))
    assert _same(draw(), indep)


def test_predict_temporal_refuses_a_conditioned_object(env, general):
    fc, _lib = env
    m, cond, draws, indep, yhat_c = general
    w = fc.row_windows(32, 8)
    args = (m.spec, m.theta, m.y_scale, m.grid, m.fut, w, m.spec, m.theta, m.y_scale, m.grid, m.fut[7::8], None, [0.5],
            m.keys, m.keys + 1)
    for kw in (dict(noise_ar=cond), dict(period_noise_ar=cond)):
        with pytest.raises(ValueError, match='stationary start'):
            fc.predict_temporal(*args, floor=m.floor, extra_future=m.extra, uncertainty_samples=50, **kw)


# ---- 7. plain C ----------------------------------------------------------------------------------------------------------------

def test_abi_ar_start_plain_c(env, tmp_path):
    """tests/c/abi_ar_start.c drives tsf_residual_last / tsf_noise_ar_mean / tsf_set_noise_ar_start /
    tsf_predict_quantiles from plain C99 and writes what they return"""
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
    y[2, -1] = np.nan
    y[5, -3:] = np.nan
    p = str(tmp_path)
    for name, v in (('theta.f64', theta), ('ys.f64', ys), ('grid.bin', grid), ('extra.f64', extra), ('fut.i64', fut),
                    ('key.i64', keys), ('y.f64', y), ('fitted.f64', fitted)):
        np.ascontiguousarray(v).tofile(os.path.join(p, name))
    exe = p + '/abi_ar_start'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_ar_start.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(N), str(Hc), str(T), p])
    got = np.fromfile(p + '/out.f64')
    est = fc.residual_autocorrelation(y, fitted)
    assert est.phi.max() > 0.3 and list(est.last_gap[[2, 5]]) == [1, 3]
    cond = est.conditioned()
    lv = [0.1, 0.5, 0.9]
    want = [est.phi, est.last_resid, ars.mean_rows(est.phi, est.last_resid, cond.steps, Hc).ravel()]
    for noise_ar in (cond, None):
        r = fc._predict_quantiles_call(c.spec, theta, ys, grid, fut, None, None, extra, keys, 50, 5, lv,
                                       ['q', 'cum_q', 'samples'], None, noise_ar=noise_ar)
        want += [r['yhat'].ravel(), r['q'].ravel(), r['cum_q'].ravel(), r['samples'].ravel()]
    want = np.concatenate(want)
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0
    per_call = N * Hc * (1 + 6 + 50)
    at = 2 * N + N * Hc
    assert not np.array_equal(got[at:at + per_call], got[at + per_call:])
    ints = np.fromfile(p + '/ints.i32', dtype=np.int32)
    assert np.array_equal(ints, np.concatenate([est.last_gap, np.zeros(N, np.int32), cond.steps]))


# ---- 8. end to end through forecaster --------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def planted(env):
    """tests/ar_start_ref.py's planted panel (256 x 200 + 8 held back, phi = 0.6) fitted by fit_aligned: linear growth,
    five changepoints, a weekly seasonality of order 3.  A series whose fit failed takes no part, as a caller would
    treat it."""
    fc, _lib = env
    from time_series_spark_amd import synth
    T, hold = ars.PLANT_T, ars.PLANT_HOLD
    t, y_all, X = ars.planted_panel(5)
    ds_all = synth.daily_grid(T + 32)
    ds, y = ds_all[:T], np.ascontiguousarray(y_all[:, :T])
    spec = fc.ModelSpec(growth='linear', n_changepoints=5,
                        seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3, 'mode': 'additive'}])
    res = fc.fit_aligned(spec, ds, y)
    ok = res.status > 0
    print('fitted', int(ok.sum()), 'of', len(ok))
    assert ok.sum() >= len(ok) // 4
    est = fc.fit_residual_autocorrelation(spec, res, ds, y)
    return spec, res, ds, y, ds_all[T:], y_all[:, T:], ok, est


def test_end_to_end_point_forecast(env, planted):
    """Measured on this panel (fit_aligned, 256 series): pooled squared error corrected / uncorrected and the mean
    estimated phi are printed; theory for an exact fit of the deterministic part is phi^2 removed at row 0 (0.64)."""
    fc, _lib = env
    spec, res, ds, y, fut, y_fut, ok, est = planted
    hold = ars.PLANT_HOLD
    assert (est.last_gap == 0).all() and (est.last_ds_ns == ds[-1]).all() and (est.status[ok] == _lib.AR_OK).all()
    assert list(est.frame(last=True).columns[-3:]) == ['last_resid', 'last_gap', 'last_ds_ns']
    cond = est.conditioned()
    yhat0 = fc.predict(spec, res.theta, res.y_scale, res.grid, fut[:hold])
    yhat1 = fc.predict(spec, res.theta, res.y_scale, res.grid, fut[:hold], noise_ar=cond)
    ratios = [float(((y_fut[ok, a:b] - yhat1[ok, a:b]) ** 2).sum() / ((y_fut[ok, a:b] - yhat0[ok, a:b]) ** 2).sum())
              for a, b in ((0, 1), (0, 3))]
    fitted = fc.fitted_history(spec, res, ds)
    assert _same(est.last_resid, y[:, -1] - fitted[:, -1])
    want, corrected = ars.accuracy_ratios(y[ok], fitted[ok], y_fut[ok, :hold], yhat0[ok], est.phi[ok])
    print('mean phi %.4f over %d series; pooled squared error corrected / uncorrected: row 0 %.4f, rows 0..2 %.4f'
          % (est.phi[ok].mean(), int(ok.sum()), ratios[0], ratios[1]))
    assert ratios[0] < 1.0 and ratios[1] < 1.0
    assert abs(ratios[0] - want[0]) <= 1e-9 and abs(ratios[1] - want[1]) <= 1e-9
    assert _same(yhat1[ok], corrected)
    with pytest.raises(ValueError, match='after the history'):
        fc.predict(spec, res.theta, res.y_scale, res.grid, ds[-3:], noise_ar=cond)


def test_width_of_the_first_row(env, planted):
    """P10 - P90 of 1 000 samples at row 0 and at row 31, conditioned against the stationary chain and the independent
    draw.  The bound.  The level-p quantile of n draws from a density f has standard error sqrt(p (1 - p) / n) / f(q_p)
    and two of them (p < q) the covariance p (1 - q) / (n f(q_p) f(q_q)); for a normal law at p = 0.1, q = 0.9,
    n = 1 000: f = 0.17550, each quantile 0.05406, their covariance 3.247e-4, the width (2.5631) a standard deviation of
    sqrt(2 * 0.05406^2 - 2 * 3.247e-4) = 0.07208, 2.812 % of itself.  A ratio of two widths, taken as independent (they
    are positively dependent here: the same normals and trend draws), has at most sqrt(2) times that, and the band is
    Z_MAX of them: 21.9 %."""
    fc, _lib = env
    spec, res, ds, y, fut, y_fut, ok, est = planted
    n, p = 1000, 0.1
    f = math.exp(-0.5 * 1.2815515655446004 ** 2) / math.sqrt(2.0 * math.pi)
    var = 2.0 * p * (1.0 - p) / (n * f * f) - 2.0 * p * p / (n * f * f)
    band = sr.Z_MAX * math.sqrt(2.0) * math.sqrt(var) / (2.0 * 1.2815515655446004)
    assert band == pytest.approx(0.2187, abs=1e-3)
    keys = np.arange(len(ok), dtype=np.int64)[ok] + 1000
    width = {}
    for tag, noise_ar in (('indep', None), ('stat', est.phi[ok]),
                          ('cond', fc.NoiseARStart(est.phi[ok], est.last_resid[ok], est.conditioned().steps[ok], est.last_ds_ns[ok]))):
        r = fc.predict_quantiles(spec, res.theta[ok], res.y_scale[ok], res.grid, fut, [0.1, 0.9], series_key=keys,
                                 uncertainty_samples=n, seed=3, noise_ar=noise_ar)
        width[tag] = r.q[:, 1] - r.q[:, 0]
    pos = est.phi[ok] > 0
    assert pos.any() and (width['cond'][pos, 0] < width['stat'][pos, 0]).all()
    c0 = np.sqrt(1.0 - est.phi[ok] ** 2)
    ratio = width['cond'][:, 0] / width['indep'][:, 0]
    far = width['cond'][:, 31] / width['stat'][:, 31]
    print('row 0: width / independent width over c0 in [%.4f, %.4f]; row 31: conditioned / stationary in [%.6f, %.6f]'
          % ((ratio / c0).min(), (ratio / c0).max(), far.min(), far.max()))
    assert (np.abs(ratio / c0 - 1.0) <= band).all()
    assert (np.abs(far - 1.0) <= band).all() and (np.abs(width['cond'][:, 31] / width['indep'][:, 31] - 1.0) <= band).all()
