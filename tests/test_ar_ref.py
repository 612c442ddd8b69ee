"""CPU tests of the reference for the serially correlated observation noise (tests/ar_ref.py): the restated estimator
recovers a planted autocorrelation (less its derived bias), NaN rows break pairs, and two subtly wrong estimators are
rejected; the restated chain obeys its laws at sampler_ref's thresholds and three subtly wrong chains are rejected at
the same thresholds.  tests/test_gpu_noise_ar.py holds the device against this reference."""
import math

import numpy as np
import pytest

from tests import ar_ref as ar, sampler_ref as sr

PHI = 0.6
N_SERIES, T_ROWS = 2000, 730


def _report(tag, results):
    for name, kind, value in results:
        print('%s    %-60s %s %.6g' % (tag, name, kind, value))


@pytest.fixture(scope='module')
def planted():
    r = ar.synth_ar1(np.random.default_rng(11), N_SERIES, T_ROWS, PHI, sd=3.0)
    r.setflags(write=False)
    return r


def _mean_z(raw, phi, T):
    """z of the mean of the raw estimates against phi less the derived bias 2 phi / T, at Bartlett's standard error"""
    return (raw.mean() - (phi - 2.0 * phi / T)) / math.sqrt((1.0 - phi * phi) / T / len(raw))


def test_wave_sum_is_the_partials_and_the_butterfly():
    rng = np.random.default_rng(3)
    for L in (0, 1, 63, 64, 65, 129, 730):
        x = rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)
        part = [0.0] * 64
        for i, v in enumerate(x):
            part[i % 64] = part[i % 64] + float(v)
        for d in (1, 2, 4, 8, 16, 32):
            part = [part[l] + part[l ^ d] for l in range(64)]
        assert ar.wave_sum(x) == part[0]
        assert len(set(part)) == 1          # (a + b commutes: every lane ends with the same bits)


def test_estimator_recovers_the_planted_autocorrelation(planted):
    res = ar.autocorr(planted, np.zeros_like(planted))
    assert (res['status'] == ar.AR_OK).all() and (res['n_pairs'] == T_ROWS - 1).all()
    raw = res['phi_raw']
    z = _mean_z(raw, PHI, T_ROWS)
    sd_law = math.sqrt((1.0 - PHI * PHI) / T_ROWS)
    print('mean %.5f sd %.5f (law %.5f) z %.3f; z without the bias term %.3f'
          % (raw.mean(), raw.std(), sd_law, z, (raw.mean() - PHI) / (sd_law / math.sqrt(len(raw)))))
    assert abs(z) <= sr.Z_MAX
    # the spread is the law's: a sample variance of N values, relative standard error sqrt(2 / (N - 1)) (its kurtosis is
    # that of a near-normal estimate at T = 730)
    assert abs(raw.var(ddof=1) / sd_law ** 2 - 1.0) <= sr.Z_MAX * math.sqrt(2.0 / (len(raw) - 1))
    np.testing.assert_array_equal(res['phi'], np.clip(raw, 0.0, 0.95))
    np.testing.assert_allclose(res['scale'], 3.0, rtol=0.25)


def test_fitted_is_subtracted_and_the_dtype_is_widened_first():
    rng = np.random.default_rng(5)
    r = ar.synth_ar1(rng, 3, 100, 0.5)
    fit = rng.standard_normal((3, 100)) * 5.0
    y32 = (r + fit).astype(np.float32)
    a = ar.autocorr(y32, fit)
    b = ar.autocorr(y32.astype(np.float64) - fit, np.zeros_like(fit))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_nan_rows_break_pairs():
    r = np.arange(1.0, 21.0)
    r[[4, 5, 12]] = np.nan
    phi, raw, npairs, scale, status = ar.autocorr_series(r, np.zeros(20), min_pairs=1)
    ok = np.isfinite(r)
    pairs = [(t - 1, t) for t in range(1, 20) if ok[t] and ok[t - 1]]
    assert npairs == len(pairs) == 19 - 5
    want = (sum(r[a] * r[b] for a, b in pairs) / len(pairs)) / (np.nansum(r * r) / ok.sum())
    assert raw == pytest.approx(want, rel=1e-14) and status == ar.AR_OK
    assert scale == pytest.approx(math.sqrt(np.nansum(r * r) / ok.sum()), rel=1e-14)
    # a NaN in fitted is a NaN residual as well
    fit = np.zeros(20)
    fit[8] = np.nan
    assert ar.autocorr_series(r, fit, min_pairs=1)[2] == npairs - 2


def test_too_few_pairs_and_zero_residuals():
    r = np.ones(9)
    assert ar.autocorr_series(r, np.zeros(9), min_pairs=8)[4] == ar.AR_OK
    phi, raw, npairs, scale, status = ar.autocorr_series(r, np.zeros(9), min_pairs=9)
    assert (phi, npairs, scale, status) == (0.0, 8, 1.0, ar.AR_NO_PAIRS) and math.isnan(raw)
    phi, raw, npairs, scale, status = ar.autocorr_series(r, r)
    assert (phi, npairs, status) == (0.0, 8, ar.AR_NO_PAIRS) and math.isnan(raw) and math.isnan(scale)
    phi, raw, npairs, scale, status = ar.autocorr_series(np.zeros(0), np.zeros(0))
    assert (phi, npairs, status) == (0.0, 0, ar.AR_NO_PAIRS) and math.isnan(raw) and math.isnan(scale)
    # a constant residual: C / np and ss / n are means of equal terms
    assert ar.autocorr_series(np.full(64, 3.0), np.zeros(64))[1] == 1.0


GAPPY_N, GAPPY_T = 50, 30000


@pytest.fixture(scope='module')
def gappy():
    """long series with every third row absent: one pair per three rows (rows 3j, 3j + 1)"""
    r = ar.synth_ar1(np.random.default_rng(13), GAPPY_N, GAPPY_T, PHI)
    r[:, 2::3] = np.nan
    r.setflags(write=False)
    return r


def _mean_against_phi(raw):
    """(mean - phi, the standard error of the mean from the estimates' own spread).  The series are long so that the
    estimator's bias, of order phi / np = 6e-5, is a few hundredths of that standard error (about 1.7e-3) and is left out."""
    return raw.mean() - PHI, raw.std(ddof=1) / math.sqrt(len(raw))


def test_estimator_on_a_gappy_panel(gappy):
    res = ar.autocorr(gappy, np.zeros_like(gappy))
    assert (res['n_pairs'] == GAPPY_T // 3).all()
    d, se = _mean_against_phi(res['phi_raw'])
    print('contract: mean - phi %.5f, standard error %.5f' % (d, se))
    assert abs(d) <= sr.Z_MAX * se


@pytest.mark.parametrize('mutant', ar.ESTIMATOR_MUTANTS)
def test_estimator_mutants_are_rejected_on_a_gappy_panel(gappy, mutant):
    # C over n halves the estimate (np = n / 2 here); pairs across the gap mix lag two in: (phi + phi^2) / 2
    d, se = _mean_against_phi(ar.autocorr(gappy, np.zeros_like(gappy), mutant=mutant)['phi_raw'])
    print('%s: mean - phi %.5f, standard error %.5f' % (mutant, d, se))
    assert abs(d) > sr.Z_MAX * se


CHAIN_ROWS, CHAIN_SAMPLES = 32, 64 * 4096


@pytest.fixture(scope='module')
def normals():
    z = np.random.default_rng(17).standard_normal((CHAIN_ROWS, CHAIN_SAMPLES))
    z.setflags(write=False)
    return z


@pytest.mark.parametrize('phi', [0.3, 0.6, -0.5, 0.95])
def test_chain_obeys_its_laws(normals, phi):
    res = ar.chain_law_stats(ar.chain(normals, phi), phi)
    _report('phi = %g' % phi, res)
    assert not sr.failures(res)
    assert sr.ks_normal(ar.chain(normals, phi)[-1]) >= sr.P_MIN


@pytest.mark.parametrize('mutant', ar.CHAIN_MUTANTS)
def test_chain_mutants_are_rejected(normals, mutant):
    res = ar.chain_law_stats(ar.chain(normals, PHI, mutant=mutant), PHI)
    bad = sr.failures(res)
    _report(mutant, bad)
    assert bad


def test_independent_noise_fails_the_sum_law(normals):
    bad = sr.failures(ar.chain_law_stats(np.asarray(normals), PHI))
    assert any(name.startswith('running sum') for name, _, _ in bad)


def test_chain_with_phi_zero_and_one_row_is_the_input(normals):
    np.testing.assert_array_equal(ar.chain(normals, 0.0), normals)
    np.testing.assert_array_equal(ar.chain(normals[:1], 0.6), normals[:1])
    e = ar.chain(normals[:3, :5], 0.6)
    c = float(np.sqrt(1.0 - 0.6 * 0.6))
    np.testing.assert_array_equal(e[1], 0.6 * normals[0, :5] + c * normals[1, :5])
    np.testing.assert_array_equal(e[2], 0.6 * e[1] + c * normals[2, :5])


def test_sum_variance_tends_to_the_long_run_factor():
    for phi in (0.3, 0.6):
        lim = (1.0 + phi) / (1.0 - phi)
        assert ar.sum_variance(9999, phi) / 10000.0 == pytest.approx(lim, rel=1e-3)
    assert math.sqrt(ar.sum_variance(31, 0.6) / 32.0) == pytest.approx(1.94, abs=0.01)
