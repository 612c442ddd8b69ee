"""CPU tests of the reference for the conditioned start of the AR(1) noise chain (tests/ar_start_ref.py): the restated
draw obeys its laws at sampler_ref's thresholds, three subtly wrong starts are rejected at the same thresholds, the
library's host-only tsf_noise_ar_mean is the reference bit for bit (it needs the library and no device), and the
corrected point forecast is more accurate than the uncorrected one on planted data.  tests/test_gpu_ar_start.py holds
the device against this reference."""
import ctypes
import math

import numpy as np
import pytest

from tests import ar_ref as ar, ar_start_ref as ars, sampler_ref as sr

ROWS, SAMPLES = 32, 4096
CASES = [(phi, steps, r) for phi in (0.6, 0.3) for steps in (1, 3) for r in (2.0, -2.0)]


def _report(tag, results):
    for name, kind, value in results:
        print('%s    %-60s %s %.6g' % (tag, name, kind, value))


@pytest.fixture(scope='module')
def normals():
    z = np.random.default_rng(29).standard_normal((ROWS, SAMPLES))
    z.setflags(write=False)
    return z


def _stats(z, phi, steps, r, mutant=None):
    yhat, x = ars.draw(z, phi, r, steps, mutant=mutant)
    return ars.start_law_stats(x, yhat, phi, r, steps)


@pytest.mark.parametrize('phi,steps,r', CASES)
def test_reference_obeys_its_laws(normals, phi, steps, r):
    res = _stats(normals, phi, steps, r)
    _report('phi %g steps %d r %g' % (phi, steps, r), res)
    assert len(res) == 3 * 3 + 3 + 2 * 3 and not sr.failures(res)


def test_stationary_chain_fails_the_start_laws(normals):
    """the chain of tsf_set_noise_ar alone (e_0 = z_0, no mean): row 0's mean and variance reject"""
    x = ar.chain(normals, 0.6)
    bad = [name for name, _, _ in sr.failures(ars.start_law_stats(x, np.zeros(ROWS), 0.6, 2.0, 1))]
    assert 'row 0: mean' in bad and 'row 0: variance' in bad and 'row 0: yhat is the law\'s mean' in bad


@pytest.mark.parametrize('mutant,steps,name', [('c0_one', 1, 'row 0: variance'), ('p0_phi', 3, 'row 0: mean'),
                                               ('no_mean_in_yhat', 1, 'row 0: yhat is the law\'s mean')])
def test_start_mutants_are_rejected(normals, mutant, steps, name):
    bad = sr.failures(_stats(normals, 0.6, steps, 2.0, mutant=mutant))
    _report(mutant, bad)
    assert name in [n for n, _, _ in bad]


def test_laws_in_closed_form():
    # v_h by its recursion, the running sum's variance against the double sum of the covariances
    phi, steps, H = 0.6, 3, 12
    v = ars.law_variance(phi, steps, H)
    c2 = 1.0 - phi * phi
    for h in range(1, H):
        assert v[h] == pytest.approx(phi * phi * v[h - 1] + c2, rel=1e-14)
    V = ars.sum_variance(phi, steps, H)
    for m in range(H):
        want = sum(phi ** abs(i - j) * v[min(i, j)] for i in range(m + 1) for j in range(m + 1))
        assert V[m] == pytest.approx(want, rel=1e-13)
    # far from the data: the stationary chain's law
    assert ars.sum_variance(phi, 2000, 32)[31] == pytest.approx(ar.sum_variance(31, phi), rel=1e-12)
    assert ars.law_mean(phi, 2.0, 1, 3) == pytest.approx([1.2, 0.72, 0.432])


def test_constants_and_phi_zero():
    p0, c0, m0 = ars.start_constants([0.6, 0.6, -0.5, 0.0, 0.5], [1.5, 1.5, -2.0, 7.0, 1.0], [1, 3, 2, 4, 2000])
    assert p0[0] == 0.6 and p0[1] == (0.6 * 0.6) * 0.6 and p0[2] == 0.25 and p0[3] == 0.0 and p0[4] == 0.0
    assert c0[0] == math.sqrt(1.0 - 0.6 * 0.6) and c0[3] == 1.0 and c0[4] == 1.0
    assert m0[0] == 1.5 * 0.6 and m0[2] == -0.5 and m0[3] == 0.0
    z = np.random.default_rng(1).standard_normal((5, 7))
    yhat, x = ars.draw(z, 0.0, 7.0, 1, base=np.arange(5.0))
    assert np.array_equal(yhat, np.arange(5.0)) and np.array_equal(x, np.arange(5.0)[:, None] + z)
    # resid = 0, steps = 1: the stationary chain but for the factor c0 at row 0
    _, x = ars.draw(z, 0.6, 0.0, 1)
    assert np.array_equal(x[0], 0.8 * z[0]) and np.array_equal(x[1], 0.6 * x[0] + 0.8 * z[1])


def test_residual_last_reference():
    y = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, np.nan, np.nan], [np.nan] * 4])
    got = ars.residual_last(y, np.ones((3, 4)))
    assert list(got['last_resid']) == [3.0, 1.0, 0.0] and list(got['last_gap']) == [0, 2, 4]
    assert list(got['status']) == [ars.AR_OK, ars.AR_OK, ars.AR_NO_ROW] and not np.signbit(got['last_resid'][2])
    got = ars.residual_last(np.array([5, 7], np.int32), np.array([1.0, np.inf]), offsets=np.array([0, 0, 2]))
    assert list(got['last_resid']) == [0.0, 4.0] and list(got['last_gap']) == [0, 1]
    assert list(got['status']) == [ars.AR_NO_ROW, ars.AR_OK]


# ---- tsf_noise_ar_mean through ctypes ---------------------------------------------------------------------------

def test_noise_ar_mean_bit_for_bit(built):
    from time_series_spark_amd import _lib, forecaster as fc
    rng = np.random.default_rng(7)
    phi = np.concatenate([[0.0, 0.0, 0.6, 0.6, 0.3, -0.5, -0.5, 0.95, 1e-200, -0.999], rng.uniform(-0.99, 0.99, 30)])
    steps = np.concatenate([[1, 5, 1, 2, 1000, 1, 3, 1000, 2, 1], rng.integers(1, 40, 30)]).astype(np.int32)
    resid = np.concatenate([[3.0, -3.0, 1.5, -2.0, 1e300, 2.0, -2.0, 4.0, 1.0, 0.0], rng.normal(0, 10, 30)])
    H = 40
    want = ars.mean_rows(phi, resid, steps, H)
    got = fc.noise_ar_mean(phi, resid, steps, H)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert got[4, 0] == 0.0 and got[7, 0] > 0.0 and not got[0].any()       # (0.3^1000 underflows, 0.95^1000 does not)
    assert got[2, 0] == 1.5 * 0.6 and got[2, 1] == 0.6 * (1.5 * 0.6) and got[3, 0] == -2.0 * (0.6 * 0.6)
    assert got[6, 0] == -2.0 * ((-0.5 * -0.5) * -0.5) and got[5, 1] == -0.5 * (2.0 * -0.5)
    assert fc.noise_ar_mean(phi, resid, steps, 0).shape == (40, 0)
    L = _lib.load()
    one, bad_steps, mean = np.array([0.5]), np.array([0], np.int32), np.zeros(4)
    p = lambda a: a.ctypes.data                                               # noqa: E731
    ok_steps = np.array([1], np.int32)
    assert L.tsf_noise_ar_mean(1, p(one), p(one), p(ok_steps), 4, p(mean)) == 0 and mean[0] == 0.25
    assert L.tsf_noise_ar_mean(0, None, None, None, 4, None) == 0
    for args in ((1, p(one), p(one), p(bad_steps), 4, p(mean)), (1, p(np.array([1.0])), p(one), p(ok_steps), 4, p(mean)),
                 (1, p(one), p(np.array([np.nan])), p(ok_steps), 4, p(mean)), (1, p(one), p(one), p(ok_steps), 4, None),
                 (-1, p(one), p(one), p(ok_steps), 4, p(mean)), (1, None, p(one), p(ok_steps), 4, p(mean)),
                 (1, p(one), p(one), p(ok_steps), -1, p(mean))):
        assert L.tsf_noise_ar_mean(*args) < 0
    with pytest.raises(ValueError, match='tsf_noise_ar_mean'):
        fc.noise_ar_mean([1.0], [0.0], [1], 3)
    assert ctypes.sizeof(_lib.TsfArLastOut) == L.tsf_ar_last_out_size() and _lib.AR_NO_ROW == ars.AR_NO_ROW == -52


# ---- the accuracy claim on planted data -------------------------------------------------------------------------

def test_correction_improves_the_first_held_back_row():
    """256 series x 200 rows + 8 held back, trend + weekly sine + AR(1) noise at phi = 0.6, fitted by least squares on
    the true design; phi estimated in sample by the reference estimator.  Theory: the correction removes the share
    phi^2 of row 0's squared error (ratio 0.64); required: a ratio below 1."""
    t, y, X = ars.planted_panel(5)
    T = ars.PLANT_T
    fit = ars.least_squares_forecast(y, X, T)
    est = ar.autocorr(y[:, :T], fit[:, :T])
    assert (est['status'] == ar.AR_OK).all()
    ratios, corrected = ars.accuracy_ratios(y[:, :T], fit[:, :T], y[:, T:], fit[:, T:], est['phi'])
    print('mean phi %.4f; pooled squared error, corrected / uncorrected: row 0 %.4f, rows 0..2 %.4f'
          % (est['phi'].mean(), ratios[0], ratios[1]))
    assert ratios[0] < 1.0 and ratios[1] < 1.0
    # the correction dies out along the horizon: by row 7 it is phi^8 of the last residual
    last = ars.residual_last(y[:, :T], fit[:, :T])
    assert np.abs(corrected[:, 7] - fit[:, T + 7]).max() <= 0.95 ** 8 * np.abs(last['last_resid']).max()
