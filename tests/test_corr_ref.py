"""CPU tests of tests/corr_ref.py, the numpy restatement of the correlated group roll-ups (include/tsf.h): the
estimator's law, its clipping and edge cases, the factor draw's laws, and that the laws reject a subtly wrong factor.
The GPU suite (tests/test_gpu_rollup_corr.py) ties the device to this restatement; this file shows that the restatement
says what it should.  Thresholds: tests/sampler_ref.py's Z_MAX = 5.5 and P_MIN = 1e-7 (derived there, not measured)."""
import math

import numpy as np
import pytest

from tests import corr_ref as cr, sampler_ref as sr

SEED = 20240611


def _planted(rho, m, T, seed):
    """e [m][T] = sqrt(rho) f_t + sqrt(1 - rho) eps_it: unit variance, every pair correlated rho at the same row"""
    rng = np.random.default_rng(seed)
    f = rng.normal(0, 1, T)
    return math.sqrt(rho) * f[None, :] + math.sqrt(1.0 - rho) * rng.normal(0, 1, (m, T))


# ---- the summation order -------------------------------------------------------------------------------------------

def test_lane_sum_is_the_stated_order():
    """against a scalar loop written from the header: 64 partials, rows l, l + 64, ..., then the butterfly"""
    rng = np.random.default_rng(1)
    for T in (1, 63, 64, 70, 129, 4096):
        v = rng.normal(0, 1, T) * 10.0 ** rng.integers(-3, 4, T)
        part = [0.0] * 64
        for t in range(T):                      # (ascending t visits each lane's rows in ascending order)
            part[t % 64] = part[t % 64] + float(v[t])
        for d in (1, 2, 4, 8, 16, 32):
            part = [part[i] + part[i ^ d] for i in range(64)]
        assert len(set(part)) == 1
        assert np.float64(part[0]).view(np.int64) == np.float64(cr.lane_sum(v)).view(np.int64)
    p = rng.integers(0, 1000, (3, 130))
    assert np.array_equal(cr.lane_sum(p), p.sum(axis=1)) and cr.lane_sum(p).dtype == np.int64


# ---- the estimator's law -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rho', [0.0, 0.3, 0.7])
def test_estimator_law(rho):
    """rho_raw against the planted rho at 5.5 standard errors.  The standard error comes from the data: the row values
    v_t = ((sum_i e_it)^2 - sum_i e_it^2) / (m (m - 1)) of the planted e are iid over t with mean rho, so their mean has
    standard error sd(v_t) / sqrt(T).

    The estimator divides each series by its own root mean square s_i instead of the true scale 1, which makes it the
    (uncentred) sample correlation coefficient averaged over the pairs.  For normal data that has the bias
    -rho (1 - rho^2) / (2 T) + O(T^-2), at most 0.193 / T in magnitude (rho = 1 / sqrt(3)) -- below 5e-5 at T = 4096,
    under 2 % of the smallest standard error here (0.003 at rho = 0) -- and a variance no larger than the unnormalised
    mean's ((1 - rho^2)^2 against 1 + rho^2 per pair and row), so the threshold is not tightened by the normalisation."""
    m, T = 8, 4096
    e = _planted(rho, m, T, seed=SEED + int(100 * rho))
    v = (e.sum(axis=0) ** 2 - (e * e).sum(axis=0)) / (m * (m - 1))
    se = v.std(ddof=1) / math.sqrt(T)
    assert 0.2 / T < 0.02 * se
    y = 3.0 + 2.5 * e * np.arange(1, m + 1)[:, None]            # a scale per series: the estimator must not see it
    r = cr.residual_corr(y, np.full((m, T), 3.0), np.zeros(m, dtype=np.int64), 1, rho_max=1.0)
    z = (r['rho_raw'][0] - rho) / se
    print('rho %.1f: rho_raw %.5f, se %.5f, z %.2f' % (rho, r['rho_raw'][0], se, z))
    assert abs(z) <= sr.Z_MAX
    assert r['status'][0] == cr.CORR_OK and r['n_used'][0] == m and r['n_pairs'][0] == T * m * (m - 1) // 2
    assert np.allclose(r['scale'], 2.5 * np.arange(1, m + 1) * np.sqrt((e * e).mean(axis=1)), rtol=1e-12)
    assert r['rho'][0] == max(r['rho_raw'][0], 0.0)


def test_clipping():
    T = 256
    rng = np.random.default_rng(3)
    f = rng.normal(0, 1, T)
    # two series that move against each other: rho_raw near -1, clipped to 0; two that move together: clipped to rho_max
    y = np.stack([f, -f + 0.01 * rng.normal(0, 1, T), f, f + 0.01 * rng.normal(0, 1, T)])
    r = cr.residual_corr(y, np.zeros((4, T)), np.array([0, 0, 1, 1]), 2, rho_max=0.95)
    assert r['rho_raw'][0] < -0.99 and r['rho'][0] == 0.0 and r['status'][0] == cr.CORR_OK
    assert r['rho_raw'][1] > 0.99 and r['rho'][1] == 0.95
    assert cr.residual_corr(y, np.zeros((4, T)), np.array([0, 0, 1, 1]), 2, rho_max=1.0)['rho'][1] == r['rho_raw'][1]


def test_edge_cases():
    """a singleton, an empty group, a group entry of -1, NaN rows, a zero-residual series, n_i < min_rows"""
    T = 40
    rng = np.random.default_rng(4)
    f = rng.normal(0, 1, T)
    y = f[None, :] + 0.5 * rng.normal(0, 1, (9, T))
    fitted = np.zeros((9, T))
    group = np.array([0, 0, 0, 1, -1, 3, 3, 4, 4])             # group 1: a singleton; group 2: empty; series 4: no part
    y[1, 5:12] = np.nan                                         # NaN rows: absent for series 1 only
    fitted[2, 30] = np.inf                                      # a non-finite residual is an absent row
    y[5] = 7.0
    fitted[5] = 7.0                                             # a zero-residual series: unused
    y[7, 6:] = np.nan                                           # 6 present rows < min_rows = 8: unused
    r = cr.residual_corr(y, fitted, group, 5)
    assert list(r['status']) == [cr.CORR_OK] + [cr.CORR_NO_PAIRS] * 4
    assert list(r['n_used']) == [3, 1, 0, 1, 1]
    assert np.isnan(r['scale'][[5, 7]]).all() and np.isfinite(r['scale'][[0, 1, 2, 3, 4, 6, 8]]).all()
    assert np.isnan(r['rho_raw'][1:]).all() and not r['rho'][1:].any() and not r['n_pairs'][1:].any()
    # group 0's pairs: 3 members on the rows all have, 2 where one is absent
    k = np.full(T, 3)
    k[5:12] -= 1
    k[30] -= 1
    assert r['n_pairs'][0] == int((k * (k - 1)).sum()) // 2
    # ... and its value is the plain-numpy mean of the pair products over the rows both members have
    e = (y[:3] - fitted[:3])
    e[~np.isfinite(e)] = np.nan
    e = e / np.sqrt(np.nanmean(e * e, axis=1))[:, None]
    prod = [e[i] * e[j] for i in range(3) for j in range(3) if i != j]
    want = np.nansum(prod) / np.count_nonzero(~np.isnan(prod))
    assert abs(r['rho_raw'][0] - want) <= 1e-13
    # the series outside every group changes nothing: the same call without it
    keep = group >= 0
    r2 = cr.residual_corr(y[keep], fitted[keep], group[keep], 5)
    for key in ('rho', 'rho_raw', 'n_pairs', 'n_used', 'status'):
        assert np.array_equal(r[key], r2[key], equal_nan=True)
    # members that never overlap: no pair
    y2 = np.full((2, T), np.nan)
    y2[0, :20], y2[1, 20:] = f[:20], f[20:]
    r3 = cr.residual_corr(y2, np.zeros((2, T)), np.zeros(2, dtype=np.int64), 1)
    assert r3['status'][0] == cr.CORR_NO_PAIRS and r3['n_used'][0] == 2 and np.isnan(r3['rho_raw'][0])
    # no series at all
    r4 = cr.residual_corr(np.zeros((0, T)), np.zeros((0, T)), np.zeros(0, dtype=np.int64), 2)
    assert list(r4['status']) == [cr.CORR_NO_PAIRS] * 2 and not r4['rho'].any()


# ---- the factor draw's laws ------------------------------------------------------------------------------------------

NS, H = 4096, 8
SN = np.array([12.5, 12.5, 12.5, 12.5, 3.0, 3.0, 3.0, 3.0])     # two scales within a group


def _variance_z(noise, rho, sn):
    """z of the sample variance (known mean 0) of a group's summed noise over the samples and rows against the law's:
    the summed noise is normal, so the mean square has relative standard error sqrt(2 / n)"""
    n = noise.size
    return (np.mean(noise * noise) / cr.group_variance(rho, sn) - 1.0) / math.sqrt(2.0 / n)


@pytest.mark.parametrize('rho', [0.0, 0.3, 0.9])
def test_factor_draw_laws(rho):
    keys = 7919 * np.arange(8, dtype=np.int64) + 3
    x = cr.group_noise(SEED, keys, 5, rho, SN, NS, H)
    assert abs(_variance_z(x, rho, SN)) <= sr.Z_MAX
    assert sr.ks_normal(x / math.sqrt(cr.group_variance(rho, SN))) >= sr.P_MIN
    # a member's own marginal law is unchanged: N(0, sn^2)
    one = cr.group_noise(SEED, keys[:1], 5, rho, SN[:1], NS, H)
    assert abs(_variance_z(one, rho, SN[:1])) <= sr.Z_MAX and sr.ks_normal(one / SN[0]) >= sr.P_MIN
    # two members of the group: correlation rho at the same row and sample
    a = cr.group_noise(SEED, keys[1:2], 5, rho, SN[1:2], NS, H) / SN[1]
    b = cr.group_noise(SEED, keys[5:6], 5, rho, SN[5:6], NS, H) / SN[5]
    assert abs((np.mean(a * b) - rho) / math.sqrt((1.0 + rho * rho) / a.size)) <= sr.Z_MAX
    # another group (another factor key, other members): independent; rows and samples of one group: independent
    other = cr.group_noise(SEED, keys + 1, 6, rho, SN, NS, H)
    sd = math.sqrt(cr.group_variance(rho, SN))
    name, kind, z = sr.corr_stat('groups', x / sd, other / sd)
    assert abs(z) <= sr.Z_MAX
    assert abs(sr.corr_stat('rows', x[:-1] / sd, x[1:] / sd)[2]) <= sr.Z_MAX
    assert abs(sr.corr_stat('samples', x[:, :-1] / sd, x[:, 1:] / sd)[2]) <= sr.Z_MAX


@pytest.mark.parametrize('rho', [0.3, 0.9])
def test_the_laws_reject_a_wrong_coefficient(rho):
    """a_g = sqrt(1 - rho) without the - 1: each member's own noise is counted twice over"""
    keys = 7919 * np.arange(8, dtype=np.int64) + 3
    x = cr.group_noise(SEED, keys, 5, rho, SN, NS, H, mutant='a_without_minus_one')
    assert abs(_variance_z(x, rho, SN)) > sr.Z_MAX


def test_rho_zero_adds_nothing():
    keys = np.arange(5, dtype=np.int64)
    a, b = cr.corr_coefficients(0.0)
    assert a == 0.0 and b == 0.0
    assert not cr.corr_term(SEED, keys, 0, 0.0, SN[:5], 64, 3).any()
    # and the term is the difference between the group's noise with and without the correlation (to rounding)
    t = cr.corr_term(SEED, keys, 0, 0.6, SN[:5], 64, 3)
    d = cr.group_noise(SEED, keys, 0, 0.6, SN[:5], 64, 3) - cr.group_noise(SEED, keys, 0, 0.0, SN[:5], 64, 3)
    assert np.abs(t - d).max() <= 1e-12 * 5 * SN.max()
