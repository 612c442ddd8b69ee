"""CPU tests of reconciliation's host side (include/tsf.h "reconciliation"): tsf_reconcile_shares against the numpy
restatement of tests/reconcile_ref.py bit for bit, its refusals, the Python helpers on top of it, and the restatement
itself against the laws of the method on synthetic normal draws (coherence within a bound derived from the operation
count, the variance of a reconciled member, mu = sum lambda)."""
import ctypes

import numpy as np
import pytest

from tests import reconcile_ref as rr


@pytest.fixture(scope='module')
def lib(built):
    from time_series_spark_amd import _lib, forecaster as fc
    return _lib.load(), fc, _lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _call(L, group, w, G, v):
    group = np.ascontiguousarray(group, dtype=np.int64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    lam, mu = np.full(len(group), -7.0), np.full(G, -7.0)
    rc = L.tsf_reconcile_shares(len(group), group.ctypes.data, None if w is None else w.ctypes.data, G, v.ctypes.data,
                                lam.ctypes.data, mu.ctypes.data)
    return rc, lam, mu


# group 0: 4 members; 1: no member; 2: NaN v (no total); 3: a group of one; 4: 9 members
GROUP = np.array([0, 4, 4, 0, 2, 4, 3, 4, 0, 4, 2, 4, 4, 0, 4, 2, 4], dtype=np.int64)
V = np.array([0.37, 2.5, np.nan, 1e-3, 41.0])


def test_exports(lib):
    L, fc, _lib = lib
    for sym in ('tsf_reconcile_shares', 'tsf_reconcile_out_size', 'tsf_rollup_set_totals', 'tsf_rollup_reconcile',
                'tsf_rollup_reconciled_totals'):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.tsf_reconcile_out_size() == ctypes.sizeof(_lib.TsfReconcileOut) == 32


@pytest.mark.parametrize('weights', ['given', 'null'])
def test_shares_are_the_restatement(lib, weights):
    L, fc, _lib = lib
    w = None if weights == 'null' else np.random.default_rng(3).uniform(1e-3, 30.0, len(GROUP))
    rc, lam, mu = _call(L, GROUP, w, 5, V)
    assert rc == 0
    want_lam, want_mu = rr.shares(GROUP, w, 5, V)
    assert _bits(lam, want_lam) and _bits(mu, want_mu)
    # no member / NaN v: +0.0 bit for bit; a group of one: lambda is mu
    assert _bits(mu[[1, 2]], [0.0, 0.0]) and _bits(lam[GROUP == 2], np.zeros(3))
    assert _bits(lam[GROUP == 3], mu[3:4]) and 0 < mu[3] < 1
    assert (lam[GROUP != 2] > 0).all() and (lam < 1).all() and (mu <= 1).all()
    if w is None:
        assert _bits(lam[GROUP == 0], np.full(4, 1.0 / (0.37 + 4.0))) and mu[4] == 9.0 / (41.0 + 9.0)


def test_refusals(lib):
    L, fc, _lib = lib
    w = np.ones(len(GROUP))

    def bad(a, i, x):
        a = a.copy()
        a[i] = x
        return a

    assert _call(L, GROUP, w, 5, V)[0] == 0
    for g in (-1, 5):
        assert _call(L, bad(GROUP, 6, g), w, 5, V)[0] == -1
    for x in (0.0, -1.0, np.inf, np.nan):
        assert _call(L, GROUP, bad(w, 2, x), 5, V)[0] == -1, x
    for x in (0.0, -2.0, np.inf, -np.inf):
        assert _call(L, GROUP, w, 5, bad(V, 1, x))[0] == -1, x
    assert _call(L, GROUP, w, 5, bad(V, 1, np.nan))[0] == 0         # (NaN v: the group has no total)
    # a bad weight in a group without a total is still a bad weight
    assert _call(L, GROUP, bad(w, 4, -1.0), 5, V)[0] == -1


def test_python_policies(lib):
    L, fc, _lib = lib
    lam, mu = fc.reconcile_shares(GROUP, 5, total_weight=V)
    assert _bits(lam, rr.shares(GROUP, None, 5, V)[0]) and _bits(mu, rr.shares(GROUP, None, 5, V)[1])
    lam, mu = fc.reconcile_shares(GROUP, 5, total_weight='ols')
    assert _bits(mu, [4 / 5.0, 0.0, 3 / 4.0, 1 / 2.0, 9 / 10.0])
    w = np.linspace(0.5, 2.0, len(GROUP))
    lam, mu = fc.reconcile_shares(GROUP, 5, weight=w, total_weight='struct')
    want = rr.shares(GROUP, w, 5, [4.0, np.nan, 3.0, 1.0, 9.0])
    assert _bits(lam, want[0]) and _bits(mu, want[1]) and mu[1] == 0
    for kw in (dict(group=GROUP + 1), dict(weight=w[:-1]), dict(weight=-w), dict(total_weight='mint'),
               dict(total_weight=V[:4]), dict(total_weight=-V), dict(n_groups=0)):
        a = dict(dict(group=GROUP, n_groups=5), **kw)
        with pytest.raises(ValueError):
            fc.reconcile_shares(a.pop('group'), a.pop('n_groups'), **a)
    lam, mu = fc.reconcile_shares(np.zeros(0, dtype=np.int64), 2)
    assert lam.shape == (0,) and _bits(mu, [0.0, 0.0])


def test_aggregate_aligned(lib):
    L, fc, _lib = lib
    y = np.random.default_rng(1).normal(100, 30, (7, 11))
    group = np.array([2, 0, 2, 2, 0, 3, 2])
    tot = fc.aggregate_aligned(y, group, 4)
    want = np.zeros((4, 11))
    for n in range(7):
        want[group[n]] = want[group[n]] + y[n]
    assert _bits(tot, want) and _bits(tot[1], np.zeros(11))
    assert _bits(fc.aggregate_aligned(y.astype(np.float32), group, 4), fc.aggregate_aligned(y.astype(np.float32).astype(np.float64), group, 4))
    for a in ((y[0], group, 4), (y, group[:-1], 4), (y, group, 3), (y, group - 1, 4)):
        with pytest.raises(ValueError):
            fc.aggregate_aligned(*a)


# ---- the restatement alone satisfies the laws of the method -----------------------------------------------------------

S = 4096
SIZES = (1, 4, 9)


@pytest.fixture(scope='module')
def synthetic():
    """3 groups of 1, 4 and 9 members: x_i ~ N(m_i, w_i), t ~ N(sum m_i + bias, v), independent, one row, S = 4096 draws;
    weights equal to the true variances"""
    rng = np.random.default_rng(2024)
    group = np.repeat(np.arange(3), SIZES)
    N = len(group)
    m, w = rng.uniform(20.0, 200.0, N), rng.uniform(0.5, 25.0, N)
    v, bias = np.array([3.0, 10.0, 60.0]), np.array([4.0, -15.0, 30.0])
    x = m[:, None, None] + np.sqrt(w)[:, None, None] * rng.standard_normal((N, 1, S))
    tm = np.array([m[group == g].sum() for g in range(3)]) + bias
    top = tm[:, None, None] + np.sqrt(v)[:, None, None] * rng.standard_normal((3, 1, S))
    acc = np.zeros((3, 1, S))
    for n in range(N):
        acc[group[n]] = acc[group[n]] + x[n]
    lam, mu = rr.shares(group, w, 3, v)
    d = rr.incoherence(top, acc, [1, 1, 1])
    return dict(group=group, w=w, v=v, x=x, top=top, acc=acc, lam=lam, mu=mu, xr=rr.members(x, group, lam, d),
                tr=rr.totals(acc, mu, d))


def test_reconciled_members_sum_to_the_reconciled_total(synthetic):
    """within rr.coherence_bound, which is derived there from the operation count (not fitted)"""
    s = synthetic
    for g, n_g in enumerate(SIZES):
        idx = np.flatnonzero(s['group'] == g)
        total = np.zeros((1, S))
        for n in idx:
            total = total + s['xr'][n]
        bound = rr.coherence_bound(n_g, np.abs(s['x'][idx]).sum(axis=0), np.abs(s['top'][g]))
        err = np.abs(total - s['tr'][g])
        print('group of %d: max |sum of members - total| / bound = %.3f' % (n_g, (err / bound).max()))
        assert (err <= bound).all()
        # the incoherent pair it started from is far apart: the bound is not vacuous
        assert np.abs(s['acc'][g] - s['top'][g]).mean() > 1e10 * bound.max()


def test_reconciled_member_variance(synthetic):
    """w_i - w_i^2 / (v + W) within 5 standard errors, sqrt(2 / (S - 1)) times the value"""
    s = synthetic
    for n in range(len(s['group'])):
        g = s['group'][n]
        W = s['w'][s['group'] == g].sum()
        want = s['w'][n] - s['w'][n] ** 2 / (s['v'][g] + W)
        got = s['xr'][n, 0].var(ddof=1)
        assert want < s['w'][n]
        assert abs(got - want) <= 5 * np.sqrt(2.0 / (S - 1)) * want, (n, got, want)
    for g in range(3):                                             # and the total's: v - v^2 / (v + W) = v W / (v + W)
        W = s['w'][s['group'] == g].sum()
        want = s['v'][g] * W / (s['v'][g] + W)
        assert abs(s['tr'][g, 0].var(ddof=1) - want) <= 5 * np.sqrt(2.0 / (S - 1)) * want


def test_mu_is_the_sum_of_lambda(synthetic):
    s = synthetic
    for g, n_g in enumerate(SIZES):
        tot = 0.0
        for lam in s['lam'][s['group'] == g]:
            tot = tot + lam
        assert abs(tot - s['mu'][g]) <= n_g * np.spacing(s['mu'][g])
    assert s['lam'][0] == s['mu'][0]                               # a group of one


def test_no_total_and_zero_share_are_neutral(synthetic):
    s = synthetic
    d = rr.incoherence(s['top'], s['acc'], [1, 0, 1])
    xr = rr.members(s['x'], s['group'], s['lam'], d)
    assert _bits(xr[s['group'] == 1], s['x'][s['group'] == 1]) and not _bits(xr[0], s['x'][0])
    assert _bits(rr.totals(s['acc'], s['mu'], d)[1], s['acc'][1])
    d = rr.incoherence(s['top'], s['acc'], [1, 1, 1])
    assert _bits(rr.members(s['x'], s['group'], np.zeros(14), d), s['x'])
    assert _bits(rr.totals(s['acc'], np.zeros(3), d), s['acc'])
