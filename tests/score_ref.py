"""The contract of tsf_score_actuals (include/tsf.h, "scoring observed values") restated in numpy, operation for
operation, and the sample CRPS in exact rational arithmetic on the same doubles.  Not a test file: shared by
tests/test_score_ref.py (CPU: the restatement against the exact value) and tests/test_gpu_scores.py (the kernels
against the restatement, bit for bit).

Every numpy operation below is one IEEE double operation per element (add, subtract, multiply, divide, abs), in the
order the header writes them; nothing here can fuse a multiply with an add."""
from fractions import Fraction

import numpy as np


def nsp(n_samples):
    """n_samples rounded up to a power of two, at least 2"""
    p = 2
    while p < n_samples:
        p *= 2
    return p


def quantile(v, level):
    """tsf_predict_quantiles' expression on sorted rows v [..., S] at one level -> [...]"""
    S = v.shape[-1]
    pos = np.float64(level) * np.float64(S - 1)
    lo = min(int(np.floor(pos)), S - 1)
    hi = min(lo + 1, S - 1)
    return v[..., lo] + (v[..., hi] - v[..., lo]) * (pos - np.float64(lo))


def pinball(y, q, level):
    e = y - q
    p = np.float64(level)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(y), np.nan, np.where(e >= 0, p * e, (p - np.float64(1.0)) * e))


def pit_row(v, y):
    """sorted row v [S], scalar y -> pit (NaN for a NaN y): the counts by searchsorted"""
    if np.isnan(y):
        return np.float64(np.nan)
    S = len(v)
    lt = int(np.searchsorted(v, y, side='left'))
    eq = int(np.searchsorted(v, y, side='right')) - lt
    return (np.float64(lt) + np.float64(0.5) * np.float64(eq)) / np.float64(S)


def crps_row(v, y):
    """sorted row v [S], scalar y -> the regrouped sample CRPS by the halving tree (NaN for a NaN y)"""
    if np.isnan(y):
        return np.float64(np.nan)
    S = len(v)
    P = nsp(S)
    i = np.arange(S, dtype=np.int64)
    d = v - np.float64(y)
    w = (2 * i - (S - 1)).astype(np.float64) / np.float64(S)
    wd = w * d
    a = np.zeros(P)
    a[:S] = np.abs(d) - wd
    n = P // 2
    while n >= 1:
        a = a[:n] + a[n:2 * n]
        n //= 2
    return a[0] / np.float64(S)


def score(draws, y, levels):
    """draws [N][H][S] (any order), y [N][H] (NaN = not observed), levels [Q] -> dict of every tsf_score_out field but
    yhat: pit, crps [N][H]; q, pinball [N][Q][H]; n_obs [N] int32; mean_crps [N]; mean_pinball, coverage [N][Q]."""
    draws = np.asarray(draws, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N, H, S = draws.shape
    Q = len(levels)
    v = np.sort(draws, axis=-1)
    out = {'pit': np.zeros((N, H)), 'crps': np.zeros((N, H)), 'q': np.zeros((N, Q, H)), 'pinball': np.zeros((N, Q, H))}
    for i, p in enumerate(levels):
        out['q'][:, i] = quantile(v, p)
        out['pinball'][:, i] = pinball(y, out['q'][:, i], p)
    for n in range(N):
        for h in range(H):
            out['pit'][n, h] = pit_row(v[n, h], y[n, h])
            out['crps'][n, h] = crps_row(v[n, h], y[n, h])
    out.update(series(y, out['crps'], out['q'], out['pinball']))
    return out


def series(y, crps, q, pinball_):
    """the per-series rule: sequential sums from +0.0 over the observed rows in row order"""
    N, H = y.shape
    Q = q.shape[1]
    n_obs = np.zeros(N, np.int32)
    mean_crps = np.full(N, np.nan)
    mean_pinball, coverage = np.full((N, Q), np.nan), np.full((N, Q), np.nan)
    for n in range(N):
        obs = [h for h in range(H) if not np.isnan(y[n, h])]
        n_obs[n] = len(obs)
        if not obs:
            continue
        cnt = np.float64(len(obs))
        tot = np.float64(0.0)
        for h in obs:
            tot = tot + crps[n, h]
        mean_crps[n] = tot / cnt
        for i in range(Q):
            tot, below = np.float64(0.0), 0
            for h in obs:
                tot = tot + pinball_[n, i, h]
                below += bool(y[n, h] <= q[n, i, h])
            mean_pinball[n, i] = tot / cnt
            coverage[n, i] = np.float64(below) / cnt
    return {'n_obs': n_obs, 'mean_crps': mean_crps, 'mean_pinball': mean_pinball, 'coverage': coverage}


def crps_exact(v, y):
    """the sample CRPS mean|X - y| - mean|X - X'| / 2 of the doubles v [S] and y, as an exact Fraction (the pairwise
    term over the sorted values: sum_{i<j} (v_j - v_i) = sum_i (2 i - (S - 1)) v_i)"""
    vs = sorted(Fraction(float(x)) for x in v)
    S = len(vs)
    fy = Fraction(float(y))
    first = sum(abs(x - fy) for x in vs) / S
    pair = sum((2 * i - (S - 1)) * x for i, x in enumerate(vs)) / (S * S)       # = mean_{i,j} |v_i - v_j| / 2
    return first - pair


def mean_abs_exact(v, y):
    fy = Fraction(float(y))
    return sum(abs(Fraction(float(x)) - fy) for x in v) / len(v)


def crps_bound(v, y, exact=None):
    """the header's bound on |crps - exact|: 2^-53 (4 mean|v - y| + (log2(NSP) + 2) exact), as a Fraction"""
    exact = crps_exact(v, y) if exact is None else exact
    lg = nsp(len(v)).bit_length() - 1
    return Fraction(1, 2 ** 53) * (4 * mean_abs_exact(v, y) + (lg + 2) * exact)


def same(a, b):
    """bit for bit, NaN where and only where the other has one (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
