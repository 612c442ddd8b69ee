"""Reference for the serially correlated observation noise (include/tsf.h "serially correlated observation noise"):
a numpy restatement of tsf_residual_autocorr's contract, operation for operation (the 64 partials and the xor butterfly
included), and of the AR(1) chain of the draws, with the laws the chain must obey.  Written from the contract in
include/tsf.h, not from the kernels.  Each restatement has switches for mutants of it, so the CPU suite shows that its
checks reject a subtly wrong estimator or chain.

The laws of the chain, for iid standard normal z_h and |phi| < 1, c = sqrt(1 - phi^2):
    e_0 = z_0,  e_h = phi e_(h-1) + c z_h   =>   e_h ~ N(0, 1) for every h (the start is stationary),
    cov(e_i, e_j) = phi^|i-j|,
    Var(sum_(h<=m) e_h) = (m + 1) + 2 sum_(k=1..m) (m + 1 - k) phi^k.
For a Gaussian pair with correlation r, Var(e_i e_j) = 1 + r^2, so mean(e_i e_j) over n samples has variance
(1 + phi^(2k)) / n at lag k; a sample variance of n Gaussian values has relative standard error sqrt(2 / (n - 1)).

The estimator's bias (derived in include/tsf.h): E[phi_raw] ~ phi - 2 phi / T on a Gaussian AR(1) of T rows, and its
standard error sqrt((1 - phi^2) / T) (Bartlett), so the mean over N series has standard error sqrt((1 - phi^2) / T / N)."""
import math

import numpy as np

AR_OK, AR_NO_PAIRS = 0, -51
ESTIMATOR_MUTANTS = ('c_over_n', 'pairs_across_gap')
CHAIN_MUTANTS = ('c_one_minus_phi', 'restart_8', 'scaled_start')


def wave_sum(terms):
    """The library's sum of a series' terms [L] (absent ones given as +0.0): 64 partials from +0.0, partial l adds terms
    l, l + 64, ... in ascending order, then the xor butterfly d = 1, 2, 4, 8, 16, 32.  -> the value of lane 0."""
    terms = np.asarray(terms, dtype=np.float64)
    L = len(terms)
    steps = (L + 63) // 64
    pad = np.zeros(steps * 64)
    pad[:L] = terms
    part = np.zeros(64)
    for s in range(steps):
        part = part + pad[64 * s:64 * s + 64]
    lanes = np.arange(64)
    for d in (1, 2, 4, 8, 16, 32):
        part = part + part[lanes ^ d]
    return float(part[0])


def autocorr_series(y, fitted, phi_max=0.95, min_pairs=8, mutant=None):
    """One series of tsf_residual_autocorr: y [T] in its own dtype, fitted [T] double ->
    (phi, phi_raw, n_pairs, scale, status)."""
    assert mutant is None or mutant in ESTIMATOR_MUTANTS
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.asarray(y).astype(np.float64) - np.asarray(fitted, dtype=np.float64)
    T = len(r)
    present = np.isfinite(r)
    n = int(present.sum())
    rr = np.where(present, r, 0.0)
    ss = wave_sum(rr * rr)
    if mutant == 'pairs_across_gap':
        # the neighbour of a row is the last present row before it, whatever lies between
        idx = np.where(present, np.arange(T), -1)
        last = np.maximum.accumulate(idx)
        prev_i = np.concatenate([[-1], last[:-1]])
        pair = present & (prev_i >= 0)
        prev = np.where(pair, rr[np.maximum(prev_i, 0)], 0.0)
    else:
        pair = np.zeros(T, dtype=bool)
        pair[1:] = present[1:] & present[:-1]
        prev = np.concatenate([[0.0], rr[:-1]])
    C = wave_sum(np.where(pair, rr * prev, 0.0))
    npairs = int(pair.sum())
    nan = float('nan')
    with np.errstate(invalid='ignore', divide='ignore'):
        var = np.float64(ss) / np.float64(n)
        scale = nan if ss == 0.0 else float(np.sqrt(var))
        if npairs < min_pairs or ss == 0.0:
            return 0.0, nan, npairs, scale, AR_NO_PAIRS
        raw = float((np.float64(C) / np.float64(n if mutant == 'c_over_n' else npairs)) / var)
    phi = float(np.fmin(np.fmax(raw, 0.0), phi_max))
    return phi, raw, npairs, scale, AR_OK


def autocorr(y, fitted, offsets=None, phi_max=0.95, min_pairs=8, mutant=None):
    """tsf_residual_autocorr on a panel: aligned y, fitted [N][T], or 1-D with offsets [N + 1] ->
    dict(phi, phi_raw, n_pairs, scale, status), each [N]."""
    y, fitted = np.asarray(y), np.asarray(fitted, dtype=np.float64)
    if offsets is None:
        rows = [(y[i], fitted[i]) for i in range(y.shape[0])]
    else:
        rows = [(y[a:b], fitted[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    res = [autocorr_series(a, b, phi_max, min_pairs, mutant) for a, b in rows]
    N = len(res)
    cols = list(zip(*res)) if N else [[]] * 5
    return {'phi': np.array(cols[0], dtype=np.float64).reshape(N), 'phi_raw': np.array(cols[1], dtype=np.float64).reshape(N),
            'n_pairs': np.array(cols[2], dtype=np.int64).reshape(N), 'scale': np.array(cols[3], dtype=np.float64).reshape(N),
            'status': np.array(cols[4], dtype=np.int32).reshape(N)}


def noise_c(phi):
    """c = sqrt(1 - phi * phi) as tsf_set_noise_ar forms it: a product, a subtraction, IEEE sqrt"""
    phi = np.asarray(phi, dtype=np.float64)
    return np.sqrt(1.0 - phi * phi)


def chain(z, phi, axis=0, mutant=None):
    """The chain along `axis` of z (the standard normals of a sample's rows in the caller's order) at one phi:
    e_0 = z_0, e_h = fl(fl(phi e_(h-1)) + fl(c z_h)); phi == 0 gives z itself."""
    assert mutant is None or mutant in CHAIN_MUTANTS
    z = np.moveaxis(np.asarray(z, dtype=np.float64), axis, 0)
    phi = float(phi)
    if phi == 0.0:
        return np.moveaxis(z.copy(), 0, axis)
    c = float(noise_c(phi)) if mutant != 'c_one_minus_phi' else 1.0 - phi
    e = np.empty_like(z)
    for h in range(z.shape[0]):
        if h == 0 or (mutant == 'restart_8' and h % 8 == 0):
            e[h] = c * z[h] if (mutant == 'scaled_start' and h == 0) else z[h]
        else:
            e[h] = phi * e[h - 1] + c * z[h]
    return np.moveaxis(e, 0, axis)


def sum_variance(m, phi):
    """Var(e_0 + ... + e_m) of the stationary chain"""
    k = np.arange(1, m + 1)
    return (m + 1) + 2.0 * float(np.sum((m + 1 - k) * phi ** k))


def chain_law_stats(e, phi, lags=(1, 2, 5), pair_row=10, sum_rows=(1, 7, 31)):
    """The statistics of chained noise e [R][n] (R rows in order, n independent samples) against the laws above ->
    [(name, 'z', value)], each standard normal under the laws (to the normal approximation of a mean over n).  Needs
    R > max(sum_rows) and pair_row + max(lags) < R."""
    R, n = e.shape
    out = []
    for h in (0, R // 2, R - 1):
        out.append(('row %d: mean' % h, 'z', e[h].mean() * math.sqrt(n)))
        out.append(('row %d: variance' % h, 'z', ((e[h] ** 2).mean() - 1.0) / math.sqrt(2.0 / n)))
    for k in lags:
        r = phi ** k
        out.append(('lag %d: mean(e_i e_j) - phi^k' % k, 'z',
                    ((e[pair_row] * e[pair_row + k]).mean() - r) / math.sqrt((1.0 + r * r) / n)))
    cs = np.cumsum(e, axis=0)
    for m in sum_rows:
        v = sum_variance(m, phi)
        out.append(('running sum at row %d: variance' % m, 'z', (cs[m].var(ddof=1) / v - 1.0) / math.sqrt(2.0 / (n - 1))))
    return out


def synth_ar1(rng, N, T, phi, sd=1.0):
    """[N][T] stationary Gaussian AR(1) rows with marginal standard deviation sd"""
    z = rng.standard_normal((N, T))
    return sd * chain(z, phi, axis=1)
