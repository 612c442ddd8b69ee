"""Reference for the correlated group roll-ups (include/tsf.h "correlated group roll-ups"), in numpy and written from
the header's contract, not from the kernels.

Two parts:
  1. the estimator of a group's residual correlation (tsf_residual_corr), with the contract's summation order -- the
     device's results are compared bit for bit;
  2. the factor draw of tsf_rollup_set_noise_corr's add route: what rollup_add_corr_kernel adds to a cell beyond the
     members' own draws, on tests/sampler_ref.py's restated streams (stream_key, u01, box_muller by import), with one
     switch for a mutant of it.

The summation order of the two sums over the rows (ss of a series, A of a group): 64 partials from +0.0, partial l adds
the values of rows l, l + 64, ... in ascending order (an absent row contributes +0.0, which changes no bit), then
v[l] = v[l] + v[l ^ d] for d = 1, 2, 4, 8, 16, 32; every lane ends with the same bits (a + b is commutative)."""
import numpy as np

from tests import sampler_ref as sr

CORR_OK, CORR_NO_PAIRS = 0, -50
_LANES = np.arange(64)


def lane_sum(v):
    """the contract's sum of v [..., T] over its last axis -> [...]"""
    v = np.asarray(v)
    T = v.shape[-1]
    pad = (-T) % 64
    if pad:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (pad,), dtype=v.dtype)], axis=-1)
    v = v.reshape(v.shape[:-1] + (-1, 64))
    part = np.zeros(v.shape[:-2] + (64,), dtype=v.dtype)
    for j in range(v.shape[-2]):                # rows l, l + 64, ... in ascending order
        part = part + v[..., j, :]
    for d in (1, 2, 4, 8, 16, 32):
        part = part + part[..., _LANES ^ d]
    return part[..., 0]


def series_scale(y, fitted, min_rows=8):
    """-> (scale [N] (NaN: unused), e [N][T] (NaN: the row is absent or the series unused))"""
    r = np.asarray(y).astype(np.float64) - np.asarray(fitted, dtype=np.float64)
    present = np.isfinite(r)
    with np.errstate(invalid='ignore', over='ignore'):
        ss = lane_sum(np.where(present, r * r, 0.0))
    n = present.sum(axis=1)
    used = (n >= min_rows) & (ss != 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = np.where(used, np.sqrt(ss / n.astype(np.float64)), np.nan)
        e = np.where(present & used[:, None], r / scale[:, None], np.nan)
    return scale, e


def group_rows(e, members):
    """(c [T] double, p [T] int64) of one group: its used members present at each row, in ascending series index"""
    T = e.shape[1]
    u, q, k = np.zeros(T), np.zeros(T), np.zeros(T, dtype=np.int64)
    for i in sorted(int(m) for m in members):
        ok = ~np.isnan(e[i])
        ei = np.where(ok, e[i], 0.0)
        u = np.where(ok, u + ei, u)
        q = np.where(ok, q + ei * ei, q)
        k = k + ok
    return u * u - q, k * (k - 1)


def residual_corr(y, fitted, group, G, rho_max=0.95, min_rows=8):
    """the contract of tsf_residual_corr -> dict(rho, rho_raw, n_pairs, n_used, status [G]; scale [N])"""
    group = np.asarray(group, dtype=np.int64)
    y = np.asarray(y)
    N, T = y.shape
    scale, e = (series_scale(y, fitted, min_rows) if N else (np.zeros(0), np.zeros((0, T))))
    out = dict(rho=np.zeros(G), rho_raw=np.zeros(G), n_pairs=np.zeros(G, np.int64), n_used=np.zeros(G, np.int32),
               status=np.zeros(G, np.int32), scale=scale)
    for g in range(G):
        members = np.flatnonzero(group == g)
        c, p = group_rows(e, members)
        A, P = lane_sum(c), int(lane_sum(p))
        out['n_used'][g] = int((~np.isnan(scale[members])).sum())
        out['n_pairs'][g] = P // 2
        if P == 0:
            out['rho_raw'][g], out['rho'][g], out['status'][g] = np.nan, 0.0, CORR_NO_PAIRS
        else:
            raw = A / np.float64(P)
            out['rho_raw'][g], out['rho'][g], out['status'][g] = raw, np.fmin(np.fmax(raw, 0.0), rho_max), CORR_OK
    return out


# ---- the factor draw ---------------------------------------------------------------------------------------------

MUTANTS = ('a_without_minus_one',)


def corr_coefficients(rho, mutant=None):
    """(a, b) = (sqrt(1 - rho) - 1, sqrt(rho)), as tsf_rollup_set_noise_corr forms them on the host"""
    assert mutant is None or mutant in MUTANTS
    rho = np.asarray(rho, dtype=np.float64)
    a = np.sqrt(1.0 - rho) - (0.0 if mutant == 'a_without_minus_one' else 1.0)
    return a, np.sqrt(rho)


def stream_normal(seed, key, S, H, stream):
    """[len(key)][H][S]: Box-Muller on the stream keyed (seed, key, sample, stream) at counters 2h, 2h + 1 -- with
    stream 1 the z a member's noise is made from (sampler_ref.restated_draws), with stream 2 a group's factor w"""
    key = np.atleast_1d(np.asarray(key, dtype=np.int64))
    n = len(key)
    k = sr.stream_key(seed, np.repeat(key, S), np.tile(np.arange(S, dtype=np.int64), n), stream).reshape(n, 1, S)
    h2 = (2 * np.arange(H, dtype=np.uint64)).reshape(1, H, 1)
    return sr.box_muller(sr.u01(k, h2), sr.u01(k, h2 + np.uint64(1)))


def corr_term(seed, series_key, group_key, rho, sn, S, H, mutant=None):
    """[H][S]: what the correlated add puts into a group's cells beyond the members' own draws -- the sum over the
    members, in list order from +0.0, of (a z_i + b w) sn_i"""
    a, b = corr_coefficients(rho, mutant)
    z = stream_normal(seed, series_key, S, H, 1)
    w = stream_normal(seed, group_key, S, H, 2)[0]
    out = np.zeros((H, S))
    for i in range(len(z)):
        out = out + ((a * z[i] + b * w) * sn[i])
    return out


def group_noise(seed, series_key, group_key, rho, sn, S, H, mutant=None):
    """[H][S]: the summed observation noise of a group's members under the correlated add: each member's own
    (z_i sn_i) plus its part of the correlated term, added member by member as the accumulator adds them"""
    a, b = corr_coefficients(rho, mutant)
    z = stream_normal(seed, series_key, S, H, 1)
    w = stream_normal(seed, group_key, S, H, 2)[0]
    out = np.zeros((H, S))
    for i in range(len(z)):
        out = out + (z[i] * sn[i] + ((a * z[i] + b * w) * sn[i]))
    return out


def group_variance(rho, sn):
    """the law's variance of a group's summed noise: (1 - rho) sum sn^2 + rho (sum sn)^2"""
    sn = np.asarray(sn, dtype=np.float64)
    return (1.0 - rho) * np.sum(sn * sn) + rho * np.sum(sn) ** 2
