"""The contract of include/tsf.h "reconciliation" restated in numpy, for tests/test_reconcile_ref.py (CPU) and
tests/test_gpu_reconcile.py.  Every function performs the header's operations in the header's order on float64 arrays
(numpy's elementwise +, -, *, / are the IEEE operations; nothing here fuses), so a comparison with the library is bit
for bit."""
import numpy as np


def shares(group, w, G, v):
    """tsf_reconcile_shares: group [N], w [N] or None (all 1.0), v [G] (NaN: no total) -> (share [N], share_total [G]).
    W_g from +0.0 in ascending member index; lambda = w / (v + W), mu = W / (v + W); NaN v or no member: +0.0."""
    group = np.asarray(group, dtype=np.int64)
    N = len(group)
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    W = np.zeros(G)
    for n in range(N):
        W[group[n]] = W[group[n]] + w[n]
    lam, mu = np.zeros(N), np.zeros(G)
    for n in range(N):
        g = group[n]
        if not np.isnan(v[g]):
            lam[n] = w[n] / (v[g] + W[g])
    for g in range(G):
        if not np.isnan(v[g]) and W[g] != 0.0:
            mu[g] = W[g] / (v[g] + W[g])
    return lam, mu


def incoherence(top, acc, has_top):
    """d [G][...]: top - acc where the group has a total, +0.0 where it has none"""
    d = np.zeros_like(acc)
    for g in range(len(acc)):
        if has_top[g]:
            d[g] = top[g] - acc[g]
    return d


def members(x, group, share, d):
    """x [N][...] (draws [N][H][S] or yhat [N][H]), d = incoherence(...) -> x + share[n] * d[group[n]]"""
    out = np.empty_like(x)
    for n in range(len(x)):
        out[n] = x[n] + share[n] * d[group[n]]
    return out


def totals(acc, share_total, d):
    """acc [G][...] -> acc + share_total[g] * d[g]"""
    out = np.empty_like(acc)
    for g in range(len(acc)):
        out[g] = acc[g] + share_total[g] * d[g]
    return out


def running_sums(x):
    """c[..., 0, s] = x[..., 0, s], c[..., h, s] = c[..., h-1, s] + x[..., h, s] over the row axis (-2), sequentially"""
    c = np.array(x, dtype=np.float64, copy=True)
    for h in range(1, c.shape[-2]):
        c[..., h, :] = c[..., h - 1, :] + x[..., h, :]
    return c


def quantiles(v, levels):
    """tsf_predict_quantiles' expression on draws v [..., S] -> [..., Q]: ascending sort, pos = p (S - 1),
    lo = floor(pos), hi = min(lo + 1, S - 1), v[lo] + (v[hi] - v[lo]) * (pos - lo)"""
    v = np.sort(v, axis=-1)
    S = v.shape[-1]
    out = []
    for p in levels:
        pos = np.float64(p) * np.float64(S - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, S - 1)
        out.append(v[..., lo] + (v[..., hi] - v[..., lo]) * (pos - np.float64(lo)))
    return np.stack(out, axis=-1)


def q_and_cum_q(x, levels):
    """draws [K][H][S] -> (q, cum_q) [K][Q][H]"""
    return (np.moveaxis(quantiles(x, levels), -1, 1), np.moveaxis(quantiles(running_sums(x), levels), -1, 1))


def coherence_bound(n_g, x_abs_sum, t_abs):
    """A bound on |sum_i member'_i - total'| for one cell of a group of n_g members, u = 2^-53 the unit roundoff, first
    order in u, with A = sum_i |x_i| and B = |t| of the cell.

    With the computed acc, d, lam_i, mu (the same d on both sides, whatever its own rounding), exact arithmetic on them
    would give  sum_i (x_i + lam_i d) - (acc + mu d) = (sum_i x_i - acc) + (sum_i lam_i - mu) d.  Term by term, with
    |d| <= A + B and mu <= 1:
      acc is a sum of the n_g draws from +0.0 in some fixed order:   |sum_i x_i - acc| <= (n_g - 1) u A
      lam_i = fl(w_i / D), mu = fl(W / D) with the same D = fl(v + W), and W = sum_i w_i (1 + th_i), |th_i| <=
      (n_g - 1) u:  sum_i lam_i - mu = sum_i w_i (dl_i - th_i - dm) / D with |dl_i|, |dm| <= u, so
                                                                     |sum_i lam_i - mu| |d| <= (n_g + 1) u (A + B)
      member'_i = fl(x_i + fl(lam_i d)): u lam_i |d| + u (|x_i| + lam_i |d|) each; over the group
                                                                     u (A + 2 mu |d|) <= 3 u (A + B)
      total' = fl(acc + fl(mu d)): u mu |d| + u (|acc| + mu |d|)  <= 3 u (A + B)
      the test's own sum of the n_g values member'_i, in any order: (n_g - 1) u sum_i |member'_i| <= (n_g - 1) u (2 A + B)
                                                                     <= 2 (n_g - 1) u (A + B)
    Together ((n_g - 1) + (n_g + 1) + 3 + 3 + 2 (n_g - 1)) u (A + B) = (4 n_g + 4) u (A + B) = (2 n_g + 2) 2^-52 (A + B);
    one more 2^-52 (A + B) stands for every term of second order in u (each is below n_g^2 u^2 (A + B)).  That is of the
    order (n_g + 4) 2^-52 (sum |x_i| + |t|), with the constant written out."""
    return (2 * n_g + 3) * 2.0 ** -52 * (x_abs_sum + t_abs)
