"""The contract of include/tsf.h "temporal reconciliation" restated in numpy, for tests/test_temporal_ref.py (CPU) and
tests/test_gpu_temporal.py.  Every function performs the header's operations in the header's order on float64 arrays
(numpy's elementwise +, -, *, / are the IEEE operations; nothing here fuses), so a comparison with the library is bit
for bit."""
import numpy as np

from tests import reconcile_ref as rr


def shares(N, H, w0, w1, w, v):
    """tsf_temporal_shares: windows [w0[k], w1[k]), w [N][H] or None (all 1.0), v [N][K] (NaN: the window is not
    reconciled) -> (share [N][H], share_total [N][K]).  W from +0.0 in ascending row order; share = w / (v + W),
    share_total = W / (v + W); NaN v: +0.0 in the window's share cells, NaN in share_total; a row in no window: +0.0."""
    K = len(w0)
    w = np.ones((N, H)) if w is None else np.asarray(w, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    share, share_total = np.zeros((N, H)), np.zeros((N, K))
    for n in range(N):
        for k in range(K):
            if np.isnan(v[n, k]):
                share_total[n, k] = np.nan
                continue
            W = np.float64(0.0)
            for h in range(w0[k], w1[k]):
                W = W + w[n, h]
            D = v[n, k] + W
            for h in range(w0[k], w1[k]):
                share[n, h] = w[n, h] / D
            share_total[n, k] = W / D
    return share, share_total


def window_sums(x, w0, w1):
    """x [N][H][...] -> [N][K][...]: x[a], then + x[h] for h = a + 1 .. b - 1 in row order"""
    out = np.empty((x.shape[0], len(w0)) + x.shape[2:])
    for k, (a, b) in enumerate(zip(w0, w1)):
        c = x[:, a].copy()
        for h in range(a + 1, b):
            c = c + x[:, h]
        out[:, k] = c
    return out


def reconcile(x, t, w0, w1, share, share_total):
    """The rule on draws x [N][H][S], t [N][K][S] (or on the point forecasts y [N][H], yp [N][K]) -> (x', win'):
    d = t - sum where share_total is not NaN, +0.0 where it is; x' = x + share * d on the window's rows (a row in no
    window as it is); win' = sum + share_total * d (the NaN read as +0.0)."""
    active = ~np.isnan(share_total)
    mu = np.where(active, share_total, 0.0)
    tail = (1,) * (x.ndim - 2)
    s = window_sums(x, w0, w1)
    d = np.zeros_like(s)
    sel = active.reshape(active.shape + tail) & np.ones(s.shape, dtype=bool)
    d[sel] = (t - s)[sel]
    win = s + mu.reshape(mu.shape + tail) * d
    xr = x.copy()
    for k, (a, b) in enumerate(zip(w0, w1)):
        for h in range(a, b):
            xr[:, h] = x[:, h] + share[:, h].reshape((-1,) + tail) * d[:, k]
    return xr, win


def contract(x, t, y, yp, w0, w1, share, share_total, levels):
    """Everything tsf_predict_temporal returns, from the two models' draws x [N][H][S], t [N][K][S] and point forecasts
    y [N][H], yp [N][K]: dict of samples, win_samples, yhat, total, q, cum_q [N][Q][H], win_q [N][Q][K]."""
    xr, win = reconcile(x, t, w0, w1, share, share_total)
    yr, total = reconcile(y, yp, w0, w1, share, share_total)
    r = dict(samples=xr, win_samples=win, yhat=yr, total=total)
    if len(levels):
        r['q'], r['cum_q'] = rr.q_and_cum_q(xr, levels)
        r['win_q'] = np.moveaxis(rr.quantiles(win, levels), -1, 1)
    return r


def coherence_bound(m, x_abs_sum, d_abs):
    """A bound on |sum_h x'_h - win'| for one sample of an active window of m rows, u = 2^-53 the unit roundoff, first
    order in u, with A = sum_h |x_h| and |d| the computed incoherence of the sample (the same d on both sides, whatever
    its own rounding).

    Exact arithmetic on the computed sum, d, lam_h, mu would give
      sum_h (x_h + lam_h d) - (sum + mu d) = (sum_h x_h - sum) + (sum_h lam_h - mu) d.
    Term by term, with mu <= 1 and sum_h lam_h <= 1 + O(u):
      sum is the sequential sum of the m draws:                          |sum_h x_h - sum| <= (m - 1) u A
      lam_h = fl(w_h / D), mu = fl(W / D), the same D = fl(v + W), W = sum_h w_h (1 + th_h) with |th_h| <= (m - 1) u
      (the first add, to +0.0, is exact): sum_h lam_h - mu = sum_h w_h (dl_h - th_h - dm) / D, |dl_h|, |dm| <= u:
                                                                         |sum_h lam_h - mu| |d| <= (m + 1) u |d|
      x'_h = fl(x_h + fl(lam_h d)): u lam_h |d| + u (|x_h| + lam_h |d|) each; over the window   u (A + 2 |d|)
      win' = fl(sum + fl(mu d)):    u mu |d| + u (|sum| + mu |d|)                            <= u (A + 2 |d|)
      the test's own sequential sum of the m values x'_h: (m - 1) u sum_h |x'_h|             <= (m - 1) u (A + |d|)
    Together A's coefficient is (m - 1) + 1 + 1 + (m - 1) = 2 m and |d|'s (m + 1) + 2 + 2 + (m - 1) = 2 m + 4, so the sum
    is at most (2 m + 4) u (A + |d|) = (m + 2) 2^-52 (A + |d|); one more 2^-52 (A + |d|) stands for every term of second
    order in u (each is below m^2 u^2 (A + |d|)).  The multiple of m 2^-52 (A + |d|) is therefore (m + 3) / m: 4 for a
    one-row window, 10 / 7 for a week.  The same holds for the point forecasts with y, ysum, dy in the place of x, sum,
    d."""
    return (m + 3) * 2.0 ** -52 * (x_abs_sum + d_abs)
