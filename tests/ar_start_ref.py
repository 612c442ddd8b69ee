"""Reference for the conditioned start of the AR(1) noise chain (include/tsf.h "the conditioned start"): numpy
restatements of tsf_residual_last, of the host constants tsf_set_noise_ar_start stores (p0, c0, m0), of
tsf_noise_ar_mean's rows and of the conditioned chain, with the laws the conditioned draw must obey.  Written from the
contract in include/tsf.h, not from the kernels.  The draw has switches for three mutants, so the CPU suite shows that
the checks reject a subtly wrong start.

The laws, for iid standard normal z_h, |phi| < 1, c = sqrt(1 - phi^2), p0 = phi^steps, c0 = sqrt(1 - p0^2) and a last
residual r (here in units of sigma * y_scale):
    e_0 = c0 z_0,  e_h = phi e_(h-1) + c z_h,  x_h = m_h + e_h  with  m_h = p0 phi^h r
    =>  E[x_h] = m_h,  v_h = Var(e_h) = 1 - (p0 phi^h)^2   (v_h = phi^2 v_(h-1) + c^2, v_0 = c0^2),
        Cov(e_i, e_j) = phi^(j-i) v_i  for i <= j,
        V_m = Var(e_0 + ... + e_m):  g_0 = v_0, V_0 = v_0;  g_m = v_m + phi g_(m-1)  (g_m = Cov(S_m, e_m)),
                                     V_m = V_(m-1) + v_m + 2 phi g_(m-1).
For a zero-mean Gaussian pair, Var(a b) = Var(a) Var(b) + Cov(a, b)^2; a sample variance of n Gaussian values has
relative standard error sqrt(2 / (n - 1)).  As h grows p0 phi^h -> 0 and every law tends to the stationary chain's
(tests/ar_ref.py)."""
import math

import numpy as np

from tests import ar_ref as ar

AR_OK, AR_NO_ROW = 0, -52
START_MUTANTS = ('c0_one', 'p0_phi', 'no_mean_in_yhat')


# ---- tsf_residual_last ----------------------------------------------------------------------------------------

def residual_last_series(y, fitted):
    """One series: y [T] in its own dtype, fitted [T] double -> (last_resid, last_gap, status)"""
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.asarray(y).astype(np.float64) - np.asarray(fitted, dtype=np.float64)
    T = len(r)
    for t in range(T - 1, -1, -1):
        if np.isfinite(r[t]):
            return float(r[t]), T - 1 - t, AR_OK
    return 0.0, T, AR_NO_ROW


def residual_last(y, fitted, offsets=None):
    """tsf_residual_last on a panel (aligned [N][T], or 1-D with offsets [N + 1]) -> dict(last_resid, last_gap, status)"""
    y, fitted = np.asarray(y), np.asarray(fitted, dtype=np.float64)
    if offsets is None:
        rows = [(y[i], fitted[i]) for i in range(y.shape[0])]
    else:
        rows = [(y[a:b], fitted[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    res = [residual_last_series(a, b) for a, b in rows]
    N = len(res)
    cols = list(zip(*res)) if N else [[]] * 3
    return {'last_resid': np.array(cols[0], dtype=np.float64).reshape(N), 'last_gap': np.array(cols[1], dtype=np.int32).reshape(N),
            'status': np.array(cols[2], dtype=np.int32).reshape(N)}


# ---- the host constants and the mean --------------------------------------------------------------------------

def p0_of(phi, steps, mutant=None):
    """phi multiplied by itself steps - 1 more times, one rounding each; the loop stops at the first zero"""
    phi = np.float64(phi)
    p = phi
    if mutant == 'p0_phi':
        return float(p)
    for _ in range(int(steps) - 1):
        if p == 0.0:
            break
        p = p * phi
    return float(p)


def start_constants(phi, resid, steps, mutant=None):
    """(p0, c0, m0), each [N], as tsf_set_noise_ar_start stores them: products, a subtraction, IEEE sqrt"""
    assert mutant is None or mutant in START_MUTANTS
    phi, resid = np.atleast_1d(np.asarray(phi, dtype=np.float64)), np.atleast_1d(np.asarray(resid, dtype=np.float64))
    steps = np.atleast_1d(steps)
    p0 = np.array([p0_of(p, s, mutant) for p, s in zip(phi, steps)], dtype=np.float64)
    with np.errstate(under='ignore'):
        c0 = np.ones_like(p0) if mutant == 'c0_one' else np.sqrt(1.0 - p0 * p0)
        m0 = resid * p0
    return p0, c0, m0


def mean_rows(phi, resid, steps, H, mutant=None):
    """tsf_noise_ar_mean: [N][H], mean[i][0] = m0, mean[i][h] = phi * mean[i][h - 1]"""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    _, _, m0 = start_constants(phi, resid, steps, mutant)
    out = np.zeros((len(phi), H))
    m = m0.copy()
    with np.errstate(under='ignore'):
        for h in range(H):
            out[:, h] = m
            m = phi * m
    return out


# ---- the conditioned chain and draw ---------------------------------------------------------------------------

def chain(z, phi, c0, axis=0):
    """The conditioned chain along `axis` of z at one phi: e_0 = fl(c0 z_0), e_h = fl(fl(phi e_(h-1)) + fl(c z_h));
    phi == 0 gives z itself (the independent expression, whatever c0 is)."""
    z = np.moveaxis(np.asarray(z, dtype=np.float64), axis, 0)
    phi = float(phi)
    if phi == 0.0:
        return np.moveaxis(z.copy(), 0, axis)
    c = float(ar.noise_c(phi))
    e = np.empty_like(z)
    for h in range(z.shape[0]):
        e[h] = float(c0) * z[h] if h == 0 else phi * e[h - 1] + c * z[h]
    return np.moveaxis(e, 0, axis)


def draw(z, phi, resid, steps, base=None, scale=1.0, mutant=None):
    """One series of the conditioned draw on a model whose sample is base_h + noise (trend * (1 + mult) = +0.0, the
    additive piece base [H], default zeros; sigma * y_scale = scale): z [H][n] the standard normals ->
    (yhat [H], samples [H][n]) with samples = (0 + (base + m_h)) + (e_h * scale) and yhat = base + m_h, the contract's
    order of the adds.  phi == 0: neither is touched by resid."""
    assert mutant is None or mutant in START_MUTANTS
    z = np.asarray(z, dtype=np.float64)
    H = z.shape[0]
    base = np.zeros(H) if base is None else np.asarray(base, dtype=np.float64)
    if float(phi) == 0.0:
        return base.copy(), (0.0 + base[:, None]) + z * scale
    _, c0, _ = start_constants(phi, resid, steps, mutant)
    m = mean_rows(phi, resid, steps, H, mutant)[0]
    e = chain(z, phi, c0[0])
    xa = base + m
    yhat = base.copy() if mutant == 'no_mean_in_yhat' else base + m
    return yhat, (0.0 + xa[:, None]) + e * scale


# ---- the laws -------------------------------------------------------------------------------------------------

def law_mean(phi, r, steps, H):
    """m_h = phi^(steps + h) r, [H]"""
    return r * float(phi) ** (int(steps) + np.arange(H))


def law_variance(phi, steps, H):
    """v_h = 1 - (phi^(steps + h))^2, [H]"""
    return 1.0 - (float(phi) ** (int(steps) + np.arange(H))) ** 2


def sum_variance(phi, steps, H):
    """V_m = Var(e_0 + ... + e_m) for m < H, by the recursion of the module's docstring"""
    v = law_variance(phi, steps, H)
    V, g = np.zeros(H), np.zeros(H)
    V[0] = g[0] = v[0]
    for m in range(1, H):
        g[m] = v[m] + phi * g[m - 1]
        V[m] = V[m - 1] + v[m] + 2.0 * phi * g[m - 1]
    return V


def start_law_stats(x, center, phi, r, steps, lags=(1, 2, 5), pair_row=0, sum_rows=(1, 7, 31)):
    """The statistics of conditioned draws x [R][n] (R rows in order, n independent samples, in units of sigma *
    y_scale, the model's deterministic part removed) and of their point forecast center [R] (alike) against the laws
    above -> [(name, 'z' | 'p', value)]: each z standard normal under the laws (to the normal approximation of a mean
    over n); the p of the point forecast is 1 where it is the law's mean to 1e-12 (relative to max(1, |r|)) and 0
    otherwise.  Needs R > max(sum_rows) and pair_row + max(lags) < R."""
    R, n = x.shape
    m, v, V = law_mean(phi, r, steps, R), law_variance(phi, steps, R), sum_variance(phi, steps, R)
    d = x - m[:, None]
    out = []
    for h in (0, R // 2, R - 1):
        out.append(('row %d: mean' % h, 'z', d[h].mean() * math.sqrt(n / v[h])))
        out.append(('row %d: variance' % h, 'z', ((d[h] ** 2).mean() / v[h] - 1.0) / math.sqrt(2.0 / n)))
        out.append(('row %d: yhat is the law\'s mean' % h, 'p',
                    1.0 if abs(center[h] - m[h]) <= 1e-12 * max(1.0, abs(r)) else 0.0))
    i = pair_row
    for k in lags:
        cov = phi ** k * v[i]
        out.append(('lag %d from row %d: mean(e_i e_j) - phi^k v_i' % (k, i), 'z',
                    ((d[i] * d[i + k]).mean() - cov) / math.sqrt((v[i] * v[i + k] + cov * cov) / n)))
    cs = np.cumsum(d, axis=0)
    for k in sum_rows:
        out.append(('running sum at row %d: mean' % k, 'z', cs[k].mean() * math.sqrt(n / V[k])))
        out.append(('running sum at row %d: variance' % k, 'z', (cs[k].var(ddof=1) / V[k] - 1.0) / math.sqrt(2.0 / (n - 1))))
    return out


# ---- the accuracy claim: a planted panel ----------------------------------------------------------------------

PLANT_N, PLANT_T, PLANT_HOLD, PLANT_PHI = 256, 200, 8, 0.6


def planted_panel(seed, N=PLANT_N, T=PLANT_T, hold=PLANT_HOLD, phi=PLANT_PHI, sd=3.0):
    """N series of T + hold daily rows: level 100, a trend, a weekly sine of amplitude 5 and stationary Gaussian AR(1)
    noise of deviation sd -> (t [T + hold], y [N][T + hold], X [T + hold][4]: the true design 1, t, sin, cos)"""
    rng = np.random.default_rng(seed)
    t = np.arange(T + hold, dtype=np.float64)
    slope, phase = rng.uniform(0.0, 0.1, (N, 1)), rng.uniform(0.0, 2.0 * math.pi, (N, 1))
    y = 100.0 + slope * t + 5.0 * np.sin(2.0 * math.pi * t / 7.0 + phase) + ar.synth_ar1(rng, N, T + hold, phi, sd=sd)
    X = np.stack([np.ones_like(t), t, np.sin(2.0 * math.pi * t / 7.0), np.cos(2.0 * math.pi * t / 7.0)], axis=1)
    return t, y, X


def least_squares_forecast(y, X, T):
    """least squares of each series' first T rows on the design -> the fitted values of every row, [N][T + hold]"""
    beta = np.linalg.lstsq(X[:T], y[:, :T].T, rcond=None)[0]
    return (X @ beta).T


def accuracy_ratios(y_hist, fitted_hist, y_future, yhat_future, phi, lead=1, rows=((0, 1), (0, 3))):
    """The pooled squared error of the corrected forecast yhat_future + mean_rows over that of yhat_future, on the held-
    back rows [a, b) of each pair of `rows`; the correction from residual_last of (y_hist, fitted_hist) and phi [N]
    (series with phi == 0 are left as they are) -> (ratios, corrected [N][H])"""
    last = residual_last(y_hist, fitted_hist)
    H = y_future.shape[1]
    mean = mean_rows(phi, last['last_resid'], last['last_gap'].astype(np.int64) + lead, H)
    corrected = np.where((np.asarray(phi) != 0.0)[:, None], yhat_future + mean, yhat_future)
    ratios = [float(((y_future[:, a:b] - corrected[:, a:b]) ** 2).sum() / ((y_future[:, a:b] - yhat_future[:, a:b]) ** 2).sum())
              for a, b in rows]
    return ratios, corrected
