"""The judge of the regime tests: prophet.stan's log-posterior (oracle/fbprophet_restated.py stan_neg_log_prob_grad,
the dense-A numpy statement) carried in np.longdouble, and the CONDITIONED bound of one quadratic-form evaluation
against it.  Shared by tests/test_regime_cases.py (the CPU oracle) and tests/test_gpu_regimes.py (the kernels).

The quadratic form keeps, at a reference point theta_ref, s0 = |r0|^2 (r0 = y - mu(theta_ref)), c = Z^T r0 and
M = Z^T Z (Z: the Jacobian of mu in k, m, delta, beta; mu is linear in them), and evaluates the data term
SSE / 2 sigma^2 at theta_ref + D with SSE = s0 - 2 c^T D + D^T M D.  Each of the three terms is rounded at its own
magnitude and the sum is divided by 2 sigma^2.  Two bounds are kept, with u = 2^-53 and every quantity on the right
computed here in long double:

STATED -- the terms of the quadratic form alone:

    |f - f_ld|     <= C u (s0 + 2 |c^T D| + |Z D|^2) / (2 sigma^2)               + C u |f_ld|
    |g_j - g_ld_j| <= C u |Z_j| (sqrt(s0) + |Z D|) / sigma^2                     + C u |g_ld_j|     (j: k, m, delta, beta)
    |g_s - g_ld_s| <= C u (s0 + 2 |c^T D| + |Z D|^2) / sigma^2                   + C u (T + |g_ld_s|)   (log sigma)

(|c_j| <= |Z_j| sqrt(s0) and |(M D)_j| <= |Z_j| |Z D| by Cauchy-Schwarz; |Z_j| the column norm).  It leaves out what
dominates at small sigma: a residual row r_t = y_t - mu_t is formed in float64 at the magnitude
a_t = |y_t| + sum_j |Z_tj theta_j| (~1 after absmax scaling) while |r_t| ~ sigma, in the residual pass of the quadratic
form and in a plain residual-form evaluation alike.  So the constant this bound needs is ~1 / sigma: 1.1e5 measured for
the oracle's quadratic form and 1.3e5 for its residual form (tests/test_regime_cases.py).

ROUNDED -- the same with that term, |a| = sqrt(sum a_t^2): the error of r0 enters s0 by 2 u |a| sqrt(s0), c^T D by
u |a| |Z D| and c_j by u |a| |Z_j|:

    f, g_s:  (s0 + 2 |c^T D| + |Z D|^2)  ->  (s0 + 2 |c^T D| + |Z D|^2 + 2 |a| (sqrt(s0) + |Z D|))
    g_j:     (sqrt(s0) + |Z D|)          ->  (sqrt(s0) + |Z D| + |a|)

Under it the oracle's two forms need a constant of ~2 on every regime, and a quadratic form that is never re-centred
needs > 100 on the low-sigma regimes.  Both constants are measured on the oracle and recorded in
tests/test_regime_cases.py."""
import numpy as np

from tests import helpers, regime_cases as rc

LD = np.longdouble
U = 2.0 ** -53


def literal_dat(name, T=rc.T_LONG):
    """(dat, th0) of the LITERAL model (fbprophet_restated.ProphetOracle.stan_data) for a linear regime series, on the
    canonical design values."""
    import pandas as pd
    from oracle.fbprophet_restated import ProphetOracle
    ds, y = rc.linear(name, T)
    with helpers.literal_on_canonical_design():
        m = ProphetOracle(growth='linear', seasonality_mode='additive', yearly_seasonality=(T >= rc.T_LONG),
                          weekly_seasonality=True, daily_seasonality=False)
        dat, th0 = m.stan_data(pd.DataFrame({'ds': pd.to_datetime(ds), 'y': y}))
    return dat, th0


def to_ld(dat):
    return {k: (v.astype(LD) if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else v) for k, v in dat.items()}


def ld_eval(dat_ld, theta):
    """f, g of the literal model in long double at a float64 theta."""
    from oracle.fbprophet_restated import stan_neg_log_prob_grad
    f, g = stan_neg_log_prob_grad(dat_ld, np.asarray(theta, dtype=np.float64).astype(LD))
    assert g.dtype == LD
    return f, g


def jacobian(dat_ld):
    """Z [T][2 + S + K] in long double: d mu / d (k, m, delta, beta) of linear growth with additive columns."""
    A, t, tc, X = dat_ld['A'], dat_ld['t'], dat_ld['t_change'], dat_ld['X']
    assert dat_ld['trend_indicator'] == 0 and not np.any(dat_ld['s_m'])
    return np.concatenate([t[:, None], np.ones_like(t)[:, None], A * (t[:, None] - tc[None, :]), X * dat_ld['s_a'][None, :]], axis=1)


def bound_terms(dat_ld, Z, theta_ref, theta):
    """(f_ld, g_ld, stated, rounded): the long-double value and gradient at theta, and the right-hand sides (bf, bg) of
    the two bounds above divided by C."""
    T = int(dat_ld['T'])
    ref, th = np.asarray(theta_ref, np.float64).astype(LD), np.asarray(theta, np.float64).astype(LD)
    lin = np.r_[0, 1, 3:len(th)]
    r0 = dat_ld['y'] - Z @ ref[lin]
    D = th[lin] - ref[lin]
    ZD = Z @ D
    s0, cD, zd2 = r0 @ r0, (Z.T @ r0) @ D, ZD @ ZD
    sig2 = np.exp(2 * th[2])
    a = np.abs(dat_ld['y']) + np.abs(Z) @ np.abs(th[lin])        # the magnitudes a residual row is rounded at
    na = np.sqrt(a @ a)
    zn = np.sqrt((Z * Z).sum(axis=0))
    f_ld, g_ld = ld_eval(dat_ld, theta)
    out = []
    for extra in (0, na):
        amp = s0 + 2 * abs(cD) + zd2 + 2 * extra * (np.sqrt(s0) + np.sqrt(zd2))
        bf = U * amp / (2 * sig2) + U * abs(f_ld)
        bg = np.zeros(len(th), LD)
        bg[lin] = U * zn * (np.sqrt(s0) + np.sqrt(zd2) + extra) / sig2 + U * np.abs(g_ld[lin])
        bg[2] = U * amp / sig2 + U * (T + abs(g_ld[2]))
        out.append((bf, bg))
    return f_ld, g_ld, out[0], out[1]


def eval_points(name, theta_ref):
    """The two evaluation points of a reference point: 1e-5 and 1e-3 away per parameter (a late and an early
    line-search trial), log sigma as at the reference."""
    rng = rc._rng('points:' + name, 0)
    out = []
    for sc in (1e-5, 1e-3):
        th = np.asarray(theta_ref, np.float64) + rng.normal(0, sc, len(theta_ref))
        th[2] = theta_ref[2]
        out.append(th)
    return out


def reference_points(name, T=rc.T_LONG):
    """The oracle's iterate after 50 iterations and its end point, for a linear regime series (quadratic form)."""
    from oracle import canon_lib as cl
    ds, y = rc.linear(name, T)
    return [cl.fit(rc.oracle_spec(T, max_iter=50), ds, y)['theta'], cl.fit(rc.oracle_spec(T), ds, y)['theta']]


def ratios(f, g, terms):
    """What the constant of the STATED and of the ROUNDED bound has to cover for this (f, g): the largest of
    |f - f_ld| / bf and |g - g_ld| / bg, for each."""
    f_ld, g_ld = terms[0], terms[1]
    ef, eg = abs(LD(f) - f_ld), np.abs(np.asarray(g, np.float64).astype(LD) - g_ld)
    return tuple(float(max(ef / bf, np.max(eg / bg))) for bf, bg in terms[2:])


def numpy_quadratic_form(dat, theta_ref, theta):
    """The same quadratic form in plain float64 numpy (s0, c, M at theta_ref): f, g.  The sensitivity check of the
    bound: with theta_ref fbprophet's initial point -- a form that is never re-centred -- it must MISS the bound on the
    low-sigma regimes."""
    Z = jacobian(dat).astype(np.float64)
    th, ref = np.asarray(theta, np.float64), np.asarray(theta_ref, np.float64)
    lin = np.r_[0, 1, 3:len(th)]
    r0 = dat['y'] - Z @ ref[lin]
    s0, c, M = r0 @ r0, Z.T @ r0, Z.T @ Z
    D = th[lin] - ref[lin]
    MD = M @ D
    sse = s0 - 2 * (c @ D) + D @ MD
    S = int(dat['S'])
    k, m, ls, delta, beta = th[0], th[1], th[2], th[3:3 + S], th[3 + S:]
    sig2 = np.exp(2 * ls)
    f = (0.5 * k * k / 25.0 + 0.5 * m * m / 25.0 + np.sum(np.abs(delta)) / dat['tau'] + 2.0 * sig2
         + 0.5 * np.sum((beta / dat['sigmas']) ** 2) + dat['T'] * ls + 0.5 * sse / sig2)
    g = np.zeros_like(th)
    g[lin] = (MD - c) / sig2
    g[0] += k / 25.0
    g[1] += m / 25.0
    g[2] = dat['T'] - sse / sig2 + 4.0 * sig2
    g[3:3 + S] += np.sign(delta) / dat['tau']
    g[3 + S:] += beta / dat['sigmas'] ** 2
    return f, g
