"""Extended-precision forecast reference -- TEST INFRASTRUCTURE ONLY.

Prophet.predict's point forecast written in fbprophet 0.5's own terms (piecewise_linear,
piecewise_logistic, fourier_series, ``trend * (1 + multiplicative) + additive``; see
oracle/fbprophet_restated.py), NOT in the kernel's order of operations:

  * t is the exact int64 difference ds - start divided by t_scale in long double;
  * the Fourier day value is the float64 fbprophet forms (ns / 1e9 / 86400); the argument
    2 pi k t / period, its sine and cosine and everything after them are long double;
  * a grid with S = 0 means what a fit without changepoints produces: fbprophet's dummy
    changepoint at t = 0 with delta 0 (the fitted delta is folded into k,
    tests/test_oracle.py::test_no_changepoints_is_fitted_on_fbprophets_dummy_changepoint).

Besides yhat it returns two error scales per element:

  M  the sum of the absolute values of every term of the forecast (the trend's terms, for
     logistic growth through the sigmoid's derivative; every |beta_j x_j| weighted by y_scale
     or by |trend|), so that a float64 evaluation in ANY order is within a small multiple of
     u M -- a relative error would fail where yhat crosses zero;
  D  the design term: sum over Fourier columns of |beta_j| w_j k (|theta_1| + k), with k the
     harmonic, theta_1 the base argument and w_j the column's weight.  It covers a float64
     argument whose rounding is amplified k times (|theta_1| ~ 1e5 rad for daily seasonality
     on 2026 dates) and the k^2 error growth of a harmonic recurrence.

``tolerance(M, D)`` = TOL_C u (M + D), u = 2^-53.  TOL_C is calibrated on oracle cn_predict
(bit-identical to the kernel by contract) in tests/test_forecast_ref.py.

Layout: theta rows are the kernel's, [k, m, log sigma, delta[n_changepoints], beta[K]]
(beta in original column order, after ALL n_changepoints delta slots; slots S.. of delta are
unused).  ``canon_theta`` maps a row to oracle cn_predict's layout (beta right after delta[S]).
"""
import numpy as np

LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))
U = 2.0 ** -53          # unit roundoff of float64
TOL_C = 4.0             # calibrated constant, see tests/test_forecast_ref.py::test_tolerance_calibrated_on_cn_predict


def model_K(model):
    return 2 * sum(int(o) for _, o, _ in model['seasonalities']) + len(model['extra_modes'])


def theta_stride(model):
    return 3 + int(model['n_changepoints']) + model_K(model)


def columns(model):
    """Per original design column: (seasonality index or -1, harmonic k or 0, is_sine, multiplicative)."""
    out = []
    for i, (_, order, mode) in enumerate(model['seasonalities']):
        for k in range(1, int(order) + 1):
            out.append((i, k, True, mode == 'multiplicative'))
            out.append((i, k, False, mode == 'multiplicative'))
    for mode in model['extra_modes']:
        out.append((-1, 0, False, mode == 'multiplicative'))
    return out


def canon_theta(model, theta_row, S):
    """Kernel layout -> cn_predict layout: [k, m, log sigma, delta[:S], beta]."""
    ncp = int(model['n_changepoints'])
    th = np.asarray(theta_row, dtype=np.float64)
    return np.concatenate([th[:3 + S], th[3 + ncp:3 + ncp + model_K(model)]])


def fourier_days(ds_ns):
    """Days since the epoch as fbprophet's fourier_series forms them (float64)."""
    return (np.asarray(ds_ns, dtype=np.int64).astype(np.float64) / 1e9) / (3600 * 24.)


def _per_series(a, N, H):
    a = np.asarray(a)
    return np.broadcast_to(a, (N, H)) if a.ndim == 1 else a


def predict(model, theta, y_scale, grid, ds_future, floor=None, cap=None, extra_future=None):
    """yhat, M, D -- each long double [N][H].

    model: {'growth': 'linear' | 'logistic', 'n_changepoints': int,
            'seasonalities': [(period_days, order, mode)], 'extra_modes': [mode]}
    theta [N][theta_stride], y_scale [N], grid: records with start_ns, t_scale_ns, S, t_change
    (1 or N of them), ds_future int64 [H] or [N][H], floor / cap [N] or None,
    extra_future [n_extra][H] or [N][n_extra][H] (None without extra columns)."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    N = theta.shape[0]
    ds = np.asarray(ds_future, dtype=np.int64)
    H = ds.shape[-1]
    ds = _per_series(ds, N, H)
    ncp, K = int(model['n_changepoints']), model_K(model)
    logistic = model['growth'] == 'logistic'
    g = np.asarray(grid)
    if len(g) == 1:
        g = np.repeat(g, N)
    S = g['S'].astype(np.int64)
    if (S < 0).any() or (S > ncp).any() or (g['t_scale_ns'] <= 0).any():
        raise ValueError('grid out of range for the model')
    ys = np.asarray(y_scale, dtype=np.float64).astype(LD)[:, None]
    fl = np.zeros((N, 1), dtype=LD) if floor is None else np.asarray(floor, np.float64).astype(LD)[:, None]
    # ---- trend (predict_trend: piecewise_linear / piecewise_logistic, scaled back) ----------------
    diff = ds - g['start_ns'][:, None]                                   # exact int64
    t = diff.astype(LD) / g['t_scale_ns'].astype(LD)[:, None]
    k = theta[:, 0].astype(LD)[:, None]
    m = theta[:, 1].astype(LD)[:, None]
    # changepoints padded to a common count: padding never becomes active (t_change = +inf, delta = 0);
    # S = 0 is fbprophet's dummy changepoint at 0 with delta 0
    Sm = max(1, int(S.max()))
    tc = np.full((N, Sm), np.inf, dtype=LD)
    dl = np.zeros((N, Sm), dtype=LD)
    for n in range(N):
        s = int(S[n])
        if s == 0:
            tc[n, 0] = 0
        else:
            tc[n, :s] = g['t_change'][n, :s]
            dl[n, :s] = theta[n, 3:3 + s]
    kt = np.broadcast_to(k, (N, H)).copy()
    mt = np.broadcast_to(m, (N, H)).copy()
    ka = np.broadcast_to(abs(k), (N, H)).copy()           # |k| + sum |delta| over the active changepoints
    ga = np.zeros((N, H), dtype=LD)                       # sum of the gammas' term scales
    if not logistic:
        gam = -np.where(np.isfinite(tc), tc, 0) * dl
        gsc = abs(gam)
    else:
        # gammas[i] = (t_s - m - sum(gammas)) * (1 - k_cum[i] / k_cum[i + 1])
        kc = np.concatenate([k, k + np.cumsum(dl, axis=1)], axis=1)
        gam = np.zeros((N, Sm), dtype=LD)
        gsc = np.zeros((N, Sm), dtype=LD)
        # (the offset after changepoint i is m_i r + t_i (1 - r), r = k_i / k_{i+1}: an error in m_i is carried
        # on times r, and products of r telescope to k_a / k_b -- so the terms of step i are its own)
        msum = m[:, 0].copy()
        for i in range(Sm):
            live = np.isfinite(tc[:, i]) & (kc[:, i + 1] != 0)
            tci = np.where(live, tc[:, i], 0)
            r = np.where(live, kc[:, i] / np.where(kc[:, i + 1] != 0, kc[:, i + 1], 1), 1)
            gam[:, i] = np.where(live, (tci - msum) * (1 - r), 0)
            gsc[:, i] = np.where(live, (abs(tci) + abs(msum)) * (1 + abs(r)), 0)
            msum = msum + gam[:, i]
    for i in range(Sm):
        act = t >= tc[:, i:i + 1]
        kt += np.where(act, dl[:, i:i + 1], 0)
        mt += np.where(act, gam[:, i:i + 1], 0)
        ka += np.where(act, abs(dl[:, i:i + 1]), 0)
        ga += np.where(act, gsc[:, i:i + 1], 0)
    if not logistic:
        trend_sc = kt * t + mt
        trend_m = ka * abs(t) + abs(m) + ga
        trend = trend_sc * ys                                # fbprophet adds df['floor'] = 0 for linear growth
        M_tr = trend_m * ys
    else:
        capsc = (np.asarray(cap, np.float64).astype(LD)[:, None] - fl) / ys
        z = kt * (t - mt)
        sg = 1 / (1 + np.exp(-z))
        trend = capsc * sg * ys + fl
        Z = ka * (abs(t) + abs(m) + ga) + abs(z)
        M_tr = abs(capsc) * ys * (sg + sg * (1 - sg) * Z) + abs(fl)
    # ---- seasonal features (fourier_series; extra columns as given) ---------------------------------
    cols = columns(model)
    beta = theta[:, 3 + ncp:3 + ncp + K].astype(LD)
    tdays = fourier_days(ds).astype(LD)
    add = np.zeros((N, H), dtype=LD)
    mul = np.zeros((N, H), dtype=LD)
    add_a = np.zeros((N, H), dtype=LD)
    mul_a = np.zeros((N, H), dtype=LD)
    dsc_a = np.zeros((N, H), dtype=LD)
    dsc_m = np.zeros((N, H), dtype=LD)
    nf = K - len(model['extra_modes'])
    ex = None
    if len(model['extra_modes']):
        ex = np.asarray(extra_future, dtype=np.float64)
        ex = np.broadcast_to(ex, (N,) + ex.shape) if ex.ndim == 2 else ex
    base = {}
    for j, (si, hk, is_sin, mult) in enumerate(cols):
        if si >= 0:
            period = LD(float(model['seasonalities'][si][0]))
            if si not in base:
                base[si] = abs(2 * PI_LD * tdays / period)
            arg = 2 * LD(hk) * PI_LD * tdays / period
            x = np.sin(arg) if is_sin else np.cos(arg)
            dj = abs(beta[:, j:j + 1]) * hk * (base[si] + hk)
        else:
            x = ex[:, j - nf, :].astype(LD)
            dj = None
        bx = beta[:, j:j + 1] * x
        if mult:
            mul += bx
            mul_a += abs(bx)
            if dj is not None:
                dsc_m += dj
        else:
            add += bx
            add_a += abs(bx)
            if dj is not None:
                dsc_a += dj
    yhat = trend * (1 + mul) + add * ys
    M = M_tr * (1 + mul_a) + abs(trend) * mul_a + ys * add_a
    D = abs(trend) * dsc_m + ys * dsc_a
    return yhat, M, D


def tolerance(M, D, c=TOL_C):
    return c * U * (np.asarray(M, dtype=np.float64) + np.asarray(D, dtype=np.float64))


def int_post_step(yhat, floor):
    """prophet_scorer.py:73-84 on a float forecast: ``astype(int)`` (truncation toward zero, int64),
    ``np.where(yhat < floor, floor, yhat)``, then the int32 cast of the output column.  Returns
    (values, outside): where the clamped value lies outside int32 the reference has no result (its
    IntegerType cast fails) and ``outside`` is True; values there are the saturated ones the kernel
    returns (include/tsf.h)."""
    y = np.asarray(yhat, dtype=np.float64)
    fl = np.broadcast_to(np.asarray(floor, dtype=np.float64).reshape(-1, *([1] * (y.ndim - 1))), y.shape)
    iv = np.clip(np.trunc(y), -2.0 ** 62, 2.0 ** 62).astype(np.int64)    # astype(int)
    r = np.where(iv < fl, fl, iv)                                        # np.where(yhat < floor, floor, yhat)
    outside = ~((r >= -2.0 ** 31) & (r < 2.0 ** 31))
    return np.trunc(np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int32), outside
