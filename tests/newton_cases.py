"""Newton case matrix shared by tests/test_newton_ref.py (CPU: the reference's calibration on oracle cn_newton)
and tests/test_gpu_newton.py (the kernels judged against the reference).

Each case is (spec, ds, y [N][T], floor [N], cap [N], extra [n_extra][T] or None).  The conditioning cases put
the finite-difference Hessian where the Cholesky route meets tiny pivots and where the eigen route's |lambda|
differs most from it: duplicate regressor columns under wide priors (condition numbers up to ~1e14), a holiday
column without rows in the history, a constant regressor (collinear with m), a logistic cap barely above max y
and an almost constant y."""
import zlib

import numpy as np

from tests import helpers

DAY_NS = helpers.DAY_NS


def _spec(growth='linear', mode='additive', seas=(helpers.WEEKLY,), extra=(), **kw):
    from time_series_spark_amd import _lib, forecaster as fc
    return fc.ModelSpec(growth=growth, seasonality_mode=mode, seasonalities=[dict(s) for s in seas],
                        extra=[dict(e) for e in extra], algorithm=_lib.ALGO_NEWTON, **kw)


def _panel(N, T, growth, seed, ds=None):
    from time_series_spark_amd import synth
    d, y = synth.make_panel(N, T, growth, seed=seed)
    return (d if ds is None else ds), np.ascontiguousarray(y, dtype=np.float64)


N_SERIES = 3


def make(name, N=N_SERIES):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    fl = np.zeros(N)
    if name.startswith('T'):                     # T<n>: linear additive, weekly, n rows
        T = int(name[1:])
        ds, y = _panel(N, T, 'linear', 751 + T)
        # (short histories the model interpolates, sigma -> 0: the quadratic-form halving trials fall back to the
        # residual form there, see tests/test_newton_ref.py::test_quadratic_form_trials_when_the_model_interpolates)
        return _spec(), ds, y, fl, y.max(axis=1) * 1.1, None
    if name == 'ref_logistic_mult':              # the reference's own model
        ds, y = _panel(N, 90, 'logistic', 17)
        return _spec('logistic', 'multiplicative'), ds, y, fl, y.max(axis=1) * 1.1, None
    if name == 'K0':                             # no seasonality: fbprophet's single zero column
        ds, y = _panel(N, 40, 'linear', 5)
        return _spec(seas=(), extra=[{'name': 'zeros'}]), ds, y, fl, y.max(axis=1) * 1.1, np.zeros((1, 40))
    if name in ('K28', 'K29'):                   # the quadratic-form limit: 28 design columns, then 29
        ds, y = _panel(N, 60, 'linear', 29)
        nx = int(name[1:]) - 6
        ex = rng.normal(0, 1, (nx, 60))
        return _spec(extra=[{'name': 'x%d' % i} for i in range(nx)]), ds, y, fl, y.max(axis=1) * 1.1, ex
    if name in ('P63', 'P64', 'P65'):            # 3 + 25 + K, one column mode
        ds, y = _panel(N, 60, 'linear', 63)
        nx = int(name[1:]) - 3 - 25 - 6
        ex = rng.normal(0, 1, (nx, 60))
        return (_spec(extra=[{'name': 'x%d' % i} for i in range(nx)], eval_form=1), ds, y, fl,
                y.max(axis=1) * 1.1, ex)
    if name == 'P127':                           # the widest Newton model: 60 changepoints, K = 64 (46 seasonal columns)
        ds, y = _panel(N, 99, 'linear', 128)
        seas = (helpers.YEARLY, helpers.WEEKLY, {'name': 'monthly', 'period': 30.5, 'fourier_order': 5},
                {'name': 'half_week', 'period': 3.5, 'fourier_order': 5})
        ex = rng.normal(0, 1, (18, 99))
        return (_spec(seas=seas, extra=[{'name': 'x%d' % i, 'prior_scale': 0.1} for i in range(18)], n_changepoints=60,
                      eval_form=1), ds, y, fl, y.max(axis=1) * 1.1, ex)
    if name == 'mixed':                          # additive weekly + multiplicative regressors, P <= 64
        ds, y = _panel(N, 80, 'linear', 6)
        ex = rng.normal(0, 1, (2, 80))
        return (_spec(extra=[{'name': 'x0', 'mode': 'multiplicative'}, {'name': 'x1'}]), ds, y, fl,
                y.max(axis=1) * 1.1, ex)
    if name == 'holidays':                       # indicator columns and a regressor
        ds, y = _panel(N, 90, 'linear', 44)
        ex = np.zeros((3, 90))
        ex[0, [10, 40, 70]] = 1.0
        ex[1, [25, 26]] = 1.0
        ex[2] = rng.normal(0, 1, 90)
        return _spec(extra=[{'name': 'h0'}, {'name': 'h1'}, {'name': 'r', 'prior_scale': 3.0}]), ds, y, fl, y.max(axis=1) * 1.1, ex
    if name == 'steep_logistic':                 # a near-step history: large k, a strongly non-quadratic objective
        from time_series_spark_amd import synth
        ds = synth.daily_grid(60)
        t = np.arange(60)
        y = np.stack([10 + 90 / (1 + np.exp(-(t - 30.3 + 2 * i) * 3.0)) + rng.normal(0, 0.3, 60) for i in range(N)])
        return _spec('logistic', seas=(), extra=[{'name': 'zeros'}]), ds, y, fl, np.full(N, 105.0), np.zeros((1, 60))
    if name == 'logistic_resid':                 # residual form, logistic / additive
        ds, y = _panel(N, 60, 'logistic', 8)
        return _spec('logistic'), ds, y, fl, y.max(axis=1) * 1.1, None
    if name == 'linear_mult':                    # residual form, linear / multiplicative
        ds, y = _panel(N, 60, 'linear', 9)
        return _spec('linear', 'multiplicative'), ds, y, fl, y.max(axis=1) * 1.1, None
    if name.startswith('dup'):                   # dup<log10 prior>: two identical regressor columns
        ps = 10.0 ** int(name[3:])
        ds, y = _panel(N, 60, 'linear', 70)
        x = rng.normal(0, 1, 60)
        ex = np.stack([x, x])
        return (_spec(extra=[{'name': 'a', 'prior_scale': ps}, {'name': 'b', 'prior_scale': ps}]), ds, y, fl,
                y.max(axis=1) * 1.1, ex)
    if name == 'empty_holiday':                  # a holiday column with no rows in the history
        ds, y = _panel(N, 60, 'linear', 71)
        return _spec(extra=[{'name': 'h'}]), ds, y, fl, y.max(axis=1) * 1.1, np.zeros((1, 60))
    if name == 'const_regressor':                # collinear with m
        ds, y = _panel(N, 60, 'linear', 72)
        return _spec(extra=[{'name': 'c'}]), ds, y, fl, y.max(axis=1) * 1.1, np.full((1, 60), 2.0)
    if name == 'tight_cap':                      # logistic, cap barely above max y
        ds, y = _panel(N, 60, 'logistic', 73)
        return _spec('logistic'), ds, y, fl, y.max(axis=1) * (1 + 1e-6), None
    if name == 'flat_y':                         # almost constant y
        ds, y = _panel(N, 60, 'linear', 74)
        y = 100.0 + 1e-9 * (y - y.mean(axis=1, keepdims=True))
        return _spec(), ds, y, fl, y.max(axis=1) * 1.1, None
    raise KeyError(name)


SHAPES = ['T3', 'T10', 'T31', 'T60', 'T90', 'T99', 'K0', 'K28', 'K29', 'P63', 'P64', 'P65', 'mixed', 'holidays',
          'ref_logistic_mult', 'logistic_resid', 'linear_mult', 'steep_logistic']
CONDITIONING = ['dup1', 'dup3', 'dup5', 'empty_holiday', 'const_regressor', 'tight_cap', 'flat_y']


def oracle_spec(spec):
    """helpers.oracle_spec for Newton: the quadratic-form Newton kernels stop at 28 design columns, wider linear /
    additive models run Newton in residual form (tsf_api.hip run_fit), and the twin is told so."""
    csp = helpers.oracle_spec(spec)
    if spec.K > 28:
        csp.eval_mode = 0
    return csp


def oracle_fits(name, n, max_iter=None, ks=None):
    """(Problem, cn_newton's full fit, its iterates [init, theta_1, ..., theta_n_iter]) for series n; with ks, only
    the iterates k in ks are computed (None elsewhere: every capped fit reruns the iterations before it)."""
    from oracle import canon_lib as cl, newton_ref as nr
    spec, ds, y, fl, cap, ex = make(name)
    csp = oracle_spec(spec)
    prob = nr.Problem(csp, ds, y[n], fl[n], cap[n], ex)
    full = cl.fit_newton(csp, ds, y[n], fl[n], cap[n], ex)
    last = full['n_iter'] if max_iter is None else min(full['n_iter'], max_iter)
    if callable(ks):
        ks = ks(full['n_iter'])
    ths = [prob.theta0]
    for k in range(1, last + 1):
        if ks is not None and k not in ks:
            ths.append(None)
            continue
        csp.max_iter = k
        ths.append(cl.fit_newton(csp, ds, y[n], fl[n], cap[n], ex)['theta'])
    return prob, full, ths
