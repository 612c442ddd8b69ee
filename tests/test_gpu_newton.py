"""Stan's Newton kernels judged iteration by iteration against the extended-precision reference
(oracle/newton_ref.py), on every route the library has for it, over the case matrix of tests/newton_cases.py.

For each case the GPU fit runs once per k with max_iter = k, so that iterate k of every series is on record;
the capped runs must reproduce the uncapped run bit for bit.  Each judged iteration starts from the GPU's own
iterate k - 1 (iteration 1 from the init of canon_lib.design): a well-posed step must lie on the reference
step line at an admissible 2^-j within tolerance, every step must not lower lp_LD beyond the margin; status,
n_iter, fval and (where no halving decision was ambiguous) n_eval follow the reference; and each case is
bit-identical to oracle cn_newton.  Every iteration of series 0 is judged (every series of the conditioning
cases) and a seeded sample of the others; models wider than 64 parameters and fits of more than 300
iterations get a sample of series 0 too."""
import multiprocessing as mproc
import os
import time

import numpy as np
import pytest

from tests import helpers, newton_cases as nc

pytestmark = pytest.mark.gpu

# route -> [(case, route switches, how to call)]
ROUTES = {
    'newton_quad': [(c, {'TSF_NEWTON_BATCH': '0'}, 'aligned')
                    for c in ['T2', 'T3', 'T5', 'T10', 'T31', 'T60', 'T90', 'T99', 'K0', 'K28', 'holidays', 'dup1', 'dup3', 'dup5',
                              'empty_holiday', 'const_regressor', 'flat_y']],
    'newton_batch': [(c, {'TSF_NEWTON_BATCH': '2'}, 'tiled') for c in ['T60', 'dup5']],
    'newton_batch_lcap': [(c, {'TSF_NEWTON_BATCH': '2', 'TSF_NEWTON_LCAP': '50'}, 'tiled') for c in ['T90']],
    'newton_kernel': [(c, {}, 'aligned') for c in ['ref_logistic_mult', 'logistic_resid', 'linear_mult', 'tight_cap',
                                                  'steep_logistic', 'K29', 'P63', 'P64']],
    'newton_kernel2': [(c, {}, 'aligned') for c in ['P65', 'P127', 'mixed']],
    'fit_ragged': [(c, {}, 'ragged') for c in ['T60', 'ref_logistic_mult', 'dup3']],
}
RAGGED_CUTS = (1.0, 0.7, 0.5)           # series n keeps the first cut * T rows
WIDE = 64              # wider models: a sample of iterations of every series
LONG = 300             # longer fits (short histories can take thousands): a sample too
MAX_WAVES_PER_CU = 40  # above what a CU holds of 64-lane workgroups
N_CU = 256             # compute units of an MI355X


def _n_tiled():
    """Series of a 'tiled' call: newton_batch_shape (tsf_inst_quad.hip) takes the several-series-per-wave kernel
    only from 2 x (resident workgroups per CU) x n_cu series on (TSF_NEWTON_BATCH = 2); below that the call quietly
    runs the one-series-per-wave kernel.  2 x MAX_WAVES_PER_CU x N_CU is above that bound."""
    return 2 * MAX_WAVES_PER_CU * N_CU


def _cuts(T):
    return [max(3, int(T * c)) for c in RAGGED_CUTS]


def _series(name, n, how):
    spec, ds, y, fl, cap, ex = nc.make(name)
    if how == 'ragged':
        c = _cuts(len(ds))[n]
        return spec, ds[:c], y[n][:c], fl[n], cap[n], None if ex is None else np.ascontiguousarray(ex[:, :c])
    return spec, ds, y[n], fl[n], cap[n], ex


def _fit(spec, name, how, max_iter=None):
    from time_series_spark_amd import forecaster as fc
    if max_iter is not None:
        spec = type(spec).from_dict(dict(spec.to_dict(), lbfgs=dict(spec.lbfgs, max_iter=int(max_iter))))
    _, ds, y, fl, cap, ex = nc.make(name)
    if how == 'aligned':
        return fc.fit_aligned(spec, ds, y, floor=fl, cap=cap, extra=ex)
    if how == 'tiled':          # the case's series repeated: series n is series n % N of the case
        idx = np.arange(_n_tiled()) % len(y)
        return fc.fit_aligned(spec, ds, np.ascontiguousarray(y[idx]), floor=fl[idx], cap=cap[idx], extra=ex)
    cuts = _cuts(len(ds))
    off = np.concatenate([[0], np.cumsum(cuts)]).astype(np.int64)
    exr = None if ex is None else np.concatenate([ex[:, :c] for c in cuts], axis=1)
    return fc.fit_ragged(spec, off, np.concatenate([ds[:c] for c in cuts]),
                         np.concatenate([y[i][:c] for i, c in enumerate(cuts)]), floor=fl, cap=cap, extra=exr)


def _canon(spec, row, S):
    ncp = spec.n_changepoints
    return np.concatenate([row[:3 + S], row[3 + ncp:3 + ncp + spec.K]])


def _judge(arg):
    from oracle import newton_ref as nr
    name, n, how, thetas, status, n_iter, n_eval, fval, steps = arg
    spec, ds, y, fl, cap, ex = _series(name, n, how)
    prob = nr.Problem(nc.oracle_spec(spec), ds, y, fl, cap, ex)
    thetas = [prob.theta0] + list(thetas)
    rep, _ = nr.judge_fit(prob, thetas, status, n_iter, n_eval, fval, judge_steps=steps)
    return name, n, how, rep


def _run_case(name, switches, how):
    """GPU fits of one case, uncapped and capped at every k an iteration to be judged needs; checks them against
    each other and against the twin, and returns the judge's work items."""
    from oracle import canon_lib as cl
    spec = nc.make(name)[0]
    for k, v in switches.items():
        helpers.routes[k] = v
    try:
        full = _fit(spec, name, how)
        N = nc.N_SERIES
        if how == 'tiled':
            NT = len(full.theta)
            assert NT == _n_tiled()
            for name_ in ('theta', 'fval', 'n_iter', 'n_eval', 'status'):
                v = getattr(full, name_)
                assert np.array_equal(v, v[np.arange(NT) % N]), name_      # every copy of a series, the same bits
        rng = np.random.default_rng(len(name) * 31 + N)
        plan = []
        for n in range(N):
            ni = int(full.n_iter[n])
            wide = spec.theta_stride > WIDE
            if (n == 0 or name in nc.CONDITIONING) and not wide and ni <= LONG:
                steps = None
                need = set(range(1, ni + 1))
            else:
                pick = rng.choice(np.arange(1, ni + 1), min(10 if ni <= LONG else 4, ni), replace=False)
                steps = sorted(set([1, ni] + [int(v) for v in pick]))
                need = set(steps) | set(k - 1 for k in steps) | {ni}
            plan.append((ni, steps, need - {0}))
        needed = sorted(set().union(*[p[2] for p in plan]))
        caps = {k: _fit(spec, name, how, k) for k in needed}
    finally:
        for k in switches:
            helpers.routes.pop(k)
    work = []
    for n in range(N):
        ni, steps, need = plan[n]
        sp, ds, y, fl, cap, ex = _series(name, n, how)
        o = cl.fit_newton(nc.oracle_spec(sp), ds, y, fl, cap, ex)
        S = o['info'].S
        # the capped run at k = n_iter reproduces the uncapped one bit for bit, later caps change nothing
        for k in needed:
            if k >= ni:
                assert helpers.n_bit_diff(caps[k].theta[n], full.theta[n]) == 0, (name, n, k)
        assert full.fval[n] < 1e99, (name, n)                  # lp finite at the end (no non-finite lp accepted)
        # bit-identical to the twin
        assert (int(full.status[n]), ni, int(full.n_eval[n])) == (o['status'], o['n_iter'], o['n_eval']), (name, n)
        assert helpers.n_bit_diff(_canon(spec, full.theta[n], S), o['theta']) == 0, (name, n)
        assert helpers.n_bit_diff(full.fval[n], o['f']) == 0, (name, n)
        if S == 0:
            continue
        thetas = [_canon(spec, caps[k].theta[n], S) if k in need else None for k in range(1, ni + 1)]
        work.append((name, n, how, thetas, int(full.status[n]), ni, int(full.n_eval[n]), float(full.fval[n]), steps))
    return work


@pytest.mark.parametrize('route', list(ROUTES))
def test_newton_route_against_extended_precision_reference(route):
    from time_series_spark_amd import forecaster as fc
    fc.get_context()
    work = []
    t0 = time.time()
    for name, sw, how in ROUTES[route]:
        w = _run_case(name, sw, how)
        work += w
        print('%-18s %-18s n_iter %s  %.0f s' % (route, name, [it[5] for it in w], time.time() - t0), flush=True)
    with mproc.get_context('spawn').Pool(min(16, os.cpu_count() or 1)) as pool:
        results = list(pool.imap(_judge, work))
    st = dict(judged=0, ill=0, amb=0, err=0.0)
    fails = []
    for name, n, how, rep in results:
        st['judged'] += rep['n_judged']
        st['ill'] += rep['n_ill']
        st['amb'] += rep['n_amb']
        st['err'] = max(st['err'], rep['max_err'])
        if not rep['ok']:
            fails.append((name, n, rep['fails'][:3]))
    print('REPORT %-18s fits %3d  iterations judged %5d  ill-posed %4d  ambiguous %3d  max err/tol %.3g  (%.0f s)'
          % (route, len(results), st['judged'], st['ill'], st['amb'], st['err'], time.time() - t0), flush=True)
    assert not fails, fails
