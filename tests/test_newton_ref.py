"""CPU tests of the extended-precision Newton reference (oracle/newton_ref.py): the reference against mpmath, its
tolerance constant measured on oracle cn_newton (bit-identical to the Newton kernels by contract) over the case
matrix of tests/newton_cases.py, and proof that the judge accepts correct Newton runs and rejects each of the
mistakes it is there to catch."""
import multiprocessing as mproc
import os

import mpmath
import numpy as np
import pytest

from oracle import canon_lib as cl, newton_ref as nr
from tests import helpers, newton_cases as nc

LD_EPS = float(np.finfo(np.longdouble).eps)


def _mpf(x):
    """Exact long double -> mpf (hi + lo float64 parts)."""
    x = np.longdouble(x)
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))


# ---------------------------------------------------------------------------------------------
# the reference against mpmath
# ---------------------------------------------------------------------------------------------

def _mp_lp(prob, th):
    """lp of the literal model at 50 digits, scalar loops over rows (fbprophet's piecewise_linear /
    piecewise_logistic, prophet.stan's model block)."""
    mp = mpmath.mp
    S, K = prob.S, prob.K
    k, m, ls = th[0], th[1], th[2]
    dl, beta = th[3:3 + S], th[3 + S:3 + S + K]
    tc = [_mpf(v) for v in prob.tc]
    sse = mp.mpf(0)
    if prob.logistic:
        ks = [k]
        for d in dl:
            ks.append(ks[-1] + d)
        gam, mpr = [], m
        for i in range(S):
            gam.append((tc[i] - mpr) * (1 - ks[i] / ks[i + 1]))
            mpr = mpr + gam[-1]
    for t_i in range(prob.T):
        t = _mpf(prob.t[t_i])
        kt, mt = k, m
        for i in range(S):
            if t >= tc[i]:
                kt += dl[i]
                mt += gam[i] if prob.logistic else -tc[i] * dl[i]
        trend = _mpf(prob.cap) / (1 + mp.exp(-kt * (t - mt))) if prob.logistic else kt * t + mt
        xm = xa = mp.mpf(0)
        for j in range(K):
            v = _mpf(prob.X[t_i, j]) * beta[j]
            if prob.s_m[j]:
                xm += v
            else:
                xa += v
        r = _mpf(prob.y[t_i]) - (trend * (1 + xm) + xa)
        sse += r * r
    sig = mp.exp(ls)
    lp = -k * k / 50 - m * m / 50 - sum(abs(d) for d in dl) / _mpf(prob.tau) - 2 * sig * sig
    lp += -sum((beta[j] / _mpf(prob.sigmas[j])) ** 2 for j in range(K)) / 2 - prob.T * ls - sse / (2 * sig * sig)
    return lp


def test_gradient_against_mpmath():
    """lp and its gradient (long double, complex-step J) against mpmath at 50 digits by high-precision numerical
    differentiation, on linear / logistic, additive / multiplicative iterates of real fits: within 64 long double
    units of the error scales the reference reports (E_g; the lp's own scale)."""
    worst = 0.0
    with mpmath.workdps(50):
        for name, k in (('T10', 4), ('ref_logistic_mult', 6), ('mixed', 3)):
            prob, _, ths = nc.oracle_fits(name, 0, max_iter=k)
            th64 = ths[k]
            lp, g, eg, _, _ = prob.grad(th64)
            _, elp = prob.lp(th64, with_scale=True)
            thm = [mpmath.mpf(float(v)) for v in th64]
            lpm = _mp_lp(prob, thm)
            assert abs(_mpf(lp) - lpm) <= 64 * LD_EPS * _mpf(elp)
            for p in range(prob.P):
                gm = mpmath.diff(lambda v: _mp_lp(prob, thm[:p] + [v] + thm[p + 1:]), thm[p])
                err = abs(_mpf(g[p]) - gm) / _mpf(eg[p])
                worst = max(worst, float(err / LD_EPS))
                assert err <= 64 * LD_EPS, (name, p, float(err))
    print('gradient vs mpmath: worst %.2f long double units of E_g' % worst)


def _mp_step(H, g):
    n = H.shape[0]
    Hm = mpmath.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Hm[i, j] = _mpf(H[i, j])
    lam, V = mpmath.eigsy(Hm)
    gm = mpmath.matrix([_mpf(v) for v in g])
    proj = V.T * gm
    for j in range(n):
        proj[j] = proj[j] / abs(lam[j])
    return V * proj, [lam[j] for j in range(n)]


def test_step_against_mpmath():
    """make_negative_definite_and_solve (long double eigen route) against mpmath.eigsy at 50 digits on
    finite-difference Hessians of real iterations: an indefinite one, a negative definite one and ones with a
    near-zero eigenvalue (duplicate regressors under priors of scale 1e3 and 1e5: condition ~1e10 and ~1e14).
    Eigenvalues within 64 long double units of ||H||, the step within 64 units times cond(H)."""
    cases = []
    prob, _, ths = nc.oracle_fits('T10', 0, max_iter=12)
    its = [nr.Iteration(prob, ths[k]) for k in range(12)]
    kinds = {'indefinite': [i for i in its if (i.lam > 0).any() and (i.lam < 0).any()],
             'negative definite': [i for i in its if (i.lam < 0).all()]}
    for kind, lst in kinds.items():
        assert lst, kind
        cases.append((kind, lst[0]))
    for name in ('dup3', 'dup5'):
        prob, _, ths = nc.oracle_fits(name, 0, max_iter=3)
        cases.append((name, nr.Iteration(prob, ths[3])))
    with mpmath.workdps(50):
        for kind, it in cases:
            sm, lm = _mp_step(it.H, -it.g_lp)
            hn = float(np.max(np.abs(it.lam)))
            cond = hn / float(it.lam_min)
            lam_ref = np.sort(np.array([float(v) for v in lm]))
            assert np.abs(np.sort(it.lam.astype(np.float64)) - lam_ref).max() <= 64 * LD_EPS * hn + 1e-300, kind
            err = max(abs(_mpf(it.step[i]) - sm[i]) for i in range(len(sm)))
            nrm = max(abs(v) for v in sm)
            rel = float(err / nrm)
            print('%-18s cond %.1e  step rel err %.1e (bound %.1e)' % (kind, cond, rel, 64 * LD_EPS * cond))
            assert rel <= 64 * LD_EPS * cond, kind
            if kind.startswith('dup'):
                assert cond > 1e9


# ---------------------------------------------------------------------------------------------
# calibration on cn_newton
# ---------------------------------------------------------------------------------------------

def _pool():
    n = min(16, os.cpu_count() or 1)
    return mproc.get_context('spawn').Pool(n) if n > 1 else None


def _map(fn, args):
    pool = _pool()
    if pool is None:
        return [fn(a) for a in args]
    try:
        return pool.map(fn, args)
    finally:
        pool.close()
        pool.join()


def _calib_one(arg):
    name, n, sample = arg
    plan = {}

    def pick(ni):
        if not sample and ni <= 300:
            return None
        rng = np.random.default_rng(n + 7)
        steps = sorted(set([1, 2, ni] + [int(v) for v in rng.choice(np.arange(1, ni + 1), min(sample or 40, ni),
                                                                   replace=False)]))
        plan['steps'] = steps
        return set(steps) | set(k - 1 for k in steps)

    prob, full, ths = nc.oracle_fits(name, n, ks=pick)
    rep, _ = nr.judge_fit(prob, ths, full['status'], full['n_iter'], full['n_eval'], full['f'],
                          judge_steps=plan.get('steps'))
    return name, n, rep


def test_tolerance_calibrated_on_cn_newton():
    """TOL_C measured on cn_newton trajectories (max_iter = k for every k): every iteration of the conditioning
    cases and of two short fits, a seeded sample of twelve iterations of series 0 of every other case (and of
    fits longer than 300 iterations).  The componentwise step tolerance is a first-order bound, and the twin
    comes close to it.  Measured err/tol at TOL_C = 5: at most 0.45 here (2.25 with the constant taken as 1, an
    upper bound), at most 0.48 over the GPU matrix of tests/test_gpu_newton.py.  The margin to the mutants is thin:
    'no_sym' of test_judge_rejects_each_mutant is caught at 1.02 times the tolerance.  Not covered: the reference's
    logistic / multiplicative model on an 18-row history under the 90-row cap reaches err/tol 12 at TOL_C = 5 on
    iterations 51 - 61 of 249 (the first-order bound does not hold there), so no such history is in the matrix.
    At TOL_C every iteration of the matrix is accepted
    (step on the reference line at an admissible 2^-j, ascent), and status, n_iter, fval and -- where no halving
    decision is ambiguous -- n_eval follow the reference."""
    full_cases = nc.CONDITIONING + ['T3', 'T10', 'K0']          # (T3: a sample, its fits take thousands of iterations)
    args = [(name, 0, None) for name in full_cases]
    args += [(name, 0, 12) for name in nc.SHAPES if name not in full_cases]
    worst, report = 0.0, []
    for name, n, rep in _map(_calib_one, args):
        e1 = rep['max_err'] * nr.TOL_C
        report.append('%-18s judged %3d  ill-posed %3d  ambiguous %2d  max err/tol(c=1) %.3g'
                      % (name, rep['n_judged'], rep['n_ill'], rep['n_amb'], e1))
        worst = max(worst, e1)
        assert rep['ok'], (name, rep['fails'])
    print('\n'.join(report))
    print('largest err/tol at c = 1: %.3g; TOL_C = %g' % (worst, nr.TOL_C))
    assert worst * 2 < nr.TOL_C


# ---------------------------------------------------------------------------------------------
# the judge against a plain float64 restatement and its mutants
# ---------------------------------------------------------------------------------------------

def restate(name, n=0, mutant=None, max_iter=400):
    """Stan's Newton in plain float64 numpy on the oracle's residual-form objective (cn_eval_at), numpy eigh for
    the eigen route; ``mutant`` plants one mistake.  Returns (Problem, iterates, status, n_iter, n_eval, f)."""
    spec, ds, y, fl, cap, ex = nc.make(name)
    csp = nc.oracle_spec(spec)
    prob = nr.Problem(csp, ds, y[n], fl[n], cap[n], ex)
    P = prob.P
    n_eval = [0]

    def lp_grad(x):
        n_eval[0] += 1
        f, g, rc = cl.eval_at(csp, ds, y[n], x, fl[n], cap[n], ex)
        if rc or not np.isfinite(f) or not np.isfinite(g).all():
            return -1e100, None
        return -f, -g

    eps = 1e-3
    pert = [-2 * eps, -eps, eps, 2 * eps]
    coef = [1 / 12, -2 / 3, 2 / 3, -1 / 12]
    if mutant == 'coef_sign':
        coef[3] = 1 / 12
    scale = 1 / eps if mutant == 'inv_eps' else 0.5 * eps
    conv = 1e-7 if mutant == 'conv_1e-7' else 1e-8
    th = prob.theta0.copy()
    ths = [th.copy()]
    lp, _ = lp_grad(th)
    status, it = 40, 0
    for mI in range(max_iter):
        last = lp
        f0, g = lp_grad(th)
        A = np.zeros((P, P))
        x = th.copy()
        for d in range(P):
            if mutant != 'no_restore':
                x = th.copy()
            for i in range(4):
                x[d] = th[d] + pert[i]
                A[d] += scale * coef[i] * lp_grad(x)[1]
        H = 2 * A if mutant == 'no_sym' else A + A.T
        if mutant == 'chol_abs':
            L = np.zeros((P, P))
            Hn = -H
            for j in range(P):
                s = Hn[j:, j] - L[j:, :j] @ L[j, :j]
                L[j, j] = np.sqrt(abs(s[0]))
                L[j + 1:, j] = s[1:] / L[j, j]
            z = np.linalg.solve(L, -g)
            step = np.linalg.solve(L.T, z)
        else:
            w, V = np.linalg.eigh(H)
            den = -w if mutant == 'signed' else np.abs(w)
            step = V @ ((V.T @ -g) / den)
        size, f1, new = 2.0, -1e100, th
        while f1 < f0:
            size *= 0.5
            if size < 1e-50:
                break
            new = th - size * step
            f1, _ = lp_grad(new)
        if size >= 1e-50:
            th, lp = new, f1
        else:
            lp = f0
        it += 1
        ths.append(th.copy())
        if mI > 0 and abs(lp - last) < conv:
            status = 60
            break
    return prob, ths, status, it, n_eval[0], -lp


def _judge_restated(arg):
    name, mutant, n_steps = arg
    prob, ths, st, it, ne, f = restate(name, 0, mutant, max_iter=400 if mutant in (None, 'conv_1e-7') else n_steps)
    steps = None if n_steps is None else range(1, min(it, n_steps) + 1)
    rep, _ = nr.judge_fit(prob, ths, st, it, ne, f, judge_steps=steps)
    return name, mutant, rep


def test_judge_accepts_plain_float64_restatement():
    """A correct Newton that shares no arithmetic with the kernels (numpy eigh, residual-form objective, numpy's
    summation order) passes every check of the judge, fit-level ones included."""
    for name, mutant, rep in _map(_judge_restated, [('T31', None, None), ('ref_logistic_mult', None, 20),
                                                    ('holidays', None, 20)]):
        assert rep['ok'], (name, rep['fails'])


MUTANTS = ['signed', 'inv_eps', 'coef_sign', 'no_sym', 'no_restore', 'conv_1e-7', 'chol_abs']


def test_judge_rejects_each_mutant():
    """Each planted mistake is rejected on at least one case: signed lambda instead of |lambda|, the other
    spelling 1/epsilon of the FD scale, one FD coefficient of the wrong sign, no symmetrisation (H = 2A), a
    perturbed coordinate that is not restored, a convergence threshold of 1e-7, and a Cholesky with sqrt(|s_j|)
    and no pivot check."""
    cases = ['T31', 'ref_logistic_mult', 'mixed', 'steep_logistic']
    args = [(c, m, None if m == 'conv_1e-7' else (40 if c == 'steep_logistic' else 6)) for m in MUTANTS for c in cases]
    caught = {m: [] for m in MUTANTS}
    for name, mutant, rep in _map(_judge_restated, args):
        if not rep['ok']:
            caught[mutant].append((name, rep['fails'][0]))
    for m in MUTANTS:
        print('%-10s rejected on %s' % (m, [c for c, _ in caught[m]]), caught[m][0][1] if caught[m] else '')
    assert all(caught[m] for m in MUTANTS), {m: v for m, v in caught.items() if not v}


def test_quadratic_form_trials_when_the_model_interpolates():
    """Below ~10 rows a weekly model has more parameters than rows: it interpolates and sigma goes to 0.  A halving
    trial's quadratic-form SSE, s0 + 2 size c.s + size^2 s^T M s, then keeps an absolute error of about u (|X| |D|)^2
    while -SSE / (2 sigma^2) divides it by sigma^2 < 1e-18: before the guard a trial whose lp is -1e188 came out as
    +1e189, was accepted, and the fit ended 'converged' at fval = 1e100 with log sigma = -234 (T = 3 .. 9).  Trials
    whose three terms cancel to less than 2^-20 of their sum are now evaluated in residual form (cn_newton and the
    kernels, CN_NEWTON_QGUARD): every fit ends at a finite lp with a finite sigma, and the judge accepts them."""
    from time_series_spark_amd import synth
    for T in (2, 3, 4, 5, 8, 9):
        ds, y = synth.make_panel(3, T, 'linear', seed=751 + T)
        csp = nc.oracle_spec(nc._spec())
        assert csp.eval_mode == 1
        for n in range(3):
            r = cl.fit_newton(csp, ds, y[n])
            assert r['status_name'] == 'NEWTON_CONVERGED' and r['f'] < 1e99 and abs(r['theta'][2]) < 60, (T, n, r['f'])
    for n in range(3):
        name, _, rep = _calib_one(('T3', n, 12))
        assert rep['ok'], (n, rep['fails'])
