"""Extended-precision reference for ONE iteration of Stan's Newton optimiser -- TEST INFRASTRUCTURE ONLY.

Stan 2.19's Newton as oracle/prophet_canon.c cn_newton's header recalls it, written in the literal model's
terms (prophet.stan with a dense A = [t >= t_change], see oracle/fbprophet_restated.py), NOT in the kernels'
order of operations:

  * objective: the log-posterior of the literal model, evaluated in long double on the canonical design
    (canon_lib.design: X, t, t_change, scaled y); its gradient is J^T r / sigma^2 plus the priors' terms,
    with J = d mu / d theta taken by the complex step in long double (no cancellation, independent of the
    analytic gradients of fbprophet_restated and of the kernels);
  * Hessian: grad_hess_log_prob -- epsilon 1e-3, perturbations {-2e, -e, +e, +2e} of one coordinate,
    coefficients {1/12, -2/3, 2/3, -1/12}, the recalled half_epsilon = epsilon / 2 factor, H = A + A^T; every
    perturbed point is rounded to float64 before it is evaluated, as Stan does;
  * step: make_negative_definite_and_solve, always by the eigen route (|lambda|): float64 eigh, then cyclic
    Jacobi sweeps in long double on V^T H V until the off-diagonal is at long double rounding, so the
    eigenvectors are long double accurate whatever the conditioning;
  * halving: sizes 1, 1/2, ... while size >= 1e-50, a non-finite trial counts as -1e100;
  * convergence: |lp - lastlp| < 1e-8, the first comparison never fires.

Error scales (multiplied by u = 2^-53 they bound a float64 evaluation in ANY order, up to the calibrated
constant TOL_C, as forecast_ref.M does for the forecast):

  E_g[p]  sum of |terms| of gradient component p: sum_t |J_tp| (|r_t| + |y_t| + M_t) / sigma^2 plus the
          prior's term, with M_t the sum of |terms| of mu_t;
  E_lp    sum of |terms| of the log-posterior, the SSE's scale covering the residual form AND the
          quadratic form s0 + 2 size c.s + size^2 s^T M s of the halving trials (sum_t (|r_t| + |J_t| |D|)^2).

Bounds derived from them:

  E_H            u ||E_A + E_A^T||_F, E_A[d][p] = sum_i |w_i| E_g[p](x_d,i): the float64 error of H;
  step tolerance TOL_C |W| |Lambda|^-1 |W|^T (u E_g + u (E_A + E_A^T) |s|), per component (the componentwise
                 perturbation bound of the solve |H| s = g, W the eigenvectors): an error in H moves the step
                 mostly along the eigenvectors of small |lambda|, and a norm-wise bound would hide mistakes of the
                 size of the float64 noise elsewhere;
  trial margin   TOL_C (u (E_lp(x) + E_lp(theta)) + sum_p |g_p(x)| (size * step tolerance_p + u |x_p|)).

An iteration is ILL-POSED when lambda_min <= TOL_C E_H (some eigenvalue's sign is not determined in float64):
its step is not judged, only its ascent.  A halving decision is AMBIGUOUS when a trial's lp lies within the
margin of lp0.

Layout: theta in the caller's (original column) order [k, m, log sigma, delta[S], beta[K]], S > 0.  A history
without changepoints is fitted on fbprophet's dummy changepoint and returned folded (k + delta): its iterates
cannot be restated from the output, and ``Problem`` refuses it.
"""
import numpy as np

from oracle import canon_lib as cl

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53
TOL_C = 5.0              # calibrated, see tests/test_newton_ref.py::test_tolerance_calibrated_on_cn_newton
EPSILON = 1e-3
PERT = (-2 * EPSILON, -EPSILON, EPSILON, 2 * EPSILON)
COEF = (1.0 / 12.0, -2.0 / 3.0, 2.0 / 3.0, -1.0 / 12.0)
HALF_EPS = 0.5 * EPSILON
CONV = 1e-8
MIN_SIZE = 1e-50
NEWTON_CONVERGED = 60
_H_CS = LD(2) ** -200     # complex step


class Problem(object):
    """The literal model of one series on the canonical design, in long double."""

    def __init__(self, csp, ds, y, floor=0.0, cap=0.0, extra=None):
        d = cl.design(csp, ds, y, floor, cap, extra)
        info = d['info']
        self.S, self.K, self.T = int(info.S), int(info.K), len(ds)
        if self.S == 0:
            raise ValueError('no changepoints: the fit runs on a dummy changepoint that the output folds away')
        self.P = 3 + self.S + self.K
        self.t = d['t'].astype(LD)
        self.tc = d['t_change'].astype(LD)
        self.A = (d['t'][:, None] >= d['t_change'][None, :]).astype(LD)        # [T][S]
        self.cidx = (d['t'][:, None] >= d['t_change'][None, :]).sum(axis=1)    # active changepoints per row
        self.X = d['X'].astype(LD)                                              # [T][K]
        self.y = d['y_scaled'].astype(LD)
        self.logistic = csp.growth == 1
        self.cap = LD(info.cap_scaled)
        self.tau = LD(csp.tau)
        mult, prior = [], []
        for i in range(csp.n_seas):
            mult += [csp.seas_mode[i]] * (2 * csp.seas_order[i])
            prior += [csp.seas_prior[i]] * (2 * csp.seas_order[i])
        for i in range(csp.n_extra):
            mult.append(csp.extra_mode[i])
            prior.append(csp.extra_prior[i])
        self.s_m = np.array(mult, dtype=LD).reshape(self.K)
        self.s_a = 1 - self.s_m
        self.sigmas = np.array(prior, dtype=LD).reshape(self.K)
        self.theta0 = np.zeros(self.P)
        self.theta0[0], self.theta0[1] = d['k0'], d['m0']
        self.ds, self.y_raw, self.floor, self.cap_raw, self.extra = ds, y, floor, cap, extra

    # -- mu = trend (1 + X beta_m) + X beta_a, for a batch of parameter vectors (real or complex) ------------
    def _active(self, v):
        """sum_j A[t][j] v[..., j] for every t (A is a step pattern: a prefix sum picked per row)."""
        c = np.concatenate([np.zeros(v.shape[:-1] + (1,), dtype=v.dtype), np.cumsum(v, axis=-1)], axis=-1)
        return c[..., self.cidx]

    def trend(self, th):
        th = np.atleast_2d(th)
        S = self.S
        k, m = th[:, 0:1], th[:, 1:2]
        dl = th[:, 3:3 + S]
        kt = k + self._active(dl)
        if not self.logistic:
            return kt * self.t + m + self._active(-self.tc * dl)
        ks = np.concatenate([k, k + np.cumsum(dl, axis=1)], axis=1)
        gam = np.zeros_like(dl)
        mpr = m[:, 0]
        for i in range(S):
            gam[:, i] = (self.tc[i] - mpr) * (1 - ks[:, i] / ks[:, i + 1])
            mpr = mpr + gam[:, i]
        z = kt * (self.t - (m + self._active(gam)))
        return self.cap / (1 + np.exp(-z))

    def mu(self, th):
        th = np.atleast_2d(th)
        beta = th[:, 3 + self.S:]
        trend = self.trend(th)
        return trend * (1 + (beta * self.s_m) @ self.X.T) + (beta * self.s_a) @ self.X.T, trend

    def jacobian(self, th):
        """J[p][t] = d mu_t / d theta_p at one long double parameter vector: the trend's columns by the complex
        step (k, m, delta), the beta columns and the (1 + X beta_m) factor in closed form."""
        S, P = self.S, self.P
        beta = th[3 + S:]
        nt = 3 + S
        thc = np.repeat(th[None, :nt].astype(CLD), nt, axis=0)
        thc[np.arange(nt), np.arange(nt)] += 1j * _H_CS
        tr = self.trend(thc)
        trend = tr[0].real
        xm = self.X @ (beta * self.s_m)
        J = np.zeros((P, self.T), dtype=LD)
        J[:nt] = (tr.imag / _H_CS) * (1 + xm)
        J[2] = 0
        J[nt:] = (self.X * self.s_a).T + (self.X * self.s_m).T * trend
        mu = trend * (1 + xm) + self.X @ (beta * self.s_a)
        return J, mu

    def mu_scale(self, th):
        """M_t: the sum of |terms| of mu_t at one parameter vector (long double)."""
        S, K = self.S, self.K
        k, m = th[0], th[1]
        dl, beta = th[3:3 + S], th[3 + S:3 + S + K]
        ka = abs(k) + self.A @ abs(dl)
        if not self.logistic:
            trm = ka * abs(self.t) + abs(m) + self.A @ abs(self.tc * dl)
            trend = (k + self.A @ dl) * self.t + m + self.A @ (-self.tc * dl)
        else:
            ks = np.concatenate([[k], k + np.cumsum(dl)])
            gsc = np.zeros(S, dtype=LD)
            gam = np.zeros(S, dtype=LD)
            mpr = m
            for i in range(S):
                r = ks[i] / ks[i + 1] if ks[i + 1] != 0 else LD(1)
                gam[i] = (self.tc[i] - mpr) * (1 - r)
                gsc[i] = (abs(self.tc[i]) + abs(mpr)) * (1 + abs(r))
                mpr = mpr + gam[i]
            z = (k + self.A @ dl) * (self.t - (m + self.A @ gam))
            sg = 1 / (1 + np.exp(-z))
            Z = ka * (abs(self.t) + abs(m) + self.A @ gsc) + abs(z)
            trend = self.cap * sg
            trm = abs(self.cap) * (sg + sg * (1 - sg) * Z)
        xm = abs(self.X) @ abs(beta * self.s_m)
        return trm * (1 + xm) + abs(trend) * xm + abs(self.X) @ abs(beta * self.s_a)

    # -- log-posterior --------------------------------------------------------------------------------------
    def _priors(self, th):
        S, K = self.S, self.K
        k, m, ls = th[0], th[1], th[2]
        dl, beta = th[3:3 + S], th[3 + S:3 + S + K]
        sig = np.exp(ls)
        terms = [-0.5 * k * k / 25, -0.5 * m * m / 25, -np.sum(abs(dl)) / self.tau, -2 * sig * sig,
                 -0.5 * np.sum((beta / self.sigmas) ** 2), -self.T * ls]
        scale = sum(abs(v) for v in terms)
        return sum(terms), scale, sig

    def lp(self, theta, with_scale=False):
        """lp at float64 theta (long double value); non-finite -> -1e100 (Stan's trial rule)."""
        th = np.asarray(theta, dtype=np.float64).astype(LD)
        with np.errstate(all='ignore'):
            mu = self.mu(th[None, :])[0][0]
            r = self.y - mu
            pr, psc, sig = self._priors(th)
            v = pr - 0.5 * np.sum(r * r) / (sig * sig)
            if not np.isfinite(v):
                return (LD(-1e100), LD(np.inf)) if with_scale else LD(-1e100)
            if not with_scale:
                return v
            M = self.mu_scale(th)
            esse = np.sum(r * r) + 2 * np.sum(abs(r) * (abs(self.y) + M))
            return v, psc + 0.5 * esse / (sig * sig)

    def grad(self, theta):
        """(lp, gradient of lp, E_g, |r|, |J| [P][T]) at one float64 parameter vector, in long double."""
        th = np.asarray(theta, dtype=np.float64).astype(LD)
        S, K = self.S, self.K
        with np.errstate(all='ignore'):
            J, mu = self.jacobian(th)
            r = self.y - mu
            pr, _, sig = self._priors(th)
            s2 = sig * sig
            lp = pr - 0.5 * np.sum(r * r) / s2
            M = self.mu_scale(th)
            g = J @ r / s2
            eg = abs(J) @ (abs(r) + abs(self.y) + M) / s2
            k, m = th[0], th[1]
            dl, beta = th[3:3 + S], th[3 + S:3 + S + K]
            g[0] += -k / 25
            g[1] += -m / 25
            eg[0] += abs(k) / 25
            eg[1] += abs(m) / 25
            sse = np.sum(r * r)
            g[2] = -4 * s2 - self.T + sse / s2
            eg[2] = 4 * s2 + self.T + (sse + 2 * np.sum(abs(r) * (abs(self.y) + M))) / s2
            g[3:3 + S] += -np.sign(dl) / self.tau
            eg[3:3 + S] += 1 / self.tau
            g[3 + S:] += -beta / self.sigmas ** 2
            eg[3 + S:] += abs(beta) / self.sigmas ** 2
        return lp, g, eg, abs(r), abs(J)


def _jacobi_polish(B, sweeps=8):
    """Jacobi sweeps on a nearly diagonal symmetric long double matrix: (eigenvalues, rotation W).  Parallel order
    (round-robin tournament): every round rotates n/2 disjoint index pairs at once."""
    n = B.shape[0]
    B = B.copy()
    W = np.eye(n, dtype=LD)
    m = n + (n & 1)
    rounds = []
    for r in range(m - 1):
        pr = [(m - 1, r)] + [((r + i) % (m - 1), (r - i) % (m - 1)) for i in range(1, m // 2)]
        pr = [(min(a, b), max(a, b)) for a, b in pr if a < n and b < n]
        if pr:
            rounds.append((np.array([a for a, _ in pr]), np.array([b for _, b in pr])))
    tiny = np.finfo(LD).eps * LD(1e-3)
    for _ in range(sweeps):
        off = np.sqrt(np.sum((B - np.diag(np.diag(B))) ** 2))
        if off <= tiny * np.sqrt(np.sum(np.diag(B) ** 2)):
            break
        for p, q in rounds:
            apq = B[p, q]
            nz = apq != 0
            tau = (B[q, q] - B[p, p]) / (2 * np.where(nz, apq, 1))
            t = np.where(tau >= 0, LD(1), LD(-1)) / (abs(tau) + np.sqrt(1 + tau * tau))
            t = np.where(nz, t, 0)
            c = 1 / np.sqrt(1 + t * t)
            s = t * c
            bp, bq = B[:, p].copy(), B[:, q].copy()
            B[:, p], B[:, q] = c * bp - s * bq, s * bp + c * bq
            bp, bq = B[p, :].copy(), B[q, :].copy()
            B[p, :], B[q, :] = c[:, None] * bp - s[:, None] * bq, s[:, None] * bp + c[:, None] * bq
            wp, wq = W[:, p].copy(), W[:, q].copy()
            W[:, p], W[:, q] = c * wp - s * wq, s * wp + c * wq
    return np.diag(B).copy(), W


def eigh_ld(H):
    """Symmetric eigen-decomposition accurate to long double: float64 eigh, then Jacobi polish."""
    lam64, V64 = np.linalg.eigh(np.asarray(H, dtype=np.float64))
    V = V64.astype(LD)
    I = np.eye(V.shape[0], dtype=LD)
    for _ in range(2):                     # orthonormal in long double (Newton-Schulz for the polar factor)
        V = V @ (3 * I - V.T @ V) / 2
    B = V.T @ H @ V
    B = (B + B.T) / 2
    lam, W = _jacobi_polish(B)
    return lam, V @ W


def fd_hessian(prob, theta, pert=PERT, coef=COEF, scale=HALF_EPS, restore=True, symmetrise=True):
    """grad_hess_log_prob: (H, E_A) in long double; keyword arguments give the mutants of the tests."""
    th = np.asarray(theta, dtype=np.float64)
    P = prob.P
    A = np.zeros((P, P), dtype=LD)
    EA = np.zeros((P, P), dtype=LD)
    x = th.copy()
    for d in range(P):
        if restore:
            x = th.copy()
        for i in range(4):
            x[d] = th[d] + pert[i]                     # float64, as Stan forms the perturbed point
            _, g, eg, _, _ = prob.grad(x)
            w = LD(scale * coef[i])
            A[d] += w * g
            EA[d] += abs(w) * eg
    H = A + A.T if symmetrise else 2 * A
    return H, EA


class Iteration(object):
    """The reference for the Newton iteration that starts at float64 theta (the previous iterate)."""

    def __init__(self, prob, theta, c=TOL_C, H=None):
        self.prob, self.c = prob, c
        self.theta = np.asarray(theta, dtype=np.float64).copy()
        self.lp0, g, eg, self.r0, self.J0 = prob.grad(self.theta)
        _, self.E_lp0 = prob.lp(self.theta, with_scale=True)
        self.g_lp, self.E_g = g, eg
        EA = None
        if H is None:
            H, EA = fd_hessian(prob, self.theta)
            self.E_H = U * np.sqrt(np.sum((EA + EA.T) ** 2))
        else:
            self.E_H = LD(0)
        self.H = H
        lam, W = eigh_ld(H)
        self.lam = lam
        self.step = W @ ((W.T @ -g) / abs(lam))
        self.lam_min = np.min(abs(lam))
        self.ill_posed = bool(self.lam_min <= c * self.E_H)
        # componentwise (Skeel-type) bound: |ds| <= | |H|^-1 | (u E_g + E_Hmat |s|), | |H|^-1 | <= |W| |Lambda|^-1 |W|^T
        ehm = U * (EA + EA.T) if EA is not None else np.zeros_like(H)
        self.step_tol = (c * (abs(W) @ ((abs(W).T @ (U * eg + ehm @ abs(self.step))) / abs(lam)))
                         if not self.ill_posed else np.full(prob.P, LD(np.inf)))
        self._trials = {}

    def _quad_scale(self, x):
        """Scale of the quadratic-form SSE around theta at x, over sigma^2: sum_t (|r_t| + |J_t| |x - theta|)^2."""
        D = abs(x.astype(LD) - self.theta.astype(LD))
        return 0.5 * np.sum((self.r0 + D @ self.J0) ** 2) / np.exp(2 * LD(x[2]))

    def trial(self, j):
        """(lp, margin) of trial j, size 2^-j, at the reference step."""
        if j not in self._trials:
            size = LD(2) ** -j
            x = (self.theta.astype(LD) - size * self.step).astype(np.float64)
            lp, elp = self.prob.lp(x, with_scale=True)
            if not np.isfinite(elp):
                self._trials[j] = (lp, LD(0))
            else:
                marg = self.c * U * (elp + self._quad_scale(x) + self.E_lp0)
                if abs(lp - self.lp0) < 1 + marg and not self.ill_posed:
                    _, gx, _, _, _ = self.prob.grad(x)
                    marg += self.c * np.sum(abs(gx) * (size * self.step_tol + U * abs(x)))
                self._trials[j] = (lp, marg)
        return self._trials[j]

    def n_trials_max(self):
        j = 0
        while 2.0 ** -(j + 1) >= MIN_SIZE:
            j += 1
        return j + 1          # sizes 2^0 .. 2^-166 are evaluated

    def judge(self, theta_new):
        """Judges the next iterate: dict(step_err (err / tol, None if not judged), j (trial accepted, -1 = no
        move), admissible, ambiguous, ascent_ok, lp (lp_LD of the new point), margin, n_trials)."""
        new = np.asarray(theta_new, dtype=np.float64)
        D = new.astype(LD) - self.theta.astype(LD)
        lp_new, e_new = self.prob.lp(new, with_scale=True)
        with np.errstate(all='ignore'):
            marg_new = self.c * U * (e_new + self._quad_scale(new) + self.E_lp0)
        out = dict(lp=lp_new, margin=marg_new, ill_posed=self.ill_posed, ascent_ok=bool(lp_new >= self.lp0 - marg_new),
                   step_err=None, j=None, admissible=True, ambiguous=False, n_trials=None)
        if not np.any(D):
            nt = self.n_trials_max()
            out['j'], out['n_trials'] = -1, nt
            if not self.ill_posed:
                for i in range(nt):
                    lp, m = self.trial(i)
                    if lp >= self.lp0 + m:
                        out['admissible'] = False
                    if abs(lp - self.lp0) <= m:
                        out['ambiguous'] = True
            return out
        if self.ill_posed:
            return out
        ss = np.sum(self.step * self.step)
        alpha = -np.sum(D * self.step) / ss
        if not alpha > 0:
            out['step_err'] = np.inf
            return out
        j = int(np.rint(-np.log2(float(alpha))))
        j = max(j, 0)
        size = LD(2) ** -j
        tol = size * self.step_tol + 2 * U * abs(new)
        out['step_err'] = float(np.max(abs(D + size * self.step) / tol))
        out['j'], out['n_trials'] = j, j + 1
        for i in range(j + 1):
            lp, m = self.trial(i)
            if abs(lp - self.lp0) <= m:
                out['ambiguous'] = True
            if i < j and lp >= self.lp0 + m:
                out['admissible'] = False
            if i == j and lp < self.lp0 - m:
                out['admissible'] = False
        return out


def judge_fit(prob, thetas, status, n_iter, n_eval, fval, c=TOL_C, judge_steps=None):
    """Judges a fit from its iterates thetas[0 .. n_iter] (thetas[0] = the init; None where not on record).  judge_steps: the iterations
    (1-based) whose step, halving and ascent are judged (default: all of them); the convergence test and fval
    are judged on every iterate, n_eval only when every step was judged and no halving decision was ambiguous.
    Returns (report dict, per-iteration judgements)."""
    rep = dict(ok=True, fails=[])

    def fail(msg):
        rep['ok'] = False
        rep['fails'].append(msg)

    ks = list(range(1, n_iter + 1)) if judge_steps is None else list(judge_steps)
    its = []
    for k in ks:
        jd = Iteration(prob, thetas[k - 1], c=c).judge(thetas[k])
        jd['k'] = k
        its.append(jd)
        if not jd['ascent_ok']:
            fail('iteration %d: lp fell below the margin (%.3g)' % (k, float(jd['margin'])))
        if jd['step_err'] is not None and not jd['step_err'] <= 1:
            fail('iteration %d: step off the reference line, err/tol %.3g (j = %s)' % (k, jd['step_err'], jd['j']))
        if not jd['admissible']:
            fail('iteration %d: trial %s could not have been the accepted one' % (k, jd['j']))
    # status / n_iter: Stan's convergence test on lp_LD of consecutive iterates (the first comparison never fires);
    # iterates not on record (None) leave their comparisons out
    lp_all = [None if th is None else prob.lp(th, with_scale=True) for th in thetas[:n_iter + 1]]
    rep['ambiguous_conv'] = False
    for k in range(2, n_iter + 1):
        if lp_all[k] is None or lp_all[k - 1] is None:
            continue
        d = abs(lp_all[k][0] - lp_all[k - 1][0])
        if abs(d - CONV) <= c * U * (lp_all[k][1] + lp_all[k - 1][1]):
            rep['ambiguous_conv'] = True
            continue
        if k < n_iter and d < CONV:
            fail('iteration %d: |dlp| = %.3g < 1e-8 but the fit went on' % (k, float(d)))
        if k == n_iter and status == NEWTON_CONVERGED and d >= CONV:
            fail('iteration %d: converged with |dlp| = %.3g' % (k, float(d)))
    if status == NEWTON_CONVERGED and n_iter < 2:
        fail('converged before the second comparison')
    lpf, ef = lp_all[n_iter]
    if not abs(-LD(fval) - lpf) <= 2 * c * U * ef:
        fail('fval %.17g is not -lp_LD(theta_final) = %.17g' % (fval, float(-lpf)))
    if ks == list(range(1, n_iter + 1)) and not any(jd['ambiguous'] or jd['n_trials'] is None for jd in its):
        ne = 1 + sum(1 + 4 * prob.P + jd['n_trials'] for jd in its)
        if ne != n_eval:
            fail('n_eval %d, reference %d' % (n_eval, ne))
    rep['n_judged'] = len(its)
    rep['n_ill'] = sum(jd['ill_posed'] for jd in its)
    rep['n_amb'] = sum(jd['ambiguous'] for jd in its)
    errs = [jd['step_err'] for jd in its if jd['step_err'] is not None]
    rep['max_err'] = max(errs) if errs else 0.0
    return rep, its
