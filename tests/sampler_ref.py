"""Reference for the predictive sampler (interval_sample_kernel, oracle cn_predict_intervals): what its draws must
be distributed as, written from fbprophet's definition (sample_predictive_trend, sample_model) and not from the kernel.

Four parts:
  1. the analytic laws of the linear-growth sampler (Laws);
  2. an independent vectorised sampler on numpy.random.Generator (independent_draws), for what has no closed form
     (logistic growth) -- poisson, uniform + sort, laplace, normal, none of the kernel's devices;
  3. a vectorised restatement of the device's stream scheme (restated_draws: key schedule, u01, Poisson in pieces of
     8, the order-statistic recurrence, Laplace by inversion, Box-Muller) with switches for mutants of it, so the CPU
     suite runs the battery at the full sample count and shows that it rejects a subtly wrong scheme;
  4. the battery: draws -> [(name, kind, value)], kind 'z' (a z-score, standard normal under the laws) or 'p' (a
     p-value, uniform or stochastically larger under the laws).  failures() applies the thresholds.

Scaled time t, Tm the largest row, S_cp = max(S, 1), lam = mean|delta| + 1e-8, the rate S_cp (Tm - 1) for Tm > 1.
New changepoints form a Poisson process of intensity S_cp on (1, Tm] with iid Laplace(lam) slope changes, so with
D(t) the drawn trend minus the deterministic one (in units of y_scale), D(t) = sum_j delta_j (t - tau_j)+ is compound
Poisson with cumulants
    kappa_2k(t) = S_cp E[delta^2k] int_1^t (t - tau)^2k dtau = S_cp (2k)! lam^2k (t - 1)^(2k+1) / (2k + 1),
i.e. variance 2 lam^2 S_cp (t-1)^3 / 3, fourth cumulant 24 lam^4 S_cp (t-1)^5 / 5, and for a < b
    cov(D(a), D(b)) = 2 lam^2 S_cp [(a-1)^3 / 3 + (b - a)(a-1)^2 / 2].

Thresholds (derived, not measured): |z| <= Z_MAX = 5.5 (two-sided normal tail 3.8e-8: below 1e-4 family-wise for up to
2 600 statistics) and p >= P_MIN = 1e-7.  A count is compared by the normal approximation only where its expected
number of events and of non-events is >= 1 000, otherwise by the exact binomial law (a p-value); chi-square cells are
merged until each expects >= 10."""
import math

import numpy as np
from scipy import stats

Z_MAX = 5.5
P_MIN = 1e-7
NORMAL_MIN_EVENTS = 1000.0
CHI2_MIN_EXPECTED = 10.0

# Kink detection on an equally spaced block of rows (spacing dt).  With L(t) the path in the coordinate in which it is
# piecewise linear, the second difference L(t_i+1) - 2 L(t_i) + L(t_i-1) is sum_j delta_j (dt - |tau_j - t_i|)+ over the
# kinks of the window (t_i-1, t_i+1).  A window counts as occupied where |second difference| > KINK_X0 lam dt.  A window
# with one kink is missed where |delta| w < KINK_X0 lam dt with |delta| ~ Exp(lam) and w = dt - |tau - t_i| ~ U(0, dt):
#     P(miss) = int_0^1 (1 - exp(-x0 / u)) du = x0 (1 - gamma - ln x0) + O(x0^2) = 7.9e-8 < 1e-7 at x0 = 4e-9
# (kink_miss_probability evaluates the integral; the test module asserts the bound).  Rounding cannot fake a kink: the
# battery refuses a case whose threshold is not 64 roundings of the path's largest value above zero.
KINK_X0 = 4e-9
# An isolated occupied window holds n >= 1 kinks with the truncated-Poisson weights of mu = 2 S_cp dt.  The slope change
# across it is Laplace(lam) for n = 1 and the two-fold sum for n = 2; n >= 3 is neglected.  Its mass
# P(n >= 3 | n >= 1) = mu^2 / 6 + O(mu^3) must stay below 1e-4: mu <= WINDOW_MU_MAX.
WINDOW_MU_MAX = 0.024
NEGLECTED_MAX = 1e-4

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_C1 = np.uint64(0xBF58476D1CE4E5B9)
_C2 = np.uint64(0x94D049BB133111EB)
_U = np.uint64


# ---- 1. laws ---------------------------------------------------------------------------------------------------

def kink_miss_probability(x0=KINK_X0):
    from scipy import integrate
    val, _ = integrate.quad(lambda u: -np.expm1(-x0 / u), 0.0, 1.0, limit=200, epsabs=0.0, epsrel=1e-9,
                            points=[1e-12, 1e-9, 1e-6, 1e-3])
    return val


def neglected_mass(mu):
    """P(n >= 3 | n >= 1) of a Poisson(mu) count"""
    p0, p1, p2 = math.exp(-mu), mu * math.exp(-mu), mu * mu / 2.0 * math.exp(-mu)
    return (1.0 - p0 - p1 - p2) / (1.0 - p0)


class Laws(object):
    """the laws of one linear-growth model on rows t"""

    def __init__(self, S_cp, lam, Tm):
        self.S_cp, self.lam, self.Tm = float(S_cp), float(lam), float(Tm)
        self.rate = self.S_cp * (self.Tm - 1.0) if self.Tm > 1.0 else 0.0

    def _x(self, t):
        """the time a row has been exposed to new changepoints (none where the rate is 0)"""
        return np.maximum(np.asarray(t, dtype=np.float64) - 1.0, 0.0) if self.rate > 0.0 else 0.0 * np.asarray(t, float)

    def cumulant(self, order, t):
        """kappa_order of D(t), order even"""
        x = self._x(t)
        return self.S_cp * math.factorial(order) * self.lam ** order * x ** (order + 1) / (order + 1)

    def var(self, t):
        return self.cumulant(2, t)

    def cov(self, a, b):
        xa = self._x(a)
        return 2.0 * self.lam ** 2 * self.S_cp * (xa ** 3 / 3.0 + (np.asarray(b) - np.asarray(a)) * xa ** 2 / 2.0)

    def moment4(self, t):
        return self.cumulant(4, t) + 3.0 * self.var(t) ** 2

    def moment8(self, t):
        k2, k4, k6, k8 = (self.cumulant(o, t) for o in (2, 4, 6, 8))
        return k8 + 28.0 * k6 * k2 + 35.0 * k4 ** 2 + 210.0 * k4 * k2 ** 2 + 105.0 * k2 ** 4

    def var_of_product(self, a, b):
        """Var(D(a) D(b)), a <= b: D(b) = D(a) + (b - a) K(a) + E with K(a) the slope change drawn by a and E the
        later kinks' part, independent of the past.  By the joint cumulants of (D(a), K(a)),
        kappa(D^p K^q) = S_cp E[delta^(p+q)] x^(p+1) / (p + 1) with x = a - 1."""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        x, g, lam, S = self._x(a), b - a, self.lam, self.S_cp

        def kap(p, q):
            return S * math.factorial(p + q) * lam ** (p + q) * x ** (p + 1) / (p + 1)
        # E[D^4], E[D^3 K], E[D^2 K^2] of zero-mean variables from joint cumulants (order 4 + the pairings of order 2)
        d4 = kap(4, 0) + 3.0 * kap(2, 0) ** 2
        d3k = kap(3, 1) + 3.0 * kap(2, 0) * kap(1, 1)
        d2k2 = kap(2, 2) + kap(2, 0) * kap(0, 2) + 2.0 * kap(1, 1) ** 2
        var_e = self.var(b) - (kap(2, 0) + 2.0 * g * kap(1, 1) + g * g * kap(0, 2))
        second = d4 + 2.0 * g * d3k + g * g * d2k2 + kap(2, 0) * var_e
        return second - self.cov(a, b) ** 2


def laplace_cdf(x, lam):
    x = np.asarray(x, dtype=np.float64) / lam
    return np.where(x < 0, 0.5 * np.exp(np.minimum(x, 0.0)), 1.0 - 0.5 * np.exp(-np.maximum(x, 0.0)))


def laplace2_cdf(x, lam):
    """the sum of two independent Laplace(lam): density (1 + |x| / lam) exp(-|x| / lam) / (4 lam)"""
    a = np.abs(np.asarray(x, dtype=np.float64)) / lam
    tail = 0.25 * np.exp(-a) * (2.0 + a)
    return np.where(np.asarray(x) < 0, tail, 1.0 - tail)


def window_mixture(mu):
    """weights of one and of two kinks among the occupied windows, renormalised over {1, 2}"""
    w1, w2 = mu, mu * mu / 2.0
    return w1 / (w1 + w2), w2 / (w1 + w2)


# ---- the model of a case, evaluated in plain numpy ---------------------------------------------------------------

class Model(object):
    """One series' constants as the sampler sees them: growth, k, m (after the fitted changepoints, which all lie
    before the future rows), S_cp, lam, sigma, y_scale, floor, cap, rows t [H], xa [H] (additive term times y_scale),
    opm [H] (1 + multiplicative term)."""

    def __init__(self, growth, k, m, S_cp, lam, sigma, y_scale, t, xa=None, opm=None, floor=0.0, cap=0.0):
        self.growth, self.k, self.m = growth, float(k), float(m)
        self.S_cp, self.lam, self.sigma = int(S_cp), float(lam), float(sigma)
        self.y_scale, self.floor, self.cap = float(y_scale), float(floor), float(cap)
        self.t = np.asarray(t, dtype=np.float64)
        H = len(self.t)
        self.xa = np.zeros(H) if xa is None else np.asarray(xa, dtype=np.float64)
        self.opm = np.ones(H) if opm is None else np.asarray(opm, dtype=np.float64)
        self.Tm = float(self.t.max())
        self.rate = self.S_cp * (self.Tm - 1.0) if self.Tm > 1.0 else 0.0

    @property
    def fl(self):
        return self.floor if self.growth == 'logistic' else 0.0

    @property
    def cap_sc(self):
        return (self.cap - self.fl) / self.y_scale

    def trend_of(self, k, m, t):
        """the trend in y units at state (k, m)"""
        g = k * t + m if self.growth == 'linear' else self.cap_sc / (1.0 + np.exp(-(k * (t - m))))
        return g * self.y_scale + self.fl

    def det_trend(self):
        return self.trend_of(self.k, self.m, self.t)

    def laws(self):
        return Laws(self.S_cp, self.lam, self.Tm)


def piecewise_paths(model, tau, delta, n):
    """trend [P][H] of P paths with n [P] new changepoints at sorted times tau [P][J] (beyond n: ignored) and slope
    changes delta [P][J]: fbprophet's piecewise_linear / piecewise_logistic with the new changepoints appended (linear:
    m_j = m_(j-1) - tau_j delta_j; logistic: m_j = m_(j-1) + (tau_j - m_(j-1)) (1 - k_(j-1) / k_j))"""
    P, J = tau.shape
    valid = np.arange(J)[None, :] < n[:, None]
    d = np.where(valid, delta, 0.0)
    tq = np.where(valid, tau, np.inf)
    tau = np.where(valid, tau, 0.0)
    ks = np.empty((P, J + 1))
    ms = np.empty((P, J + 1))
    ks[:, 0], ms[:, 0] = model.k, model.m
    for j in range(J):
        kn = ks[:, j] + d[:, j]
        if model.growth == 'linear':
            ms[:, j + 1] = ms[:, j] + np.where(valid[:, j], -tau[:, j] * d[:, j], 0.0)
        else:
            ms[:, j + 1] = ms[:, j] + np.where(valid[:, j], (tau[:, j] - ms[:, j]) * (1.0 - ks[:, j] / kn), 0.0)
        ks[:, j + 1] = kn
    out = np.empty((P, len(model.t)))
    rows = np.arange(P)
    for h, th in enumerate(model.t):
        c = (tq <= th).sum(axis=1)
        out[:, h] = model.trend_of(ks[rows, c], ms[rows, c], th)
    return out


# ---- 2. the independent sampler --------------------------------------------------------------------------------

def independent_draws(model, N, S, seed, chunk=8):
    """{'yhat', 'trend'} [N][H][S] from numpy's generator: fbprophet's sample_predictive_trend and sample_model"""
    rng = np.random.default_rng(seed)
    H = len(model.t)
    trend = np.empty((N, H, S))
    for n0 in range(0, N, chunk):
        nc = min(chunk, N - n0)
        P = nc * S
        cnt = rng.poisson(model.rate, P) if model.rate > 0.0 else np.zeros(P, dtype=np.int64)
        J = max(int(cnt.max()), 1)
        tau = rng.uniform(1.0, model.Tm, (P, J)) if model.Tm > 1.0 else np.ones((P, J))
        tau = np.sort(np.where(np.arange(J)[None, :] < cnt[:, None], tau, np.inf), axis=1)
        delta = rng.laplace(0.0, model.lam, (P, J))
        tr = piecewise_paths(model, tau, delta, cnt)
        trend[n0:n0 + nc] = tr.reshape(nc, S, H).transpose(0, 2, 1)
    noise = rng.normal(0.0, model.sigma, (N, H, S))
    yhat = trend * model.opm[None, :, None] + model.xa[None, :, None] + noise * model.y_scale
    return {'yhat': yhat, 'trend': trend}


# ---- 3. the device's stream scheme, restated -------------------------------------------------------------------

def mix64(z):
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)) + _GOLD
    z = (z ^ (z >> _U(30))) * _C1
    z = (z ^ (z >> _U(27))) * _C2
    return z ^ (z >> _U(31))


def stream_key(seed, series_key, sample, stream):
    as_u = lambda a: np.atleast_1d(np.asarray(a)).astype(np.int64).view(np.uint64) if np.asarray(a).dtype.kind == 'i' \
        else np.atleast_1d(np.asarray(a, dtype=np.uint64))  # noqa: E731
    return mix64(mix64(mix64(mix64(as_u(seed)) ^ as_u(series_key)) ^ as_u(sample)) ^ as_u(stream))


def u01_from_bits(x):
    """the generator's map from 64 bits to a double: ((x >> 11) + 0.5) 2^-53.  Not in (0, 1): above 2^52 the sum with
    0.5 is not representable and ties go to even, so the top value 2^53 - 1 gives 2^53 and the result is exactly 1.0
    (probability 2^-53).  The smallest result is 2^-54."""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    return ((x >> _U(11)).astype(np.float64) + 0.5) * 1.1102230246251565e-16


def u01(key, ctr):
    return u01_from_bits(mix64(key + _GOLD * np.asarray(ctr, dtype=np.uint64)))


MUTANTS = ('laplace_scale', 'drop_remainder', 'no_composition', 'noise_scale', 'u2_from_u1', 'shared_noise',
           'no_sample_in_key')


def _poisson_pieces(lam, key, drop_remainder):
    """Knuth's product method on pieces of at most 8 -> (n, counters consumed)"""
    P = len(key)
    n = np.zeros(P, dtype=np.int64)
    ctr = np.zeros(P, dtype=np.uint64)
    rest = lam
    while rest > 0.0:
        piece = rest if rest < 8.0 else 8.0
        if drop_remainder and piece < 8.0:
            break
        L = math.exp(-piece)
        p = np.ones(P)
        k = np.zeros(P, dtype=np.int64)
        act = np.arange(P)
        while len(act):
            p[act] = p[act] * u01(key[act], ctr[act])
            ctr[act] += _U(1)
            k[act] += 1
            act = act[p[act] > L]
        n += k - 1
        rest = rest - piece
    return n, ctr


def restated_kinks(model, kcp, mutant=None):
    """(n [P], tau [P][J], delta [P][J]) of the changepoint stream keys kcp [P]"""
    P = len(kcp)
    if not model.rate > 0.0:
        return np.zeros(P, dtype=np.int64), np.full((P, 1), np.inf), np.zeros((P, 1))
    n, ctr = _poisson_pieces(model.rate, kcp, mutant == 'drop_remainder')
    J = max(int(n.max()), 1)
    tau, delta = np.full((P, J), np.inf), np.zeros((P, J))
    lam = model.lam * (1.03 if mutant == 'laplace_scale' else 1.0)
    u_prev = np.zeros(P)
    for j in range(J):
        act = np.flatnonzero(n > j)
        v = u01(kcp[act], ctr[act])
        rem = (n[act] - j).astype(np.float64)
        pw = np.exp(np.log(v) / rem)
        up = 1.0 - pw if mutant == 'no_composition' else 1.0 - (1.0 - u_prev[act]) * pw
        u_prev[act] = up
        tau[act, j] = 1.0 + up * (model.Tm - 1.0)
        ul = u01(kcp[act], ctr[act] + _U(1))
        with np.errstate(divide='ignore'):
            delta[act, j] = np.where(ul < 0.5, lam * np.log(2.0 * ul), -(lam * np.log(2.0 * (1.0 - ul))))
        ctr[act] += _U(2)
    if mutant == 'no_composition':      # the sweep applies its pending time whenever a row has passed it: any order
        order = np.argsort(tau, axis=1, kind='stable')
        tau, delta = np.take_along_axis(tau, order, 1), np.take_along_axis(delta, order, 1)
    return n, tau, delta


def box_muller(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def restated_draws(model, keys, S, seed, mutant=None, chunk=8, samples=None, want_counts=False, noise_index=None):
    """{'yhat', 'trend'} [N][H][S] of the stream scheme at series keys `keys` [N] (samples: the sample indices, default
    0 .. S - 1); with want_counts also 'n_new' [N][S].  mutant: None or one of MUTANTS.  noise_index [H]: the index each row
    (in the model's increasing order) has in the caller's order, which counts the noise stream (default: its own)."""
    assert mutant is None or mutant in MUTANTS
    keys = np.asarray(keys, dtype=np.int64)
    N, H = len(keys), len(model.t)
    sidx = np.arange(S, dtype=np.int64) if samples is None else np.asarray(samples, dtype=np.int64)
    S = len(sidx)
    trend = np.empty((N, H, S))
    counts = np.empty((N, S), dtype=np.int64)
    for n0 in range(0, N, chunk):
        nc = min(chunk, N - n0)
        kk = np.repeat(keys[n0:n0 + nc], S)
        ss = np.tile(sidx, nc)
        kcp = stream_key(seed, kk, 0 * ss if mutant == 'no_sample_in_key' else ss, 0)
        cnt, tau, delta = restated_kinks(model, kcp, mutant)
        trend[n0:n0 + nc] = piecewise_paths(model, tau, delta, cnt).reshape(nc, S, H).transpose(0, 2, 1)
        counts[n0:n0 + nc] = cnt.reshape(nc, S)
    knz = stream_key(seed, np.repeat(keys, S), np.tile(sidx, N), 1).reshape(N, 1, S)
    if mutant == 'shared_noise':        # every 100th sample of an odd series reads the stream of the series before it
        share = (np.arange(N) % 2 == 1)[:, None, None] & (sidx % 100 == 0)[None, None, :]
        knz = np.where(share, np.roll(knz, 1, axis=0), knz)
    hh = np.arange(H) if noise_index is None else np.asarray(noise_index)
    h2 = (2 * hh.astype(np.uint64)).reshape(1, H, 1)
    u1 = u01(knz, h2)
    u2 = u01(knz, h2 if mutant == 'u2_from_u1' else h2 + _U(1))
    sig = model.sigma * (1.01 if mutant == 'noise_scale' else 1.0)
    z = box_muller(u1, u2)
    yhat = trend * model.opm[None, :, None] + model.xa[None, :, None] + (z * sig) * model.y_scale
    out = {'yhat': yhat, 'trend': trend}
    if want_counts:
        out['n_new'] = counts
    return out


# ---- 4. the battery ------------------------------------------------------------------------------------------------

def _z(name, value):
    return (name, 'z', float(value))


def _p(name, value):
    return (name, 'p', float(value))


def mean_stat(name, x, mean, var):
    """z of the mean of x against a law with the given mean and variance; where the law is a point mass (var = 0) the
    statistic is exact: p = 1 if every value is within 1e-12 (absolute, in the variable's units) of it, else 0"""
    x = np.asarray(x)
    if var <= 0.0:
        return _p(name + '[exact]', 1.0 if np.max(np.abs(x - mean)) <= 1e-12 else 0.0)
    return _z(name, (x.mean() - mean) / math.sqrt(var / x.size))


def count_stat(name, k, n, p):
    """k events in n trials of probability p: z where events and non-events both expect >= NORMAL_MIN_EVENTS, else the
    exact two-sided binomial p-value (doubling the smaller tail)"""
    k, n = int(k), int(n)
    if p <= 0.0:
        return _p(name + '[exact]', 1.0 if k == 0 else 0.0)
    if n * p >= NORMAL_MIN_EVENTS and n * (1.0 - p) >= NORMAL_MIN_EVENTS:
        return _z(name, (k - n * p) / math.sqrt(n * p * (1.0 - p)))
    lo, hi = stats.binom.cdf(k, n, p), stats.binom.sf(k - 1, n, p)
    return _p(name + '[binomial]', min(1.0, 2.0 * min(lo, hi)))


def chi2_stat(name, observed, expected):
    """chi-square p of counts against expected counts; the cell that expects least is merged into its neighbour until
    each expects >= CHI2_MIN_EXPECTED (never dropped)"""
    obs, exp = list(map(float, observed)), list(map(float, expected))
    assert abs(sum(obs) - sum(exp)) <= 1e-6 * max(1.0, sum(exp)), (name, sum(obs), sum(exp))
    while len(exp) > 1 and min(exp) < CHI2_MIN_EXPECTED:
        i = int(np.argmin(exp))
        e, o = exp.pop(i), obs.pop(i)
        j = i - 1 if i > 0 else 0               # into the left neighbour; the first cell into what follows it
        exp[j] += e
        obs[j] += o
    if len(exp) < 2:
        return _p(name + '[one cell]', 1.0 if obs == exp or exp[0] > 0 and abs(obs[0] - exp[0]) < 0.5 else 0.0)
    x2 = sum((o - e) ** 2 / e for o, e in zip(obs, exp))
    return _p(name, stats.chi2.sf(x2, len(exp) - 1))


def corr_stat(name, a, b):
    """z of mean(a b) for a, b standardised by their laws (mean 0, variance 1) and independent under the laws:
    variance 1 / n, so the correlation is compared with 0 at 1 / sqrt(n)"""
    return _z(name, float(np.mean(a * b)) * math.sqrt(a.size))


def ks_normal(x):
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    return stats.kstest(x, 'norm').pvalue


def _second_differences(L):
    return L[:, 2:, :] - 2.0 * L[:, 1:-1, :] + L[:, :-2, :]


ABS_MEAN, ABS_VAR = math.sqrt(2.0 / math.pi), 1.0 - 2.0 / math.pi


def battery(draws, model, fine, det_trend=None, xa=None, opm=None, ref=None, ks_rows=()):
    """The statistics of one call's draws {'yhat', 'trend'} [N][H][S] at identical parameters `model` and any keys.
    fine: (i0, i1), rows i0 .. i1 - 1 are increasing and equally spaced (the kink-detection block); every other
    statistic uses all rows, which must be increasing.  det_trend, xa, opm [N][H]: the deterministic trend, the additive
    term (y units) and 1 + the multiplicative term as the library under test reports them (default: the model's own).
    ref: draws of the independent sampler for the two-sample KS at rows ks_rows (logistic growth: required).
    -> [(name, kind, value)]; no statistic is left out for any case: where a law degenerates (rate 0) the statistic
    becomes an exact one."""
    yhat, trend = draws['yhat'], draws['trend']
    N, H, S = yhat.shape
    t = model.t
    assert (np.diff(t) > 0).all()
    bc = lambda a, d: (np.broadcast_to(d, (N, H)) if a is None else np.asarray(a))[:, :, None]     # noqa: E731
    det = bc(det_trend, model.det_trend())
    xa_, opm_ = bc(xa, model.xa), bc(opm, model.opm)
    laws = model.laws()
    lin = model.growth == 'linear'
    out = []

    # -- the noise: N(0, 1), independent across rows, samples and keys and of the trend
    z = (yhat - trend * opm_ - xa_) / (model.sigma * model.y_scale)
    nz = z.size
    out.append(_p('noise: KS against N(0,1)', ks_normal(z)))
    out.append(_z('noise: mean', z.mean() * math.sqrt(nz)))
    z2 = z * z
    out.append(_z('noise: variance', (z2.mean() - 1.0) / math.sqrt(2.0 / nz)))
    out.append(_z('noise: third moment', (z2 * z).mean() / math.sqrt(15.0 / nz)))
    out.append(_z('noise: fourth moment', ((z2 * z2).mean() - 3.0) / math.sqrt(96.0 / nz)))
    az = np.abs(z)
    for c in (3.0, 4.0, 4.5):
        out.append(count_stat('noise: beyond %g sigma' % c, (az > c).sum(), nz, 2.0 * stats.norm.sf(c)))
    a0 = (az - ABS_MEAN) / math.sqrt(ABS_VAR)
    out.append(corr_stat('noise: neighbouring keys', z[:-1], z[1:]))
    out.append(corr_stat('noise: neighbouring samples', z[:, :, :-1], z[:, :, 1:]))
    out.append(corr_stat('noise: neighbouring rows', z[:, :-1], z[:, 1:]))
    out.append(corr_stat('|noise|: neighbouring rows', a0[:, :-1], a0[:, 1:]))
    out.append(corr_stat('|noise|: neighbouring keys', a0[:-1], a0[1:]))
    out.append(corr_stat('|noise|: neighbouring samples', a0[:, :, :-1], a0[:, :, 1:]))
    del z2, az

    # -- the path in the coordinate in which it is piecewise linear
    if lin:
        L = (trend - model.fl) / model.y_scale
        Ldet = (det - model.fl) / model.y_scale
        guard_all = np.abs(L).max()
    else:
        q = (trend - model.fl) / (model.cap - model.fl)
        assert (q > 0).all() and (q < 1).all()
        L = np.log(q) - np.log1p(-q)
        qd = (det - model.fl) / (model.cap - model.fl)
        Ldet = np.log(qd) - np.log1p(-qd)
        guard_all = max(np.abs(L).max(), (1.0 / (q * (1.0 - q))).max())
        del q

    # -- kinks on the fine block
    i0, i1 = fine
    tf = t[i0:i1]
    dt = (tf[-1] - tf[0]) / (len(tf) - 1)
    assert len(tf) >= 9 and np.allclose(np.diff(tf), dt, rtol=1e-9, atol=0)
    rate_on = laws.rate > 0.0 and tf[0] >= 1.0
    thr = KINK_X0 * model.lam * dt
    # (the block's own largest value: the rounding of a second difference there; logistic: of the logit, 1 / (q (1 - q)))
    guard = np.abs(L[:, i0:i1, :]).max()
    if not lin:
        guard = max(guard, float((2.0 + 2.0 * np.cosh(L[:, i0:i1, :])).max()))
    assert thr > 64.0 * 2.2204460492503131e-16 * guard, ('kink threshold within rounding', thr, guard)
    d2 = _second_differences(L[:, i0:i1, :])                 # [N][W][S], window w centred on fine row w + 1
    occ = np.abs(d2) > thr
    W = occ.shape[1]
    mu = model.S_cp * 2.0 * dt if rate_on else 0.0
    p_occ = -math.expm1(-mu)
    if rate_on:
        assert mu <= WINDOW_MU_MAX * (1 + 1e-9) and neglected_mass(mu) < NEGLECTED_MAX, (mu, neglected_mass(mu))
    out.append(count_stat('kinks: window occupancy', occ.sum(), occ.size, p_occ))
    half = W // 2
    out.append(count_stat('kinks: occupancy, first half of the block', occ[:, :half].sum(), occ[:, :half].size, p_occ))
    out.append(count_stat('kinks: occupancy, second half of the block', occ[:, half:].sum(), occ[:, half:].size, p_occ))
    for par, nm in ((0, 'even'), (1, 'odd')):               # disjoint windows: the occupied count is Binomial(m, p)
        sel = occ[:, par::2, :]
        m = sel.shape[1]
        cnt = sel.sum(axis=1).ravel()
        obs = np.bincount(cnt, minlength=m + 1)
        exp = stats.binom.pmf(np.arange(m + 1), m, p_occ) * cnt.size
        out.append(chi2_stat('kinks: joint occupancy of the %s windows against the product' % nm, obs, exp))
    nk = occ.sum(axis=1).astype(np.float64)                 # [N][S]: occupied windows of the path
    if rate_on:
        # overlapping neighbours share half a window: Var = W p q + 2 (W - 1) cov, cov = P(both) - p^2 with
        # P(both) = 1 - 2 e^-mu + e^(-3 mu / 2) (the union of two neighbouring windows is 3 dt wide)
        q_ = math.exp(-mu)
        cov = (1.0 - 2.0 * q_ + math.exp(-1.5 * mu)) - p_occ ** 2
        nk0 = (nk - W * p_occ) / math.sqrt(W * p_occ * (1.0 - p_occ) + 2.0 * (W - 1) * cov)
        out.append(corr_stat('kink count: neighbouring keys', nk0[:-1], nk0[1:]))
        out.append(corr_stat('kink count: neighbouring samples', nk0[:, :-1], nk0[:, 1:]))
        out.append(corr_stat('kink count against |noise| at the last row', nk0, a0[:, -1, :]))
    else:
        for nm in ('neighbouring keys', 'neighbouring samples', 'against |noise| at the last row'):
            out.append(_p('kink count: %s[exact]' % nm, 1.0 if not nk.any() else 0.0))

    # -- isolated occupied windows (both flanking windows empty), disjoint ones: slope change and position of the kink
    ctr = np.arange(2, W - 2, 2)
    Lf = L[:, i0:i1, :]
    iso = occ[:, ctr, :] & ~occ[:, ctr - 2, :] & ~occ[:, ctr + 2, :]
    # window w spans fine rows w .. w + 2; the slopes beyond its flanks: rows (w + 2, w + 3) and (w - 1, w)
    slope_change = ((Lf[:, ctr + 3, :] - Lf[:, ctr + 2, :]) - (Lf[:, ctr, :] - Lf[:, ctr - 1, :])) / dt
    dsl = slope_change[iso]
    tent = d2[:, ctr, :][iso]
    if rate_on:
        w1, w2 = window_mixture(mu)
        lam = model.lam
        cdf = lambda x: w1 * laplace_cdf(x, lam) + w2 * laplace2_cdf(x, lam)      # noqa: E731
        out.append(_p('isolated window: slope change, KS against the Laplace mixture', stats.kstest(dsl, cdf).pvalue))
        e1 = w1 * lam + w2 * 1.5 * lam
        e2 = w1 * 2.0 * lam ** 2 + w2 * 4.0 * lam ** 2
        out.append(mean_stat('isolated window: mean |slope change|', np.abs(dsl), e1, e2 - e1 ** 2))
        out.append(mean_stat('isolated window: mean slope change', dsl, 0.0, e2))
        # one kink at tau: second difference = delta (dt - |tau - centre|), so 1 - d2 / (slope change dt) is
        # |tau - centre| / dt ~ U(0, 1); the windows with two kinks (w2 = mu / 2 <= 1.2 %) are part of the sample
        pos = 1.0 - tent / (dsl * dt)
        out.append(_p('isolated window: position of the kink, KS against U(0,1)',
                      stats.kstest(np.clip(pos, 0.0, 1.0), 'uniform').pvalue))
        out.append(count_stat('isolated window: share', iso.sum(), iso.size, p_occ * math.exp(-mu) ** 2))
    else:
        for nm in ('slope change, KS against the Laplace mixture', 'mean |slope change|', 'mean slope change',
                   'position of the kink, KS against U(0,1)', 'share'):
            out.append(_p('isolated window: %s[exact]' % nm, 1.0 if iso.sum() == 0 else 0.0))
    del d2, occ, iso

    # -- paths with one kink in all: its position, recovered from the end slope and the end value, is uniform
    D = L - Ldet
    out.append(_single_kink_position(D, t, laws, model.lam, 64.0 * 2.2204460492503131e-16 * guard_all))

    # -- the trend deviation's moments (linear growth) or its distribution against the independent sampler
    rows4 = sorted(set(int(round(x)) for x in np.linspace(0, H - 1, 5)[1:]))
    if lin:
        n = N * S
        # (in units of lam; at rate 0 every law is a point mass and the unit is the path's own size: 1e-12 relative)
        scale = model.lam if laws.rate > 0.0 else float(np.abs(Ldet).max())
        for h in rows4:
            d = D[:, h, :]
            v, m4 = float(laws.var(t[h])), float(laws.moment4(t[h]))
            out.append(mean_stat('trend deviation: mean at row %d' % h, d / scale, 0.0, v / scale ** 2))
            out.append(mean_stat('trend deviation: variance at row %d' % h, (d / scale) ** 2, v / scale ** 2,
                                 (m4 - v * v) / scale ** 4))
        h = H - 1
        d = D[:, h, :] / scale
        v, m4, m8 = (float(f(t[h])) for f in (laws.var, laws.moment4, laws.moment8))
        out.append(mean_stat('trend deviation: fourth moment at the last row', d ** 4, m4 / scale ** 4,
                             (m8 - m4 * m4) / scale ** 8))
        for a, b in ((rows4[0], rows4[-1]), (rows4[1], rows4[2])):
            prod = D[:, a, :] * D[:, b, :] / scale ** 2
            out.append(mean_stat('trend deviation: covariance of rows %d and %d' % (a, b), prod,
                                 float(laws.cov(t[a], t[b])) / scale ** 2,
                                 float(laws.var_of_product(t[a], t[b])) / scale ** 4))
        vend = float(laws.var(t[-1]))
        if vend > 0.0:
            e = D[:, -1, :] / math.sqrt(vend)
            out.append(corr_stat('end deviation: neighbouring keys', e[:-1], e[1:]))
            out.append(corr_stat('end deviation: neighbouring samples', e[:, :-1], e[:, 1:]))
            out.append(corr_stat('end deviation against the noise at the last row', e, z[:, -1, :]))
        else:
            for nm in ('neighbouring keys', 'neighbouring samples', 'against the noise at the last row'):
                out.append(_p('end deviation: %s[exact]' % nm, 1.0 if np.abs(D[:, -1, :]).max() <= 1e-12 else 0.0))
    else:
        assert ref is not None and len(ks_rows) >= 4
        for h in ks_rows:
            out.append(_p('trend: two-sample KS against the independent sampler at row %d' % h,
                          stats.ks_2samp(trend[:, h, :].ravel(), ref['trend'][:, h, :].ravel(), method='asymp').pvalue))
            out.append(_p('yhat: two-sample KS against the independent sampler at row %d' % h,
                          stats.ks_2samp(yhat[:, h, :].ravel(), ref['yhat'][:, h, :].ravel(), method='asymp').pvalue))
        # the end value's rank correlation across keys and samples: the logit of the end trend, standardised by the
        # independent sampler's moments
        qr = (ref['trend'][:, -1, :] - model.fl) / (model.cap - model.fl)
        lr = np.log(qr) - np.log1p(-qr)
        e = (L[:, -1, :] - lr.mean()) / lr.std()
        out.append(corr_stat('end deviation: neighbouring keys', e[:-1], e[1:]))
        out.append(corr_stat('end deviation: neighbouring samples', e[:, :-1], e[:, 1:]))
        out.append(corr_stat('end deviation against the noise at the last row', e, z[:, -1, :]))
    return out


def _single_kink_position(D, t, laws, lam, tol):
    """D [N][H][S]: the path minus the deterministic one, piecewise linear with D = 0 up to the first kink.  A path with
    one kink at tau before the last but one row is delta (t - tau)+ on every row: the end slope s (over the last gap)
    and the end value give tau = Tm - D(Tm) / s, and the path is recognised by |D - s (t - tau)+| <= tol on every row
    (tol: 64 roundings of the path's largest value, times (Tm - 1) / gap because s divides by the last gap; a second
    kink hides below it with probability of the order of tol / lam).  tau is uniform on (1, t_(H-2)].  What the rows
    cannot tell from one kink are several kinks within one gap between rows: their share of the recognised paths is at
    most
        eps = sum_gaps e^-r (e^(r w) - 1 - r w) / (r e^-r (1 - w_last)),   w = gap / (Tm - 1), r the rate,
    so the KS distance is reduced by eps before its p-value is taken (Kolmogorov's limit law).  Where eps is large
    (high rates) the statistic has no power and says so by p = 1; with no path recognised, p is the probability of
    that under the law."""
    name = 'single kink: position from the end slope and value, KS against U(0,1) less the contamination bound'
    N, H, S = D.shape
    gap = t[-1] - t[-2]
    tol = tol * (t[-1] - 1.0) / gap if t[-1] > 1.0 else tol
    s_hat = (D[:, -1, :] - D[:, -2, :]) / gap
    ok = np.abs(s_hat) > KINK_X0 * lam
    with np.errstate(divide='ignore', invalid='ignore'):
        tau = np.where(ok, t[-1] - D[:, -1, :] / s_hat, np.inf)
    resid = np.zeros((N, S))
    for h in range(H):
        resid = np.maximum(resid, np.abs(D[:, h, :] - np.where(ok, s_hat * np.clip(t[h] - tau, 0.0, None), np.inf)))
    r = laws.rate
    if not (r > 0.0 and t[0] == 1.0):
        return _p(name + '[exact]', 1.0 if not np.any(np.abs(D) > tol) else 0.0)
    span = t[-2] - 1.0
    sel = ok & (resid <= tol) & (tau > 1.0) & (tau <= t[-2] - 1e-6 * gap)
    u = (tau[sel] - 1.0) / span
    w = np.diff(t) / (t[-1] - 1.0)
    p_one = r * math.exp(-r) * (1.0 - w[-1])
    if u.size == 0:
        return _p(name + '[no such path]', (1.0 - p_one) ** (N * S))
    eps = float(np.sum(np.exp(-r) * (np.expm1(r * w) - r * w)) / p_one) + 1e-6
    dist = stats.kstest(u, 'uniform').statistic
    return _p(name, stats.kstwobign.sf(math.sqrt(u.size) * max(dist - eps, 0.0)))


def cross_stats(draws_a, draws_b, model, what):
    """two calls at the same parameters whose streams must be independent (two seeds at the same keys): the
    correlation of the noise, of the last row's trend and of the yhat draws between them"""
    out = []
    sd = model.sigma * model.y_scale
    za, zb = [(d['yhat'] - d['trend'] * model.opm[None, :, None] - model.xa[None, :, None]) / sd
              for d in (draws_a, draws_b)]
    out.append(corr_stat('%s: noise' % what, za, zb))
    v = float(model.laws().var(model.t[-1])) if model.growth == 'linear' else 0.0
    if v > 0.0:
        ea, eb = [(d['trend'][:, -1, :] - model.det_trend()[-1]) / model.y_scale / math.sqrt(v)
                  for d in (draws_a, draws_b)]
        out.append(corr_stat('%s: end deviation' % what, ea, eb))
    return out


def failures(results):
    """the statistics outside the thresholds"""
    bad = []
    for name, kind, value in results:
        ok = (abs(value) <= Z_MAX) if kind == 'z' else (value >= P_MIN)
        if not (ok and math.isfinite(value)):
            bad.append((name, kind, value))
    return bad


def extremes(results):
    """(largest |z|, smallest p)"""
    zs = [abs(v) for _, k, v in results if k == 'z']
    ps = [v for _, k, v in results if k == 'p']
    return (max(zs) if zs else 0.0), (min(ps) if ps else 1.0)
