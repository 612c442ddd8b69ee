"""The cases of the predictive sampler's distribution tests (tests/sampler_ref.py): hand-made models -- theta, grid and
y_scale written out, no fit -- of N = 64 series with identical parameters and different keys, 4 096 samples, 32 rows.
Shared by tests/test_sampler_ref.py (CPU: the restated stream scheme and the independent sampler) and
tests/test_gpu_sampler.py (the kernel).

Rows (scaled time t, one shared future calendar): 21 equally spaced rows from t = 1 at spacing 0.012 / S_cp -- the block
on which kinks are detected, windows of two spacings holding mu = 0.024 expected changepoints, so that an occupied window
holds three or more with probability mu^2 / 6 = 9.6e-5 < 1e-4 -- then 11 rows equally spaced up to Tm = 1.5.  The horizon
of 0.5 gives the rates S_cp / 2: 0.5 (no full piece of the Poisson draw), 8 (exactly one), 12.5 (one and a remainder),
30 (three and a remainder; S_cp = TSF_MAX_S = 60).  These are the smallest shapes at which the statistics have power;
each array of draws is 64 MB.

Seeds and keys are fixed here, so every test is deterministic; they are not to be tuned after a look at a result."""
import numpy as np

from tests import forecast_cases as fcs, sampler_ref as sr

N = 64
NS = 4096
H = 32
N_FINE = 21
SEED = 20240611
T_SCALE_NS = 10 ** 16
START_NS = int(fcs.T0)

# name: (growth, mode of the one extra column (None: no column), n_changepoints, S, rows)
CASES = {
    'lin_add_s1':   ('linear', 'additive', 1, 1, 'future'),
    'lin_add_s16':  ('linear', 'additive', 16, 16, 'future'),
    'lin_add_s25':  ('linear', 'additive', 25, 25, 'future'),
    'lin_add_s60':  ('linear', 'additive', 60, 60, 'future'),
    'no_cp':        ('linear', 'additive', 0, 0, 'future'),         # S_cp = 1, lam = 1e-8: noise only
    'rate0':        ('linear', 'additive', 25, 25, 'history'),      # every row at t <= 1
    'lin_mul_s16':  ('linear', 'multiplicative', 16, 16, 'future'),
    'logistic_s3':  ('logistic', 'additive', 3, 3, 'future'),
    'unsorted_s16': ('linear', 'additive', 16, 16, 'unsorted'),
}
LOGISTIC_KS_ROWS = (12, 20, 24, 28, 31)

FAMILIES = ('index', 'high_word', 'low_word', 'stride', 'next_seed')


def keys_of(family):
    """(series_key [N] or None for the default -- the series index --, seed)"""
    n = np.arange(N, dtype=np.int64)
    if family == 'index':
        return None, SEED
    if family == 'high_word':           # (series_id << 32) ^ dim_id, the series_id varying
        return ((n + 8) << 32) ^ 5, SEED
    if family == 'low_word':            # the dim_id varying
        return (np.int64(751) << 32) ^ n, SEED
    if family == 'stride':
        return 7919 * n + 3, SEED
    if family == 'next_seed':           # the default keys at the next seed
        return None, SEED + 1
    raise ValueError(family)


def row_offsets_ns(S_cp, rows):
    """ns after START_NS of the H rows (exact integers; the last is 1.5 T_SCALE_NS)"""
    step = 12 * 10 ** 13 // S_cp                            # 0.012 / S_cp of the time scale
    assert step * S_cp == 12 * 10 ** 13
    fine = T_SCALE_NS + step * np.arange(N_FINE, dtype=np.int64)
    end = 3 * T_SCALE_NS // 2
    j = np.arange(1, H - N_FINE + 1, dtype=np.int64)
    coarse = fine[-1] + ((end - fine[-1]) * j) // (H - N_FINE)
    off = np.concatenate([fine, coarse])
    assert off[-1] == end and (np.diff(off) > 0).all()
    if rows == 'history':                                   # the same pattern on (0.8, 1]: behind the fitted changepoints
        off = T_SCALE_NS - ((end - off) * 2) // 5
        assert (np.diff(off) > 0).all() and off[-1] == T_SCALE_NS
    return off


def end_state(growth, k, m, t_change, delta):
    """(k, m) after the fitted changepoints (fbprophet's piecewise_linear / piecewise_logistic)"""
    for tc, d in zip(t_change, delta):
        kn = k + d
        m = m - tc * d if growth == 'linear' else m + (tc - m) * (1.0 - k / kn)
        k = kn
    return k, m


def make(name):
    """A forecast_cases.Case (model, spec, theta, y_scale, grid, fut, floor, cap, extra, ...) with .sampler: the
    sampler_ref.Model of its identical series on the rows in increasing order, .perm: the order of the rows handed to
    the library (rows[perm]), .fine: the kink-detection block."""
    from time_series_spark_amd import _lib, forecaster as fc
    growth, mode, ncp, S, rows = CASES[name]
    S_cp = max(S, 1)
    c = fcs.Case()
    c.name, c.N, c.H, c.K, c.shared = name, N, H, 1, True
    c.model = {'growth': growth, 'n_changepoints': ncp, 'seasonalities': [], 'extra_modes': [mode]}
    c.spec = fc.ModelSpec(growth=growth, n_changepoints=ncp, seasonalities=[], extra=[{'name': 'x', 'mode': mode}])
    assert c.spec.theta_stride == 3 + ncp + 1
    t_change = 0.05 + 0.75 * (np.arange(S) + 0.5) / S_cp
    j = np.arange(S)
    if growth == 'linear':
        k, m, sigma, y_scale, floor, cap = 0.4, 0.6, 0.05, 250.0, 0.0, None
        delta = 0.3 * (-1.0) ** j * (1.0 + 0.5 * np.cos(j))
        if name == 'no_cp':
            k, m = 0.0, 0.0                                 # the trend draws are the deviation itself, at lam = 1e-8
    else:
        k, m, sigma, y_scale, floor, cap = 1.1, 1.0, 0.04, 400.0, 20.0, 520.0
        delta = np.array([0.3, -0.25, 0.35])
    beta = 0.3 if mode == 'additive' else 0.2
    theta = np.zeros(3 + ncp + 1)
    theta[:3] = k, m, np.log(sigma)
    theta[3:3 + S] = delta
    theta[3 + ncp] = beta
    c.theta = np.tile(theta, (N, 1))
    c.y_scale = np.full(N, y_scale)
    c.floor = np.full(N, floor)
    c.cap = None if cap is None else np.full(N, cap)
    c.S = np.full(N, S)
    grid = np.zeros(1, dtype=_lib.GRID_DTYPE)
    grid['start_ns'], grid['t_scale_ns'], grid['T'], grid['S'], grid['NT'] = START_NS, T_SCALE_NS, 1000, S, 16
    grid['t_change'] = fcs.POISON_TCHANGE
    grid['t_change'][0, :S] = t_change
    c.grid = grid
    off = row_offsets_ns(S_cp, rows)
    x = np.cos(0.7 * np.arange(H)) + 0.25                   # the extra column on the rows in increasing order
    c.perm = np.arange(H)
    if rows == 'unsorted':
        c.perm = np.random.default_rng(5).permutation(H)
    c.fut = START_NS + off[c.perm]
    c.extra = x[c.perm][None, :]
    t = off.astype(np.float64) / float(T_SCALE_NS)
    ke, me = end_state(growth, k, m, t_change, delta)
    lam = (np.abs(delta).sum() / S_cp if S else 0.0) + 1e-8
    xa = beta * x * y_scale if mode == 'additive' else np.zeros(H)
    opm = 1.0 + beta * x if mode == 'multiplicative' else np.ones(H)
    c.sampler = sr.Model(growth, ke, me, S_cp, lam, sigma, y_scale, t, xa=xa, opm=opm, floor=floor,
                         cap=0.0 if cap is None else cap)
    c.fine = (0, N_FINE)
    return c
