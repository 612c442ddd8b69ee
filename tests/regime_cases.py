"""The regime panel: deterministic histories of the kinds `synth.make_panel` never makes -- mostly zeros, a level of
1e8 with a wiggle of +-5, one spike of 1e6, sign changes, steps, a constant stretch before a ramp, near-noiseless
series, values at 1e-300 and 1e300 -- for the fit kernels (tests/test_gpu_regimes.py) and, first, for the CPU oracle
alone (tests/test_regime_cases.py: whatever the GPU tests rely on the oracle for is established there).

Linear regimes are built on `synth.daily_grid(T)` at T = 730 for cfg2's model (yearly 10 + weekly 3, additive: what
`ModelSpec.auto_seasonalities` gives these dates) and, where they make sense on 90 rows, at T = 90 for short_90's model
(weekly 3) and for Newton.  The logistic regimes use ref_logistic_multiplicative's model on 730 rows.  Every stochastic
regime comes with the seeds SEEDS; a series is named '<regime>' or '<regime>#<seed>'.  Values are rounded where the
reference's schema (`quantity`: an integer count) would round them; the tiny / huge regimes are an integer regime
scaled by an exact power-of-ten literal and are not integers.

Nothing here depends on the library under test: numpy only."""
import zlib

import numpy as np

DAY_NS = 86400 * 10 ** 9
START_NS = 1514764800 * 10 ** 9            # synth.START_NS (2018-01-01T00:00:00Z); asserted equal in the CPU test
SEEDS = (0, 1, 2)
T_LONG, T_SHORT = 730, 90
CONST_ROWS = 400                           # const_then_ramp: the constant stretch


def daily_grid(T):
    return START_NS + DAY_NS * np.arange(T, dtype=np.int64)


def _rng(name, seed):
    return np.random.default_rng([zlib.crc32(name.encode()), seed])


def _base(T, rng):
    """A smooth base of level ~2e4: trend, weekly and yearly sines (what make_panel makes, one series, no noise)."""
    t = np.arange(T, dtype=np.float64)
    u = t / (T - 1)
    return 2.0e4 * (1.0 + 0.3 * u + 0.1 * np.sin(2 * np.pi * t / 7.0 + rng.uniform(0, 6)) +
                    0.15 * np.sin(2 * np.pi * t / 365.25 + rng.uniform(0, 6)))


def _in_model(T, rng, rel):
    """linear + weekly + yearly sine: a signal the model holds exactly, with relative noise `rel`."""
    t = np.arange(T, dtype=np.float64)
    sig = 5.0e4 * (1.0 + 0.4 * t / (T - 1) + 0.08 * np.sin(2 * np.pi * t / 7.0 + 0.3) +
                   0.12 * np.cos(2 * np.pi * t / 365.25 + 1.1))
    return sig * (1.0 + rel * rng.normal(0, 1, T)) if rel > 0 else sig


def _offset(T, rng, level):
    t = np.arange(T, dtype=np.float64)
    return level + 0.01 * t + 5.0 * np.sin(2 * np.pi * t / 7.0) + rng.normal(0, 1, T)


def _offgrid_kink(T, rng, rel):
    """A trend kink between two rows of the changepoint grid (the grid of 25 over the first 80 % has a point about every
    23 rows at T = 730; row 0.5137 (T - 1) lies between two of them)."""
    t = np.arange(T, dtype=np.float64)
    u = t / (T - 1)
    sig = 4.0e4 * (1.0 + 0.2 * u + 0.9 * np.maximum(u - 0.5137, 0.0) + 0.05 * np.sin(2 * np.pi * t / 7.0))
    return sig * (1.0 + rel * rng.normal(0, 1, T))


def _intermittent(T, rng):
    return rng.poisson(0.15, T).astype(np.float64)


def _small_counts(T, rng):
    t = np.arange(T, dtype=np.float64)
    return rng.poisson(3.0 + 2.0 * np.sin(2 * np.pi * t / 7.0)).astype(np.float64)


def _binary(T, rng):
    return (rng.uniform(size=T) < 0.4).astype(np.float64)


def _single_spike(T, rng):
    y = np.round(_base(T, rng) + rng.normal(0, 500.0, T))
    y[int(rng.integers(T // 4, 3 * T // 4))] = 1.0e6
    return y


def _one_nonconstant(T, rng):
    y = np.full(T, 7.0)
    y[(2 * T) // 3] = 8.0
    return y


def _sign_crossing(T, rng):
    t = np.arange(T, dtype=np.float64)
    return np.round(-3000.0 + 6000.0 * t / (T - 1) + 800.0 * np.sin(2 * np.pi * t / 7.0) + rng.normal(0, 150.0, T))


def _negative(T, rng):
    return -np.round(_base(T, rng) + rng.normal(0, 500.0, T))


def _step(T, rng):
    """A level step of 2 base units behind the changepoint range (no changepoint after 0.8 T can take it up)."""
    y = _base(T, rng) + rng.normal(0, 500.0, T)
    y[int(0.9 * T):] += 2.0 * 2.0e4
    return np.round(y)


def _const_then_ramp(T, rng):
    c = CONST_ROWS if T == T_LONG else (T * CONST_ROWS) // T_LONG
    y = np.full(T, 1200.0)
    y[c:] += 25.0 * np.arange(1, T - c + 1)
    return y


def _heavy_tail(T, rng):
    return np.round(_base(T, rng) + 300.0 * rng.standard_t(1.5, T))


# name -> (builder(T, rng) -> y, stochastic, built at T = 90 as well)
LINEAR = {
    'intermittent': (_intermittent, True, True),
    'small_counts': (_small_counts, True, True),
    'binary': (_binary, True, True),
    'single_spike': (_single_spike, True, True),
    'one_nonconstant': (_one_nonconstant, False, True),
    'sign_crossing': (_sign_crossing, True, True),
    'negative': (_negative, True, True),
    'step': (_step, True, True),
    'const_then_ramp': (_const_then_ramp, False, True),
    'offset_1e4': (lambda T, r: np.round(_offset(T, r, 1.0e4)), True, False),
    'offset_1e6': (lambda T, r: np.round(_offset(T, r, 1.0e6)), True, True),
    'offset_1e8': (lambda T, r: np.round(_offset(T, r, 1.0e8)), True, True),
    'in_model_rel_1e-3': (lambda T, r: np.round(_in_model(T, r, 1e-3)), True, False),
    'in_model_rel_1e-5': (lambda T, r: np.round(_in_model(T, r, 1e-5) * 1e3) / 1e3, True, False),
    'in_model_rel_1e-7': (lambda T, r: _in_model(T, r, 1e-7), True, False),
    'in_model_rel_1e-9': (lambda T, r: _in_model(T, r, 1e-9), True, False),
    'in_model_rel_0': (lambda T, r: _in_model(T, r, 0.0), False, False),
    'offgrid_kink_rel_1e-6': (lambda T, r: _offgrid_kink(T, r, 1e-6), True, False),
    'heavy_tail': (_heavy_tail, True, True),
    'tiny_1e-300': (lambda T, r: _sign_crossing(T, _rng('sign_crossing', 0)) * 1e-300, False, False),
    'huge_1e300': (lambda T, r: _sign_crossing(T, _rng('sign_crossing', 0)) * 1e300, False, False),
}
# (below the schema's resolution nothing can be rounded: the in-model regimes from 1e-7 down and the kink keep their
# float64 values -- they are the near-noiseless series of the issue, not counts)

# a regime scaled by a power of two: theta of the unscaled series bit for bit, y_scale scaled exactly (the judge test)
POW2_OF = {'pow2_-996': ('sign_crossing#0', 2.0 ** -996), 'pow2_996': ('sign_crossing#0', 2.0 ** 996)}


def names(T=T_LONG):
    out = []
    for name, (_, stochastic, short) in LINEAR.items():
        if T == T_SHORT and not short:
            continue
        out += ['%s#%d' % (name, s) for s in SEEDS] if stochastic else [name]
    return out


def linear(name, T=T_LONG):
    """(ds, y) of one linear regime series, '<regime>' or '<regime>#<seed>'."""
    reg, _, seed = name.partition('#')
    if reg in POW2_OF:
        src, sc = POW2_OF[reg]
        ds, y = linear(src, T)
        return ds, y * sc
    fn, stochastic, short = LINEAR[reg]
    assert (seed != '') == stochastic, name
    y = np.asarray(fn(T, _rng(reg, int(seed or 0))), dtype=np.float64)
    assert y.shape == (T,) and np.isfinite(y).all()
    return daily_grid(T), y


def linear_panel(T=T_LONG):
    """(names, ds, y [n][T]) of every linear regime series at T."""
    nm = names(T)
    return nm, daily_grid(T), np.array([linear(n, T)[1] for n in nm])


# ---- logistic growth, multiplicative seasonality (ref_logistic_multiplicative's model) --------------------------------

def _sigmoid(T, k=6.0, m=0.5):
    u = np.arange(T, dtype=np.float64) / (T - 1)
    return 1.0 / (1.0 + np.exp(-k * (u - m)))


def _seas(T):
    t = np.arange(T, dtype=np.float64)
    return 0.1 * np.sin(2 * np.pi * t / 7.0 + 0.4) + 0.15 * np.sin(2 * np.pi * t / 365.25 + 2.0)


def logistic(name, T=T_LONG):
    """(ds, y, floor, cap) of one logistic regime series."""
    reg, _, seed = name.partition('#')
    rng = _rng(reg, int(seed or 0))
    floor = 0.0
    if reg == 'at_cap':                       # saturates early; clipped at the cap: a third of the rows sit ON it
        cap = 30000.0
        y = np.minimum(np.round(1.05 * cap * _sigmoid(T, 12.0, 0.3) * (1.0 + _seas(T)) + rng.normal(0, 300.0, T)), cap)
    elif reg == 'above_cap':                  # the cap the caller gave is below what the series reaches
        cap = 20000.0
        y = np.round(1.3 * cap * _sigmoid(T) * (1.0 + _seas(T)) + rng.normal(0, 300.0, T))
    elif reg == 'zeros_multiplicative':       # counts that start at zero: trend * (1 + seasonality) with trend ~ 0
        cap = 40.0
        y = rng.poisson(30.0 * _sigmoid(T, 14.0, 0.6) * (1.0 + _seas(T))).astype(np.float64)
    elif reg == 'negative_floor':
        floor, cap = -5000.0, 25000.0
        y = np.round(floor + 0.9 * (cap - floor) * _sigmoid(T) * (1.0 + _seas(T)) + rng.normal(0, 300.0, T))
    elif reg == 'noiseless_sigmoid':
        cap = 50000.0
        y = np.round(0.9 * cap * _sigmoid(T) * (1.0 + _seas(T)))
    else:
        raise KeyError(name)
    assert np.isfinite(y).all()
    return daily_grid(T), y, floor, cap


LOGISTIC_STOCHASTIC = ('at_cap', 'above_cap', 'zeros_multiplicative', 'negative_floor')


def logistic_names():
    return ['%s#%d' % (r, s) for r in LOGISTIC_STOCHASTIC for s in SEEDS] + ['noiseless_sigmoid']


# ---- the models ---------------------------------------------------------------------------------------------------------

YEARLY = {'name': 'yearly', 'period': 365.25, 'fourier_order': 10}
WEEKLY = {'name': 'weekly', 'period': 7, 'fourier_order': 3}


def seasonalities(T):
    return [dict(YEARLY), dict(WEEKLY)] if T >= T_LONG else [dict(WEEKLY)]


def oracle_spec(T=T_LONG, growth='linear', eval_mode=None, **opt):
    """oracle.canon_lib spec of the regime model at T; eval_mode defaults to the quadratic form for linear growth."""
    from oracle import canon_lib as cl
    mode = 'additive' if growth == 'linear' else 'multiplicative'
    if eval_mode is None:
        eval_mode = int(growth == 'linear')
    return cl.make_spec(growth=growth, seasonalities=[(s['period'], s['fourier_order'], mode, 10.0) for s in seasonalities(T)],
                        eval_mode=eval_mode, **opt)


def noise_free_pair():
    """(ds, y [2][120]) -- the noise-free pair of tests/test_gpu_parity.py::test_odd_shapes_against_oracle (a line with a
    weekly sine, a line), for the weekly model: there on the small-panel route only, here on every route."""
    t = np.arange(120.0)
    return daily_grid(120), np.stack([50 + 0.5 * t + 3 * np.sin(2 * np.pi * t / 7), 20 + 0.1 * t])
