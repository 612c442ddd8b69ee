"""Panels with injected outliers for the screening tests.  Not a test file: what tests/test_gpu_screen.py fits and
screens; importable without a GPU.

A case is synth.make_panel(8, T, growth, seed=21) -- the clean series -- with three spikes of 20 x the series' range
added to each series on rows drawn by RandomState(5), a weekly seasonality of order 3, and (logistic growth) floor 0
and cap = 1.1 x the CLEAN series' maximum."""
import numpy as np

from time_series_spark_amd import synth

WEEKLY3 = {'name': 'weekly', 'period': 7, 'fourier_order': 3}
N_SPIKED = 8
N_SPIKES = 3
KINDS = {'lin120': ('linear', 'additive', 120), 'lin257': ('linear', 'additive', 257),
         'log200': ('logistic', 'multiplicative', 200)}
SCREEN = dict(threshold=5.0, max_share=0.1, min_rows=10)


class Case(object):
    pass


def make(kind, n_clean_extra=0, dtype=np.float64):
    """kind: a key of KINDS.  n_clean_extra: clean series (seed 22) appended after the 8 spiked ones."""
    growth, mode, T = KINDS[kind]
    c = Case()
    c.kind, c.growth, c.mode, c.T = kind, growth, mode, T
    c.ds, clean = synth.make_panel(N_SPIKED, T, growth, seed=21)
    rs = np.random.RandomState(5)
    c.rows = np.stack([np.sort(rs.choice(T, N_SPIKES, replace=False)) for _ in range(N_SPIKED)])
    y = clean.copy()
    for n in range(N_SPIKED):
        y[n, c.rows[n]] += 20.0 * (clean[n].max() - clean[n].min())
    if n_clean_extra:
        _, more = synth.make_panel(n_clean_extra, T, growth, seed=22)
        clean, y = np.concatenate([clean, more]), np.concatenate([y, more])
    c.clean, c.y = clean, (np.rint(y) if dtype == np.int32 else y).astype(dtype)
    c.N = len(y)
    c.injected = np.zeros(y.shape, bool)
    for n in range(N_SPIKED):
        c.injected[n, c.rows[n]] = True
    c.floor = np.zeros(c.N) if growth == 'logistic' else None
    c.cap = 1.1 * clean.max(axis=1) if growth == 'logistic' else None
    c.spec_kw = dict(growth=growth, seasonality_mode=mode, seasonalities=[dict(WEEKLY3)])
    return c


def ragged(c, y=None):
    """the case's panel as a ragged one: (offsets, ds [N * T], y [N * T])"""
    y = c.y if y is None else y
    return np.arange(c.N + 1, dtype=np.int64) * c.T, np.tile(c.ds, c.N), np.ascontiguousarray(y).reshape(-1)
