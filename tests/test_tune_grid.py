"""CPU tests of prior-scale tuning (no GPU): the library exports tsf_tune and the binding's structs and constants match
include/tsf.h; the grid's candidate order and prior-scale replacement rules; the choice rule's numpy restatement
(tests/tune_rule.py) on NaN, ties, all-NaN rows and plan statuses; the validator's `tune` section."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import tune_rule
from time_series_spark_amd import _lib, features, forecaster as fc

WEEKLY = {'name': 'weekly', 'period': 7, 'fourier_order': 3}
YEARLY = {'name': 'yearly', 'period': 365.25, 'fourier_order': 10}

LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "tsf.h"
#include "tsf_dev.h"
int main(void)
{
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(tsf_tune_out), (int)offsetof(tsf_tune_out, score),
           (int)offsetof(tsf_tune_out, cand_status), (int)offsetof(tsf_tune_out, best),
           (int)offsetof(tsf_tune_out, series_status), (int)offsetof(tsf_tune_out, fit), (int)sizeof(tsf_cv_args));
    printf("%d %d %d %d %d %d %d\n", TSF_TUNE_MSE, TSF_TUNE_RMSE, TSF_TUNE_MAE, TSF_TUNE_MAPE, TSF_TUNE_NO_SCORE,
           TSF_TUNE_MAX_CAND, TSF_CV_FIT_FAILED);
    return 0;
}
'''


def test_exports_and_layout(built, tmp_path):
    L = _lib.load()
    for sym in ('tsf_tune', 'tsf_last_tune_counts'):
        assert sym in _lib.EXPORTS and hasattr(L, sym), sym
    src = tmp_path / 'layout.c'
    src.write_text(LAYOUT_C)
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(helpers.ROOT, 'include'), str(src),
                           '-o', exe])
    lines = subprocess.check_output([exe]).decode().split('\n')
    sizes = [int(x) for x in lines[0].split()]
    T = _lib.TsfTuneOut
    assert sizes == [ctypes_sizeof(T), T.score.offset, T.cand_status.offset, T.best.offset, T.series_status.offset,
                     T.fit.offset, ctypes_sizeof(_lib.TsfCvArgs)]
    consts = [int(x) for x in lines[1].split()]
    assert consts == [_lib.TUNE_MSE, _lib.TUNE_RMSE, _lib.TUNE_MAE, _lib.TUNE_MAPE, _lib.TUNE_NO_SCORE,
                      _lib.TUNE_MAX_CAND, _lib.CV_FIT_FAILED]
    assert tune_rule.TUNE_NO_SCORE == _lib.TUNE_NO_SCORE and tune_rule.CV_OK == _lib.CV_OK


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_grid_order_first_axis_slowest():
    spec = fc.ModelSpec(seasonalities=[YEARLY, WEEKLY])
    # the dict's own order does not matter: the axes go in TUNE_AXES order
    grid = {'seasonality_prior_scale': [0.1, 1.0, 10.0], 'changepoint_prior_scale': [0.001, 0.5]}
    cands, params = fc.tune_candidates(spec, grid)
    assert len(cands) == 6
    want = [(a, b) for a in (0.001, 0.5) for b in (0.1, 1.0, 10.0)]
    assert list(zip(params['changepoint_prior_scale'], params['seasonality_prior_scale'])) == want
    for c, (a, b) in zip(cands, want):
        cs = c.to_c()
        assert cs.changepoint_prior_scale == a
        assert [cs.seas_prior_scale[i] for i in range(2)] == [b, b]      # every seasonality
    assert set(params) == {'changepoint_prior_scale', 'seasonality_prior_scale'}
    # nothing but the prior scales differs from the base
    base = spec.to_c()
    for c in cands:
        cs = c.to_c()
        for name, _ in _lib.TsfSpec._fields_:
            if name not in ('changepoint_prior_scale', 'seas_prior_scale'):
                a, b = getattr(cs, name), getattr(base, name)
                assert (list(a) == list(b)) if hasattr(a, '__len__') else a == b, name


def test_seasonality_axis_overrides_per_seasonality_scales():
    spec = fc.ModelSpec(seasonalities=[dict(YEARLY, prior_scale=3.0), dict(WEEKLY, prior_scale=0.5)])
    cands, _ = fc.tune_candidates(spec, {'seasonality_prior_scale': [2.0]})
    assert [s['prior_scale'] for s in cands[0].seasonalities] == [2.0, 2.0]
    assert [s['prior_scale'] for s in spec.seasonalities] == [3.0, 0.5]     # the base is not touched


def _holiday_spec(regressor_scale):
    hol = features.normalize_holidays([{'holiday': 'xmas', 'ds': ['2020-12-25', '2021-12-25'], 'lower_window': -1,
                                        'upper_window': 0}, {'holiday': 'ny', 'ds': ['2021-01-01']}])
    names, scales, _ = features.holiday_columns(hol)
    reg = {'name': 'price'}
    if regressor_scale is not None:
        reg['prior_scale'] = regressor_scale
    extra = [{'name': n, 'prior_scale': s} for n, s in zip(names, scales)] + [reg]
    return fc.ModelSpec(seasonalities=[WEEKLY], extra=extra, holidays=hol, holidays_prior_scale=10.0), len(names)


@pytest.mark.parametrize('reg_scale', [4.0, None])
def test_holidays_axis_leaves_regressors_alone(reg_scale):
    spec, n_hol = _holiday_spec(reg_scale)
    assert n_hol == 3
    reg_before = spec.to_c().extra_prior_scale[n_hol]
    cands, params = fc.tune_candidates(spec, {'holidays_prior_scale': [0.05, 5.0]})
    assert list(params['holidays_prior_scale']) == [0.05, 5.0]
    for c, v in zip(cands, (0.05, 5.0)):
        cs = c.to_c()
        assert [cs.extra_prior_scale[i] for i in range(n_hol)] == [v] * n_hol
        assert cs.extra_prior_scale[n_hol] == reg_before            # (also where it followed holidays_prior_scale)
        assert cs.seas_prior_scale[0] == spec.to_c().seas_prior_scale[0]


def test_grid_errors():
    spec = fc.ModelSpec(seasonalities=[WEEKLY])
    bare = fc.ModelSpec(seasonalities=[])
    for g in ({}, {'yearly_seasonality': [1.0]}, {'changepoint_prior_scale': []},
              {'changepoint_prior_scale': [0.1, -1.0]}, {'changepoint_prior_scale': [float('nan')]},
              {'holidays_prior_scale': [1.0]}):
        with pytest.raises(ValueError):
            fc.tune_candidates(spec, g)
    with pytest.raises(ValueError):
        fc.tune_candidates(bare, {'seasonality_prior_scale': [1.0]})
    ds = np.arange(100, dtype=np.int64) * fc.DAY_NS
    y = np.ones((1, 100))
    with pytest.raises(ValueError):                 # exactly one of grid / candidates
        fc.tune(spec, ds, y, 10 * fc.DAY_NS)
    with pytest.raises(ValueError):
        fc.tune(spec, ds, y, 10 * fc.DAY_NS, grid={'changepoint_prior_scale': [0.1]}, candidates=[spec])
    with pytest.raises(ValueError):
        fc.tune(spec, ds, y, 10 * fc.DAY_NS, grid={'changepoint_prior_scale': [0.1]}, metric='smape')


def test_choice_rule():
    nan = np.nan
    score = np.array([[3.0, 1.0, 1.0, 2.0],          # tie: the first minimum
                      [nan, 2.0, nan, 0.5],          # NaN never chosen
                      [nan, nan, nan, nan],          # no score
                      [nan, nan, nan, nan],          # plan status kept
                      [np.inf, 7.0, 7.0, nan],       # inf is not finite
                      [5.0, 5.0, 5.0, 5.0]])         # constant: candidate 0
    plan = np.array([0, 0, 0, _lib.CV_LESS_THAN_HORIZON, 0, 0])
    best, st = tune_rule.choose(score, plan)
    assert list(best) == [1, 3, -1, -1, 1, 0]
    assert list(st) == [0, 0, _lib.TUNE_NO_SCORE, _lib.CV_LESS_THAN_HORIZON, 0, 0]
    # as np.nanargmin where a row has a finite score
    fin = np.isfinite(score).any(axis=1) & (plan == 0)
    with np.errstate(invalid='ignore'):
        ref = [int(np.nanargmin(np.where(np.isfinite(r), r, np.nan))) for r in score[fin]]
    assert list(best[fin]) == ref


def test_validator_parses_tune_section():
    from time_series_spark_amd.jobs import prophet_validator as pv
    assert pv.tune_settings({'cv': {'horizon': '30 days'}}) is None
    grid, metric = pv.tune_settings({'tune': {'changepoint_prior_scale': [0.01, 0.1], 'holidays_prior_scale': 1,
                                              'metric': 'MAE'}})
    assert grid == {'changepoint_prior_scale': [0.01, 0.1], 'holidays_prior_scale': [1.0]} and metric == 'mae'
    grid, metric = pv.tune_settings({'tune': {'seasonality_prior_scale': [0.1, 10]}})
    assert grid == {'seasonality_prior_scale': [0.1, 10.0]} and metric == 'rmse'
    for bad in ({'metric': 'rmse'}, {'changepoint_prior_scale': []}, {'changepoint_prior_scale': [1.0], 'metric': 'r2'},
                {'n_changepoints': [10]}):
        with pytest.raises(ValueError):
            pv.tune_settings({'tune': bad})
