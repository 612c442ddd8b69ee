"""CPU tests of model-structure selection: the numpy restatement of tsf_select's choice rule (tests/select_rule.py)
against a brute-force loop on hand-made score rows, select_candidates' product, and SelectResult.groups() on hand-made
arrays -- none of them loads the library."""
import math

import numpy as np
import pytest

from tests import select_rule
from tests import tune_rule

NAN, INF = float('nan'), float('inf')
LESS_THAN_HORIZON = -20
# hand-made rows: ties, NaN / inf entries, an all-NaN row, a row whose minimum is 0.0, near-ties within 5 %
ROWS = np.array([
    [3.0, 1.0, 1.0, 2.0],           # a tie at the minimum: the first
    [NAN, 2.0, INF, 1.99],          # NaN and inf skipped; 2.0 is within 5 % of 1.99
    [NAN, NAN, NAN, NAN],           # no score
    [5.0, 0.0, 0.0, 1e-300],        # minimum 0.0: only an exact 0.0 is within any finite tolerance of it
    [1.04, 1.06, 1.0, 1.05],        # 1.04 within 5 % of 1.0, first
    [1.0500000000000003, 1.0, 1.05, NAN],   # just over the 5 % threshold, then the minimum itself
    [INF, -INF, INF, INF],          # nothing finite
    [2.0, 2.0, 2.0, 2.0],           # all equal
    [7.0, NAN, NAN, NAN],           # one finite score
    [1.0, 2.0, 3.0, 4.0],           # (plan status not OK below)
])
PLAN = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, LESS_THAN_HORIZON], np.int32)
TOLERANCES = (0.0, 0.05, 1e300)


def _brute(score, plan, tol, fallback):
    best, chosen, status = [], [], []
    for row, p in zip(score, plan):
        b, st = -1, int(p)
        if p == 0:
            fin = [float(s) for s in row if math.isfinite(s)]
            if not fin:
                st = select_rule.TUNE_NO_SCORE
            else:
                thr = min(fin) * (1.0 + tol)            # Python floats are float64: one add, one multiply
                for c, s in enumerate(row):
                    if math.isfinite(s) and float(s) <= thr:
                        b = c
                        break
        best.append(b)
        chosen.append(b if b >= 0 else fallback)
        status.append(st)
    return np.array(best, np.int32), np.array(chosen, np.int32), np.array(status, np.int32)


@pytest.mark.parametrize('tol', TOLERANCES)
def test_restatement_is_the_brute_force_rule(tol):
    got = select_rule.choose(ROWS, PLAN, tol, fallback=2)
    want = _brute(ROWS, PLAN, tol, 2)
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w)


def test_hand_checked_choices():
    b0 = select_rule.choose(ROWS, PLAN, 0.0, 3)
    assert b0[0].tolist() == [1, 3, -1, 1, 2, 1, -1, 0, 0, -1]
    assert b0[1].tolist() == [1, 3, 3, 1, 2, 1, 3, 0, 0, 3]
    assert b0[2].tolist() == [0, 0, -24, 0, 0, 0, -24, 0, 0, LESS_THAN_HORIZON]
    b5 = select_rule.choose(ROWS, PLAN, 0.05, 3)[0]
    assert b5.tolist() == [1, 1, -1, 1, 0, 1, -1, 0, 0, -1]
    big = select_rule.choose(ROWS, PLAN, 1e300, 3)[0]       # every finite score is under the threshold: the first
    assert big.tolist() == [0, 1, -1, 1, 0, 0, -1, 0, 0, -1]


def test_zero_tolerance_is_tunes_first_minimum():
    rng = np.random.default_rng(5)
    score = np.concatenate([ROWS, rng.integers(0, 4, (200, 4)).astype(np.float64)])
    score[rng.random(score.shape) < 0.1] = NAN
    plan = np.concatenate([PLAN, np.where(rng.random(200) < 0.1, LESS_THAN_HORIZON, 0)]).astype(np.int32)
    best, chosen, status = select_rule.choose(score, plan, 0.0, 1)
    tb, ts = tune_rule.choose(score, plan)
    assert np.array_equal(best, tb) and np.array_equal(status, ts)
    assert np.array_equal(chosen, np.where(tb >= 0, tb, 1))


# ---- select_candidates ---------------------------------------------------------------------------------------

SEAS = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 8}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]


def test_select_candidates_product():
    from time_series_spark_amd import forecaster as fc
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    grid = {'n_changepoints': [25, 5], 'growth': ['linear', 'logistic'], 'seasonality_mode': ['additive', 'multiplicative'],
            'changepoint_prior_scale': [0.05, 0.5, 0.01]}
    cands, params = fc.select_candidates(spec, grid)
    assert len(cands) == 24 and list(params) == ['changepoint_prior_scale', 'seasonality_mode', 'growth', 'n_changepoints']
    # SELECT_AXES order, the first varying slowest
    assert params['changepoint_prior_scale'].tolist() == np.repeat([0.05, 0.5, 0.01], 8).tolist()
    assert params['seasonality_mode'].tolist() == (['additive'] * 4 + ['multiplicative'] * 4) * 3
    assert params['growth'].tolist() == (['linear'] * 2 + ['logistic'] * 2) * 6
    assert params['n_changepoints'].tolist() == [25, 5] * 12
    for c, cps, mode, growth, ncp in zip(cands, *params.values()):
        cs = c.to_c()
        assert (cs.changepoint_prior_scale, cs.n_changepoints, c.growth) == (cps, ncp, growth)
        assert cs.growth == int(growth == 'logistic')
        assert [cs.seas_mode[i] for i in range(2)] == [int(mode == 'multiplicative')] * 2
        assert c.theta_stride == 3 + ncp + 22
    cr, pr = fc.select_candidates(spec, {'changepoint_range': [0.8, 0.9]})
    assert [c.changepoint_range for c in cr] == [0.8, 0.9] and [c.to_c().changepoint_range for c in cr] == [0.8, 0.9]


def test_select_candidates_modes_of_columns():
    """seasonality_mode sets the seasonalities' and the holiday columns' mode -- over a mode they carry themselves --
    and a regressor keeps its own (the spec's default where it names none)."""
    from time_series_spark_amd import features, forecaster as fc
    hol = features.normalize_holidays([{'holiday': 'h', 'ds': [86400 * 10 ** 9 * 40], 'lower_window': 0, 'upper_window': 1}])
    names, scales, _ = features.holiday_columns(hol)
    extra = ([{'name': n, 'prior_scale': s} for n, s in zip(names, scales)]
             + [{'name': 'reg_a', 'prior_scale': 3.0}, {'name': 'reg_m', 'prior_scale': 2.0, 'mode': 'multiplicative'}])
    seas = [dict(SEAS[0], mode='additive'), SEAS[1]]
    spec = fc.ModelSpec(growth='linear', seasonalities=seas, extra=extra, holidays=hol)
    cands, params = fc.select_candidates(spec, {'seasonality_mode': ['additive', 'multiplicative']})
    n_hol = len(names)
    for c, mode in zip(cands, params['seasonality_mode']):
        cs, m = c.to_c(), int(mode == 'multiplicative')
        assert cs.n_extra == n_hol + 2
        assert [cs.seas_mode[i] for i in range(2)] == [m, m]
        assert [cs.extra_mode[i] for i in range(n_hol)] == [m] * n_hol
        assert [cs.extra_mode[n_hol], cs.extra_mode[n_hol + 1]] == [0, 1]
        assert [cs.extra_prior_scale[n_hol], cs.extra_prior_scale[n_hol + 1]] == [3.0, 2.0]


def test_select_candidates_refusals():
    from time_series_spark_amd import forecaster as fc
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    for bad in ({}, None, {'yearly_seasonality': [True]}, {'growth': []}, {'changepoint_prior_scale': []},
                {'growth': ['flat']}, {'seasonality_mode': ['both']}, {'changepoint_range': [1.5]},
                {'n_changepoints': [2.5]}, {'n_changepoints': [-1]}, {'changepoint_prior_scale': [0.0]},
                {'holidays_prior_scale': [1.0]}):
        with pytest.raises(ValueError):
            fc.select_candidates(spec, bad)
    with pytest.raises(ValueError):
        fc.select_candidates(fc.ModelSpec(changepoints=['2020-01-01'], seasonalities=SEAS), {'n_changepoints': [5]})
    cands, _ = fc.select_candidates(spec, {'growth': ['logistic']})        # (the missing cap is the call's to report)
    assert cands[0].growth == 'logistic'


# ---- SelectResult.groups() -----------------------------------------------------------------------------------

def _hand_made_result(fc, aligned):
    from time_series_spark_amd import _lib
    wide = fc.ModelSpec(growth='linear', seasonalities=SEAS)                          # stride 50
    narrow = fc.ModelSpec(growth='linear', seasonalities=SEAS[:1], n_changepoints=5)  # stride 24
    cands = [wide, narrow, wide]
    chosen = np.array([1, 0, 1, 1, 0], np.int32)
    N, stride_max = 5, 50
    theta = np.arange(N * stride_max, dtype=np.float64).reshape(N, stride_max)
    grid = np.zeros(3 if aligned else N, _lib.GRID_DTYPE)
    grid['S'] = np.arange(len(grid)) + 10
    fit = fc.FitResult(None, theta, np.arange(N) + 0.5, np.arange(N) + 0.25, np.arange(N, dtype=np.int32),
                       np.arange(N, dtype=np.int32) + 100, np.arange(N, dtype=np.int32) + 200, grid)
    return fc.SelectResult(candidates=cands, metric='rmse', score=np.zeros((N, 3)), cand_status=np.zeros((N, 3), np.int32),
                           best=np.array([1, 0, -1, 1, 0], np.int32), chosen=chosen, status=np.zeros(N, np.int32),
                           fit=fit, aligned=aligned), theta


@pytest.mark.parametrize('aligned', [True, False])
def test_groups_cut_padded_rows(aligned):
    from time_series_spark_amd import forecaster as fc
    r, theta = _hand_made_result(fc, aligned)
    gs = r.groups()
    assert [c for c, _, _ in gs] == [0, 1]              # candidate 2 chosen by nobody: no group
    want_idx = {0: [1, 4], 1: [0, 2, 3]}
    for c, idx, f in gs:
        assert idx.tolist() == want_idx[c] and f.spec is r.candidates[c]
        stride = f.spec.theta_stride
        assert stride == (50, 24)[c] and f.theta.shape == (len(idx), stride) and f.theta.flags['C_CONTIGUOUS']
        assert np.array_equal(f.theta, theta[idx, :stride])
        assert np.array_equal(f.y_scale, idx + 0.5) and np.array_equal(f.fval, idx + 0.25)
        assert np.array_equal(f.status, idx) and np.array_equal(f.n_iter, idx + 100) and np.array_equal(f.n_eval, idx + 200)
        assert f.grid['S'].tolist() == ([c + 10] if aligned else [i + 10 for i in idx])
    assert r.spec_of(2) is r.candidates[1] and r.spec_of(1) is r.candidates[0]
    fr = r.frame()
    assert list(fr.columns) == ['series', 'candidate', 'status', 'n_changepoints', 'seasonalities', 'metric', 'score']
    assert fr['candidate'].tolist() == r.chosen.tolist() and fr['n_changepoints'].tolist() == [5, 25, 5, 5, 25]
    assert fr['seasonalities'].tolist() == ['yearly', 'yearly,weekly', 'yearly', 'yearly', 'yearly,weekly']
