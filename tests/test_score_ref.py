"""CPU tests of the scoring contract (include/tsf.h, "scoring observed values"): the numpy restatement
(tests/score_ref.py, what tests/test_gpu_scores.py holds the kernels to bit for bit) against the sample CRPS in exact
rational arithmetic within the header's derived bound; PIT and pinball by hand on tiny rows; Scores.anomalies; the
validator's `scores` section; the argument-shape errors score_actuals raises before the library is touched."""
from fractions import Fraction

import numpy as np
import pytest

from tests import score_ref as sr
from time_series_spark_amd import _lib, forecaster as fc
from time_series_spark_amd.jobs import prophet_validator as pv


# ---- the regrouped CRPS against the exact value ----------------------------------------------------------------

def _rows():
    """(name, draws [S], y): sample counts at the padding and stride boundaries, offsets up to 1e6, heavy ties, y far
    outside the draws, y on a draw"""
    rng = np.random.default_rng(20)
    out = []
    for S in (2, 3, 4, 5, 64, 65, 255, 256, 257, 1000, 4096):
        for off in (0.0, 1.0e3, -1.0e6):
            v = off + rng.normal(0, 1 + abs(off) * 1e-3, S)
            out.append(('S%d off%g inside' % (S, off), v, off + rng.normal()))
            out.append(('S%d off%g far' % (S, off), v, off + 1.0e6))
            out.append(('S%d off%g on a draw' % (S, off), v, v[min(7, S - 1)]))
        t = np.round(rng.normal(0, 2, S))                  # a handful of distinct values
        out.append(('S%d ties' % S, t, 1.0))
        out.append(('S%d ties below' % S, t, -50.0))
        out.append(('S%d constant' % S, np.full(S, 3.25), 3.25))
        out.append(('S%d constant off' % S, np.full(S, 3.25), 7.0))
    return out


ROWS = _rows()


@pytest.mark.parametrize('k', range(len(ROWS)), ids=[r[0] for r in ROWS])
def test_restatement_within_the_derived_bound(k):
    """|crps - exact| <= 2^-53 (4 mean|v - y| + (log2(NSP) + 2) exact): derived (three roundings per term relative to
    |d|, log2(NSP) additions of non-negative numbers, one division), not measured"""
    _, v, y = ROWS[k]
    got = sr.crps_row(np.sort(v), y)
    exact = sr.crps_exact(v, y)
    assert exact >= 0
    assert abs(Fraction(float(got)) - exact) <= sr.crps_bound(v, y, exact)
    assert got >= 0.0


def test_exact_crps_is_the_textbook_double_sum():
    rng = np.random.default_rng(1)
    v, y = rng.normal(size=7), 0.3
    f = [Fraction(float(x)) for x in v]
    fy = Fraction(float(y))
    want = sum(abs(x - fy) for x in f) / 7 - sum(abs(a - b) for a in f for b in f) / (2 * 49)
    assert sr.crps_exact(v, y) == want
    # two draws by hand: {0, 2}, y = 1: mean|X - y| = 1, mean|X - X'| = (0 + 2 + 2 + 0) / 4 = 1 -> 1 - 1/2
    assert sr.crps_exact([0.0, 2.0], 1.0) == Fraction(1, 2)
    assert sr.crps_row(np.array([0.0, 2.0]), 1.0) == 0.5
    # every term of the regrouping is non-negative
    S = 5
    w = (2 * np.arange(S) - (S - 1)) / S
    assert (np.abs(w) < 1).all()


# ---- PIT and pinball by hand -------------------------------------------------------------------------------------

def test_pit_by_hand():
    two, three = np.array([1.0, 3.0]), np.array([1.0, 2.0, 4.0])
    assert sr.pit_row(two, 0.0) == 0.0 and sr.pit_row(two, 5.0) == 1.0            # below all, above all
    assert sr.pit_row(two, 2.0) == 0.5
    assert sr.pit_row(two, 1.0) == 0.25 and sr.pit_row(two, 3.0) == 0.75          # on a draw: half of it counts
    assert sr.pit_row(three, 0.5) == 0.0 and sr.pit_row(three, 9.0) == 1.0
    assert sr.pit_row(three, 2.0) == (1 + 0.5) / 3 and sr.pit_row(three, 3.0) == 2 / 3
    assert sr.pit_row(np.array([2.0, 2.0, 2.0]), 2.0) == 0.5                      # every draw a tie
    assert np.isnan(sr.pit_row(three, np.nan)) and np.isnan(sr.crps_row(three, np.nan))


def test_quantile_and_pinball_by_hand():
    v = np.array([[1.0, 2.0, 4.0]])
    assert sr.quantile(v, 0.0)[0] == 1.0 and sr.quantile(v, 1.0)[0] == 4.0 and sr.quantile(v, 0.5)[0] == 2.0
    assert sr.quantile(v, 0.75)[0] == 3.0                                         # pos 1.5: 2 + (4 - 2) * 0.5
    assert sr.quantile(np.array([[1.0, 3.0]]), 0.25)[0] == 1.5
    y = np.array([5.0, 0.0, 3.0, np.nan])
    q = np.full(4, 3.0)
    p = sr.pinball(y, q, 0.75)
    assert p[0] == 0.75 * 2.0 and p[1] == (0.75 - 1.0) * -3.0 and p[2] == 0.0 and np.isnan(p[3])
    assert (p[:3] >= 0).all()


def test_score_shapes_and_series_rule():
    rng = np.random.default_rng(3)
    draws = rng.normal(size=(3, 4, 5))
    y = rng.normal(size=(3, 4))
    y[0, 1] = np.nan
    y[2] = np.nan
    y[1, 2] = draws[1, 2, 3]
    lv = [0.0, 0.5, 1.0]
    r = sr.score(draws, y, lv)
    assert r['q'].shape == r['pinball'].shape == (3, 3, 4) and r['pit'].shape == r['crps'].shape == (3, 4)
    assert list(r['n_obs']) == [3, 4, 0] and r['n_obs'].dtype == np.int32
    assert np.isnan(r['mean_crps'][2]) and np.isnan(r['coverage'][2]).all() and np.isnan(r['mean_pinball'][2]).all()
    assert np.isnan(r['pit'][0, 1]) and np.isnan(r['crps'][0, 1]) and np.isnan(r['pinball'][0, :, 1]).all()
    assert not np.isnan(r['q']).any()
    assert r['mean_crps'][0] == ((0.0 + r['crps'][0, 0]) + r['crps'][0, 2] + r['crps'][0, 3]) / 3.0
    with np.errstate(invalid='ignore'):
        below_max = (y <= draws.max(axis=-1)).sum(axis=1)
    assert np.array_equal(r['coverage'][:2, 2], below_max[:2] / np.array([3.0, 4.0]))
    assert (np.diff(r['coverage'][:2], axis=1) >= 0).all()      # monotone in the level
    assert r['pit'][1, 2] == (np.sum(draws[1, 2] < y[1, 2]) + 0.5) / 5
    assert sr.same(r['q'][:, 0], draws.min(axis=-1)) and sr.same(r['q'][:, 2], draws.max(axis=-1))


# ---- Scores ------------------------------------------------------------------------------------------------------

def test_anomalies():
    pit = np.array([[0.0, 0.0004, 0.0005, 0.5, 0.9995, 0.9996, 1.0, np.nan]])
    s = fc.Scores(np.zeros((1, 8)), np.zeros((1, 8)), np.zeros(0), pit=pit)
    assert s.anomalies(0.001).tolist() == [[True, True, False, False, False, True, True, False]]
    assert s.anomalies(0.5).tolist() == [[True, True, True, False, True, True, True, False]]
    assert '0.5 / uncertainty_samples' in fc.Scores.anomalies.__doc__
    for bad in (0.0, 1.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            s.anomalies(bad)
    with pytest.raises(ValueError):
        fc.Scores(np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(0)).anomalies(0.1)


def test_scores_frame_columns():
    N, H, lv = 2, 3, np.array([0.1, 0.975])
    z = lambda *s: np.arange(int(np.prod(s)), dtype=np.float64).reshape(s)      # noqa: E731
    s = fc.Scores(z(N, H), z(N, H) + 1, lv, pit=z(N, H) + 2, crps=z(N, H) + 3, q=z(N, 2, H), pinball=z(N, 2, H) + 5)
    f = s.frame(1, np.arange(H, dtype=np.int64) * 86400 * 10 ** 9)
    assert list(f.columns) == ['ds', 'y', 'yhat', 'pit', 'crps', 'yhat_q10', 'pinball_q10', 'yhat_q97.5', 'pinball_q97.5']
    assert np.array_equal(f['pinball_q97.5'].values, s.pinball[1, 1]) and np.array_equal(f['yhat_q10'].values, s.q[1, 0])
    assert str(f['ds'].dtype) == 'datetime64[ns]'
    f0 = fc.Scores(z(N, H), z(N, H), np.zeros(0), pit=z(N, H), crps=z(N, H)).frame(0, np.arange(H))
    assert list(f0.columns) == ['ds', 'y', 'yhat', 'pit', 'crps']


# ---- the validator's section -------------------------------------------------------------------------------------

def test_validator_scores_section():
    assert pv.score_settings({'cv': {}}) is None
    assert pv.score_settings({'scores': {}}) == dict(quantiles=[], uncertainty_samples=1000, seed=0)
    got = pv.score_settings({'scores': {'quantiles': [0.1, 0.5, 0.975], 'uncertainty_samples': 300, 'seed': 4}})
    assert got == dict(quantiles=[0.1, 0.5, 0.975], uncertainty_samples=300, seed=4)
    assert pv.score_settings({'scores': {'quantiles': 0.5}})['quantiles'] == [0.5]
    assert pv.score_columns([0.1, 0.5, 0.975]) == ['series_id', 'dim_id', 'n_obs', 'crps', 'pinball_q10', 'pinball_q50',
                                                   'pinball_q97.5', 'coverage_q10', 'coverage_q50', 'coverage_q97.5']
    assert pv.score_columns([]) == ['series_id', 'dim_id', 'n_obs', 'crps']
    for bad in ({'quantiles': [0.5, 1.2]}, {'quantiles': [0.5, 0.5]}, {'quantiles': [float('nan')]},
                {'uncertainty_samples': 1}, {'uncertainty_samples': 4097}, {'levels': [0.5]}):
        with pytest.raises(ValueError):
            pv.score_settings({'scores': bad})


# ---- score_actuals: what is refused before the library is touched --------------------------------------------------

def test_argument_shape_errors_before_the_library(monkeypatch):
    def never(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', never)
    monkeypatch.setattr(_lib, 'default_spec', never)
    monkeypatch.setattr(fc, 'get_context', never)
    spec = fc.ModelSpec(growth='linear', n_changepoints=2, seasonalities=[], extra=[{'name': 'x'}])
    N, H = 3, 4
    ok = dict(spec=spec, theta=np.zeros((N, spec.theta_stride)), y_scale=np.ones(N), grid=np.zeros(N, _lib.GRID_DTYPE),
              ds_ns=np.arange(H, dtype=np.int64), y_obs=np.zeros((N, H)), extra_future=np.zeros((1, H)))
    inf = np.zeros((N, H))
    inf[1, 2] = -np.inf
    for change, why in ((dict(y_obs=np.zeros((N, H + 1))), 'y_obs'),
                        (dict(y_obs=np.zeros(N * H)), 'y_obs'),
                        (dict(y_obs=inf), 'infinite'),
                        (dict(theta=np.zeros((N, spec.theta_stride + 1))), 'theta'),
                        (dict(y_scale=np.ones(N + 1)), 'y_scale'),
                        (dict(grid=np.zeros(2, _lib.GRID_DTYPE)), 'grid'),
                        (dict(ds_ns=np.zeros((N + 1, H), np.int64)), 'ds'),
                        (dict(extra_future=None), 'extra_future'),
                        (dict(extra_future=np.zeros((2, H))), 'extra_future'),
                        (dict(series_key=np.arange(N + 1)), 'series_key'),
                        (dict(floor=np.zeros(N + 1)), 'broadcast'),
                        (dict(quantiles=[0.5, 1.5]), 'quantile'),
                        (dict(quantiles=np.linspace(0, 1, _lib.MAX_QUANT + 1)), 'quantile')):
        with pytest.raises(ValueError, match=why):
            fc.score_actuals(**dict(ok, **change))
    with pytest.raises(ValueError, match='need quantile levels'):
        fc._score_actuals_call(spec, ok['theta'], ok['y_scale'], ok['grid'], ok['ds_ns'], ok['y_obs'], None, None,
                               ok['extra_future'], None, 100, 0, [], ['coverage'], None)
    # a well-formed call gets past the checks, to the library
    with pytest.raises(AssertionError, match='touched'):
        fc.score_actuals(**ok)
