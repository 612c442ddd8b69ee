"""CPU: the numpy restatement of the calibration contracts (tests/calib_ref.py) on hand-worked cases, the finite-sample
coverage the rule promises under exchangeability, and the host-side pieces of the feature (column names, the table's
frame, the validator's `calibrate` section).  The kernels are held to the restatement in tests/test_gpu_calibrate.py."""
import numpy as np
import pytest

from tests import calib_ref as cr
from time_series_spark_amd import _lib, forecaster as fc
from time_series_spark_amd.jobs import prophet_validator as pv


def test_constants_are_the_headers():
    assert (cr.OK, cr.NO_SCORES, cr.TOO_LONG) == (_lib.CALIB_OK, _lib.CALIB_NO_SCORES, _lib.CALIB_TOO_LONG)
    assert (cr.ABS, cr.CQR) == (_lib.CALIB_ABS, _lib.CALIB_CQR) and cr.MAX_ROWS == _lib.CALIB_MAX_ROWS


def _abs(h, err, levels=(0.5,), **kw):
    """the ABS rule on errors given directly: y = err, yhat = 0"""
    err = np.asarray(err, dtype=np.float64)
    return cr.calibrate_series(h, err, np.zeros(len(err)), levels, **kw)


def test_bucket_edges_by_hand():
    # horizon 10, B = 3: w = (10 + 2) // 3 = 4; buckets (0, 4], (4, 8], (8, 10]
    h = [0, 1, 4, 5, 8, 9, 10, 11]
    e = [100., 1., 2., 3., 4., 5., 6., 200.]            # h = 0 and h = horizon + 1 are not eligible
    q, n, st = _abs(h, e, levels=(0.5,), horizon=10, n_buckets=3, min_scores=1)
    assert st == cr.OK
    assert n[:, 0].tolist() == [2, 2, 2, 6]
    # m = 2: k = ceil(3 * 0.5) = 2 -> the larger; pooled m = 6: k = ceil(7 * 0.5) = 4 -> 4.0
    assert q[:, 0].tolist() == [2., 4., 6., 4.]


def test_min_scores_boundary_and_the_maximum():
    h = np.ones(5, np.int64)
    e = [5., 1., 4., 2., 3.]
    q, n, st = _abs(h, e, levels=(0.5, 0.9), horizon=1, n_buckets=1, min_scores=5)
    # m = 5 = min_scores: level 0.5 -> k = ceil(6 * 0.5) = 3 -> 3.0; level 0.9 -> k = ceil(5.4) = 6 > m -> the maximum
    assert n.tolist() == [[5, 5], [5, 5]] and q.tolist() == [[3., 5.], [3., 5.]] and st == cr.OK
    q, n, st = _abs(h, e, levels=(0.5, 0.9), horizon=1, n_buckets=1, min_scores=6)
    assert n.tolist() == [[5, 5], [5, 5]] and np.isnan(q).all() and st == cr.NO_SCORES     # m = min_scores - 1


def test_ties_and_nan_y():
    h = np.ones(7, np.int64)
    e = [2., 2., 2., np.nan, 1., 2., 3.]
    q, n, st = _abs(h, e, levels=(0.5,), horizon=1, n_buckets=1, min_scores=1)
    # the NaN row is not live: m = 6, k = ceil(7 * 0.5) = 4 -> a = [1, 2, 2, 2, 2, 3][3]
    assert n[:, 0].tolist() == [6, 6] and q[:, 0].tolist() == [2., 2.]


def test_a_product_just_above_an_integer_takes_the_next_rank():
    # (m + 1) * level = 100 * 0.55 = 55.00000000000001 in doubles: k = 56, not 55
    assert np.float64(100) * np.float64(0.55) > 55.0
    h = np.ones(99, np.int64)
    q, n, st = _abs(h, np.arange(1., 100.), levels=(0.55,), horizon=1, n_buckets=1, min_scores=1)
    assert q[0, 0] == 56.0


def test_cqr_nan_lower_is_not_live_and_a_negative_quantile():
    h = np.ones(4, np.int64)
    y = np.array([0., 0., 0., 0.])
    lower = np.array([[-3., -2., np.nan, -4.]])
    upper = np.array([[3., 2., 1., 4.]])
    # scores fmax(lower - y, y - upper) = [-3, -2, (fmax drops the NaN: -1, but the row is not live), -4]
    q, n, st = cr.calibrate_series(h, y, np.zeros(4), (0.5,), lower, upper, mode=cr.CQR, horizon=1, n_buckets=1, min_scores=1)
    assert n[:, 0].tolist() == [3, 3]
    assert q[:, 0].tolist() == [-3., -3.]               # m = 3: k = 2 -> [-4, -3, -2][1]
    # applied: the interval narrows by 3 on each side and clamps at yhat
    yhat = np.array([[0.5, 5.0]])
    lo, hi, cell = cr.apply(yhat, np.array([1, 1]), np.array([0]), q[None], n[None], (0.5,),
                            lower=np.array([[[-4., -4.]]]), upper=np.array([[[4., 4.]]]), mode=cr.CQR, horizon=1,
                            n_buckets=1, min_scores=1)
    assert lo[0, 0].tolist() == [-1., -1.] and hi[0, 0].tolist() == [1., 5.0]      # hi clamps at yhat = 5


def test_apply_fallback_order_and_extrapolation():
    # horizon 10, B = 2: w = 5.  Bucket 0 has 3 scores, bucket 1 has 1; min_scores 2: bucket 1 falls back to the pool
    h = [1, 2, 5, 6]
    e = [1., 2., 3., 10.]
    kw = dict(horizon=10, n_buckets=2, min_scores=2)
    q, n, st = _abs(h, e, levels=(0.5,), **kw)
    assert n[:, 0].tolist() == [3, 1, 4] and q[0, 0] == 2. and np.isnan(q[1, 0]) and q[2, 0] == 3.
    q2, n2 = np.stack([q, np.full_like(q, np.nan)]), np.stack([n, np.zeros_like(n)])     # series 1: no scores at all
    yhat = np.array([[10., 10., 10., 10., 10., np.nan], [10.] * 6])
    ds = np.array([-3, 0, 5, 6, 10, 4]) + 1000          # origin 1000: h = -3, 0 (inside the history), 5, 6, 10, 4
    lo, hi, cell = cr.apply(yhat, ds, np.array([1000, 1000]), q2, n2, (0.5,), **kw)
    assert cell[0, 0].tolist() == [0, 0, 0, 2, 2, 0]
    assert lo[0, 0, :5].tolist() == [8., 8., 8., 7., 7.] and hi[0, 0, :5].tolist() == [12., 12., 12., 13., 13.]
    assert np.isnan(lo[0, 0, 5]) and np.isnan(hi[0, 0, 5])              # yhat not finite
    assert (cell[1] == -1).all() and np.isnan(lo[1]).all() and np.isnan(hi[1]).all()
    ds_far = np.array([1011, 1500])                     # beyond the calibrated horizon: the last bucket (here -> pooled)
    _, _, cell = cr.apply(np.full((1, 2), 1.), ds_far, np.array([1000]), q[None], n[None], (0.5,), **kw)
    assert cell[0, 0].tolist() == [2, 2]


def test_too_long_and_the_panel_form():
    rng = np.random.default_rng(1)
    lens = [3, 0, cr.MAX_ROWS + 1]
    off = np.concatenate([[0], np.cumsum(lens)])
    R = int(off[-1])
    h, y, yh = np.ones(R, np.int64), rng.normal(size=R), np.zeros(R)
    t = cr.calibrate_rows(off, h, y, yh, (0.8,), horizon=1, n_buckets=1, min_scores=1)
    assert t['status'].tolist() == [cr.OK, cr.NO_SCORES, cr.TOO_LONG]
    assert t['n'][:, 1, 0].tolist() == [3, 0, 0] and np.isnan(t['q'][1:]).all()
    m = cr.mask_series(t, [True, False, False])
    assert m['status'][0] == cr.NO_SCORES and np.isnan(m['q'][0]).all() and (m['n'][0] == 0).all()


def test_exchangeability_gives_the_stated_coverage():
    """2 000 series, 99 i.i.d. standard-normal errors each in one bucket, level 0.8 under ABS: k = ceil(100 * 0.8) = 80,
    so a fresh error is covered with probability exactly 80 / 100.  The covered share is Binomial(2000, 0.8) / 2000,
    sd 0.0089: it must lie in 0.8 +- 0.04.  (With default_rng(0), the errors drawn before the fresh ones, the share is 0.8075.)"""
    rng = np.random.default_rng(0)
    N, m = 2000, 99
    err = rng.standard_normal((N, m))
    fresh = rng.standard_normal(N)
    off = np.arange(N + 1, dtype=np.int64) * m
    t = cr.calibrate_rows(off, np.ones(N * m, np.int64), err.reshape(-1), np.zeros(N * m), (0.8,), horizon=1,
                          n_buckets=1, min_scores=20)
    assert (t['n'] == m).all() and (t['status'] == cr.OK).all()
    assert cr.same(t['q'][:, 0, 0], np.sort(np.abs(err), axis=1)[:, 79])
    lo, hi, _ = cr.apply(np.zeros((N, 1)), np.array([1]), np.zeros(N, np.int64), t['q'], t['n'], (0.8,), horizon=1,
                         n_buckets=1, min_scores=20)
    share = np.mean((fresh >= lo[:, 0, 0]) & (fresh <= hi[:, 0, 0]))
    print('covered share', share)
    assert abs(share - 0.8) <= 0.04


def test_calibrated_columns_names():
    assert fc.calibrated_columns([0.8, 0.95, 0.975]) == ['yhat_lower_c80', 'yhat_lower_c95', 'yhat_lower_c97.5']
    assert fc.calibrated_columns([0.5], 'q_c') == ['q_c50']
    for bad in ([], [0.0], [1.0], [0.8, 0.8], [float('nan')], [0.5] * 17):
        with pytest.raises(ValueError):
            fc.calibrated_columns(bad)


def test_frame_round_trip_bit_for_bit():
    rng = np.random.default_rng(4)
    N, B, levels = 5, 3, [0.8, 0.975]
    q = rng.normal(size=(N, B + 1, 2))
    q[1, 2, 0] = np.nan
    q[3] = np.nan
    n = rng.integers(0, 50, size=(N, B + 1, 2)).astype(np.int32)
    st = np.array([0, 0, 0, _lib.CALIB_NO_SCORES, _lib.CALIB_TOO_LONG], np.int32)
    cal = fc.Calibration(q, n, st, levels, _lib.CALIB_CQR, 10 * 86400 * 10 ** 9, B, 7)
    keys = {'series_id': np.array([7, 7, 8, 9, 11], np.int32), 'dim_id': np.array([1, 2, 1, 1, 1], np.int32)}
    df = cal.frame(keys)
    assert list(df.columns[:4]) == ['series_id', 'dim_id', 'bucket', 'horizon_upto']
    assert list(df.columns[4:8]) == ['n_c80', 'n_c97.5', 'q_c80', 'q_c97.5'] and len(df) == N * (B + 1)
    w = cal.bucket_width
    assert df['horizon_upto'].tolist()[:4] == [w, 2 * w, cal.horizon, cal.horizon]
    back, k = fc.Calibration.from_frame(df)
    assert cr.same(back.q, q) and cr.same(back.n, n) and cr.same(back.status, st)
    assert cr.same(back.levels, np.array(levels)) and (back.mode, back.horizon, back.n_buckets, back.min_scores) == \
        (cal.mode, cal.horizon, B, 7)
    assert k['series_id'].tolist() == [7, 7, 8, 9, 11] and k['dim_id'].tolist() == [1, 2, 1, 1, 1]


def test_argument_errors_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was loaded'))
    off, h, y = np.array([0, 2]), np.ones(2, np.int64), np.zeros(2)
    ok = dict(mode='abs', horizon=10, n_buckets=2, min_scores=1)
    for bad in (dict(horizon=None), dict(horizon=0), dict(mode='mad'), dict(n_buckets=0), dict(n_buckets=65),
                dict(min_scores=0), dict(mode='cqr')):
        with pytest.raises(ValueError):
            fc.calibrate_rows(off, h, y, y, [0.8], **dict(ok, **bad))
    for lv in ([], [0.0], [1.0], [0.5] * 17):
        with pytest.raises(ValueError):
            fc.calibrate_rows(off, h, y, y, lv, **ok)
    with pytest.raises(ValueError):
        fc.calibrate_rows(off, h[:1], y, y, [0.8], **ok)


def test_validator_calibrate_section():
    assert pv.calibrate_settings({}) is None
    s = pv.calibrate_settings({'calibrate': {'levels': [0.8, 0.95]}})
    assert s == dict(levels=[0.8, 0.95], mode='abs', n_buckets=10, min_scores=20)
    s = pv.calibrate_settings({'calibrate': {'levels': 0.9, 'mode': 'CQR', 'n_buckets': 4, 'min_scores': 5}})
    assert s == dict(levels=[0.9], mode='cqr', n_buckets=4, min_scores=5)
    for bad in ({'level': [0.8]}, {}, {'levels': [1.0]}, {'levels': [0.8], 'mode': 'mad'}, {'levels': [0.8], 'n_buckets': 0},
                {'levels': [0.8], 'min_scores': 0}, {'levels': [0.8], 'buckets': 3}):
        with pytest.raises(ValueError):
            pv.calibrate_settings({'calibrate': bad})
    # the section without io.calibration is refused before anything is read
    with pytest.raises(ValueError, match='io.calibration'):
        pv.ProphetValidator.check_outputs({'io': {}, 'calibrate': {'levels': [0.8]}})
    pv.ProphetValidator.check_outputs({'io': {'calibration': 'x'}, 'calibrate': {'levels': [0.8]}})
    pv.ProphetValidator.check_outputs({'io': {}})
