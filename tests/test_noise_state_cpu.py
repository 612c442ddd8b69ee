"""CPU tests around the noise state of a fitted panel: the two jobs' configuration keys (model.noise, io.noise,
forecast.noise), NoiseAR.from_frame as the inverse of frame(keys, last=True), fc.noise_lead, and the accuracy claim of
tests/test_gpu_noise_state.py's jobs test on the numpy restatements alone.  tests/test_gpu_noise_state.py holds the
device entries against the by-hand route."""
import numpy as np
import pytest

from tests import ar_ref as ar, ar_start_ref as ars
from time_series_spark_amd import _lib, forecaster as fc
from time_series_spark_amd.jobs import prophet_modeler as pm, prophet_scorer as ps

DAY = 86400 * 10 ** 9
INT_MIN = np.iinfo(np.int64).min


# ---- the configuration keys ---------------------------------------------------------------------------------------------------

def test_modeler_noise_settings():
    assert pm.noise_settings({'model': {'floor': 0}}) is None and pm.noise_settings({}) is None
    assert pm.noise_settings({'model': {'noise': {}}}) == {'phi_max': 0.95, 'min_pairs': 8}
    assert pm.noise_settings({'model': {'noise': None}}) == {'phi_max': 0.95, 'min_pairs': 8}
    got = pm.noise_settings({'model': {'noise': {'phi_max': 0.5, 'min_pairs': 3}}})
    assert got == {'phi_max': 0.5, 'min_pairs': 3} and isinstance(got['min_pairs'], int)
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['phimax'\]"):
        pm.noise_settings({'model': {'noise': {'phimax': 0.5}}})
    with pytest.raises(ValueError, match='mapping'):
        pm.noise_settings({'model': {'noise': [0.5]}})
    for bad in ({'phi_max': 1.0}, {'phi_max': -0.1}, {'min_pairs': 0}, {'min_pairs': 2.5}):
        with pytest.raises(ValueError):
            pm.noise_settings({'model': {'noise': bad}})
    with pytest.raises(ValueError, match='io.noise needs model.noise'):
        pm.check_noise_io({'io': {'noise': '/somewhere'}, 'model': {'floor': 0}})
    pm.check_noise_io({'io': {'noise': '/somewhere'}, 'model': {'noise': {}}})
    pm.check_noise_io({'io': {}, 'model': {'noise': {}}})
    with pytest.raises(ValueError, match='io.noise needs model.noise'):
        pm.ProphetModeler({'io': {'noise': '/somewhere'}, 'model': {}}).persist_noise([])
    assert list(pm._empty_noise().columns) == pm.NOISE_COLUMNS == [
        'series_id', 'dim_id', 'phi', 'phi_raw', 'n_pairs', 'scale', 'status', 'last_resid', 'last_gap', 'last_ds_ns',
        'row_step_ns']


def test_scorer_noise_settings():
    base = {'periods': 3, 'frequency': 'D'}
    assert ps.noise_settings({'forecast': base}) is None
    assert ps.noise_settings({'forecast': dict(base, noise={'table': 't'})}) == {'table': 't', 'point': True}
    assert ps.noise_settings({'forecast': dict(base, noise={'table': 't', 'point': False})}) == {'table': 't', 'point': False}
    with pytest.raises(ValueError, match='unknown key'):
        ps.noise_settings({'forecast': dict(base, noise={'table': 't', 'lead': 1})})
    with pytest.raises(ValueError, match='table'):
        ps.noise_settings({'forecast': dict(base, noise={'point': True})})
    with pytest.raises(ValueError, match='true or false'):
        ps.noise_settings({'forecast': dict(base, noise={'table': 't', 'point': 'yes'})})
    with pytest.raises(ValueError, match='mapping'):
        ps.noise_settings({'forecast': dict(base, noise='t')})
    # the three refused combinations, each before anything is read or launched (the table does not exist)
    noise = {'table': '/no/such/table'}
    with pytest.raises(ValueError, match='forecast.calibration'):
        ps.forecast_arrays({'forecast': dict(base, noise=noise, calibration='/no/such/calibration')})
    with pytest.raises(ValueError, match='forecast.components'):
        ps.forecast_arrays({'forecast': dict(base, noise=noise, components=True)})
    with pytest.raises(ValueError, match='more than one device'):
        ps.forecast_arrays({'forecast': dict(base, noise=noise), 'devices': [0, 1]})
    assert callable(ps.forecast_arrays({'forecast': dict(base, noise=noise), 'devices': [0]}))


# ---- NoiseAR.from_frame ---------------------------------------------------------------------------------------------------------

def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_from_frame_round_trip():
    est = fc.NoiseAR(np.array([0.6, 0.0, 0.95, 0.0]), np.array([0.6, np.nan, 1.3, -0.2]), np.array([199, 0, 7, 12], np.int64),
                     np.array([3.0, np.nan, 1e-300, 2.5]), np.array([_lib.AR_OK, _lib.AR_NO_PAIRS, _lib.AR_OK, _lib.AR_OK], np.int32),
                     np.array([1.5, 0.0, -2.25, 5e-324]), np.array([0, 4, 70, 0], np.int32),
                     np.array([1500000000 * 10 ** 9, INT_MIN, -1, np.iinfo(np.int64).max], np.int64))
    keys = np.array([7, 8, 9, 10])
    back = fc.NoiseAR.from_frame(est.frame(keys, last=True))
    for f in ('phi', 'phi_raw', 'n_pairs', 'scale', 'status', 'last_resid', 'last_gap', 'last_ds_ns'):
        assert _same(getattr(back, f), getattr(est, f)), f
    assert back.last_gap[1] == 4 and back.last_ds_ns[1] == INT_MIN and np.isnan(back.phi_raw[1])
    # the keys as the modeler writes them, and a frame without the dates
    frame = est.frame(keys, last=True).drop(columns=['series', 'last_ds_ns'])
    frame.insert(0, 'dim_id', keys)
    assert fc.NoiseAR.from_frame(frame).last_ds_ns is None
    with pytest.raises(ValueError, match='last_resid, last_gap'):
        fc.NoiseAR.from_frame(est.frame(keys))
    cond = back.conditioned([1, 1, 3, 2])
    assert list(cond.steps) == [1, 5, 73, 2]


# ---- fc.noise_lead --------------------------------------------------------------------------------------------------------------

def test_noise_lead_cases():
    last = np.full(8, 100 * DAY, dtype=np.int64)
    step = np.full(8, DAY, dtype=np.int64)
    days = lambda *d: np.array(d, dtype=np.int64) * DAY                            # noqa: E731
    month_ends = (np.array(['2017-01-31', '2017-02-28', '2017-03-31'], 'datetime64[ns]').astype(np.int64)
                  - np.datetime64('2017-01-30', 'ns').astype(np.int64) + 101 * DAY)
    fut = np.stack([days(101, 102, 103),           # the next day after a daily history
                    days(103, 104, 105),           # a first future row three steps on
                    days(107, 114, 121),           # weekly futures on a daily step
                    month_ends,                    # non-uniform futures
                    days(101, 102, 103),           # row_step_ns = -1 (below)
                    days(100, 101, 102),           # a first row at last_ds_ns
                    days(99, 100, 101),            # ... and before it
                    days(101, 102, 103) + DAY // 2])       # not a whole number of steps
    step[4] = -1
    lead, ok = fc.noise_lead(last, step, fut)
    assert lead.dtype == np.int64 and ok.dtype == np.bool_
    assert list(ok) == [True, True, False, False, False, False, False, False]
    assert list(lead) == [1, 3, 0, 0, 0, 0, 0, 0]
    # a shared future grid; a weekly history continued weekly; an empty series' date; a one-row future
    lead, ok = fc.noise_lead(last[:2], np.array([DAY, 7 * DAY]), days(107, 114))
    assert list(ok) == [False, True] and list(lead) == [0, 1]
    lead, ok = fc.noise_lead(np.array([INT_MIN, 100 * DAY]), np.array([DAY, DAY]), days(102))
    assert list(ok) == [False, True] and list(lead) == [0, 2]
    fc.NoiseAR(np.zeros(2), np.zeros(2), np.zeros(2, np.int64), np.zeros(2), np.zeros(2, np.int32), np.zeros(2),
               np.array([0, 3], np.int32)).conditioned(lead=np.array([1, 2]))
    with pytest.raises(ValueError):
        fc.noise_lead(last, step[:3], fut)
    with pytest.raises(ValueError):
        fc.noise_lead(last, step, fut[:3])


# ---- the accuracy claim of the jobs test, on the restatements alone -------------------------------------------------------------

def test_restatement_satisfies_the_jobs_sign_condition():
    """tests/test_gpu_noise_state.py::test_jobs_columns asserts that the pooled squared error of forecast row 0 is
    smaller corrected than uncorrected on the planted panel (seed 5, 256 series, 197 rows of history rounded to
    integers, the next row held back), on the scorer's integer column.  Here the same panel with a least-squares fit of
    the true design, the reference estimator and the reference correction, truncated as the scorer truncates: the
    condition holds on this seed before the device is asked (expectation near 1 - phi^2 = 0.64 of the noise's share)."""
    T = ars.PLANT_T - 3
    t, y_all, X = ars.planted_panel(5)
    y = np.rint(y_all[:, :T])
    fit = ars.least_squares_forecast(np.concatenate([y, y_all[:, T:]], axis=1), X, T)
    est = ar.autocorr(y, fit[:, :T])
    assert (est['status'] == ar.AR_OK).all()
    ratios, corrected = ars.accuracy_ratios(y, fit[:, :T], y_all[:, T:T + 3], fit[:, T:T + 3], est['phi'])
    held = y_all[:, T]
    se1 = float(((np.trunc(corrected[:, 0]) - held) ** 2).sum())
    se0 = float(((np.trunc(fit[:, T]) - held) ** 2).sum())
    print('restatement, pooled squared error of row 0: corrected %.1f, uncorrected %.1f (ratio %.4f, float64 ratio %.4f; '
          'mean phi %.4f)' % (se1, se0, se1 / se0, ratios[0], est['phi'].mean()))
    assert se1 < se0 and ratios[0] < 1.0
