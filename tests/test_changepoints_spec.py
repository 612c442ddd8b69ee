"""CPU tests of specified changepoint dates (`Prophet(changepoints=[...])`): ModelSpec's handling of the list, its
round trips, the job config key, and the C structure behind it (no compute: no GPU here).  The GPU side is
tests/test_gpu_changepoints.py."""
import ctypes
import json

import numpy as np
import pandas as pd
import pytest

from tests import helpers
from time_series_spark_amd import _lib, forecaster as fc, panel as pk
from time_series_spark_amd.jobs import prophet_modeler as pm

DATES = ['2020-03-16', '2019-01-05T11:00:00', '2019-07-01']
NS = np.sort(np.array(DATES, dtype='datetime64[ns]').astype(np.int64))


def test_model_spec_takes_sorts_and_counts_the_dates():
    s = fc.ModelSpec(growth='linear', seasonalities=[helpers.WEEKLY], changepoints=DATES, n_changepoints=7,
                     changepoint_range=0.5)
    assert s.specified_changepoints
    assert s.changepoints.dtype == np.int64 and np.array_equal(s.changepoints, NS)
    assert s.n_changepoints == 3                                 # the list decides, as in fbprophet
    assert s.theta_stride == 3 + 3 + 6
    # every input form numpy turns into datetime64[ns], and int64 ns
    for form in (NS, NS[::-1].copy(), list(NS), pd.DatetimeIndex(NS[::-1]), np.array(DATES, dtype='datetime64[s]'),
                 [pd.Timestamp(d) for d in DATES], [pd.Timestamp(d).to_pydatetime() for d in DATES]):
        assert np.array_equal(fc.ModelSpec(changepoints=form).changepoints, NS)
    auto = fc.ModelSpec(growth='linear', seasonalities=[helpers.WEEKLY])
    assert not auto.specified_changepoints and auto.changepoints is None and auto.n_changepoints == 25
    assert 'changepoints' not in auto.to_dict()


def test_model_spec_rejects_duplicates_and_too_many_dates():
    with pytest.raises(ValueError):
        fc.ModelSpec(changepoints=['2020-01-01', '2020-02-01', '2020-01-01'])
    with pytest.raises(ValueError):
        fc.ModelSpec(changepoints=[NS[0], NS[1], NS[0]])
    day = 86400 * 10 ** 9
    assert fc.ModelSpec(changepoints=NS[0] + day * np.arange(_lib.MAX_S)).n_changepoints == _lib.MAX_S
    with pytest.raises(ValueError):
        fc.ModelSpec(changepoints=NS[0] + day * np.arange(_lib.MAX_S + 1))


def test_an_empty_list_means_no_changepoints():
    s = fc.ModelSpec(changepoints=[])
    assert s.specified_changepoints and s.n_changepoints == 0 and len(s.changepoints) == 0
    assert fc.ModelSpec.from_dict(json.loads(json.dumps(s.to_dict()))).specified_changepoints


def test_round_trips_through_dict_json_and_yaml():
    import yaml
    odd = np.concatenate([NS, [NS[-1] + 1]])                     # a date that needs all nine sub-second digits
    s = fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=[helpers.YEARLY, helpers.WEEKLY],
                     changepoints=odd, changepoint_prior_scale=0.2, max_iter=77)
    d = s.to_dict()
    assert all(isinstance(v, str) for v in d['changepoints'])
    for back in (fc.ModelSpec.from_dict(d), fc.ModelSpec.from_dict(json.loads(json.dumps(d, sort_keys=True))),
                 fc.ModelSpec.from_dict(yaml.safe_load(yaml.safe_dump(d)))):
        assert back.specified_changepoints and np.array_equal(back.changepoints, odd)
        assert back.n_changepoints == 4 and back.to_dict() == d
    # the model blob's prefix is this JSON: what the scorer rebuilds the spec from
    hb = json.loads(pk._prefix(d)[12:].decode())
    assert np.array_equal(fc.ModelSpec.from_dict(hb).changepoints, odd)
    # a blob written before the key existed
    old = {k: v for k, v in d.items() if k != 'changepoints'}
    assert not fc.ModelSpec.from_dict(old).specified_changepoints


def test_job_config_key():
    opts = pm._spec_opts({'changepoints': DATES, 'n_changepoints': 25})
    assert np.array_equal(opts['changepoints'], NS)
    assert fc.ModelSpec(**opts).n_changepoints == 3
    assert 'changepoints' not in pm._spec_opts({'n_changepoints': 5})
    with pytest.raises(ValueError):
        pm._spec_opts({'changepoints': ['2020-01-01', '2020-01-01']})
    # the range check the jobs make where fbprophet's set_changepoints raises
    day = 86400 * 10 ** 9
    ds = np.concatenate([NS[0] + day * np.arange(600), NS[0] + day * np.arange(100, 600)])
    panel = pk.PackedPanel(pd.DataFrame({'series_id': [1, 2], 'dim_id': [1, 1]}), np.array([0, 600, 1100], np.int64), ds,
                           np.ones(1100))
    pm.check_changepoints({'changepoints': [NS[0] + 100 * day, NS[0] + 599 * day]}, panel)
    pm.check_changepoints({}, panel)
    for bad in ([NS[0] + 99 * day], [NS[0] + 600 * day], [NS[0] - 1]):
        with pytest.raises(ValueError, match='Changepoints must fall within training data.'):
            pm.check_changepoints({'changepoints': bad}, panel)


def test_c_structure_and_defaults(built):
    L = _lib.load()
    assert L.tsf_spec_size() == ctypes.sizeof(_lib.TsfSpec)
    # appended after map_tol: every earlier member keeps its offset
    assert _lib.TsfSpec.changepoints_specified.offset == _lib.TsfSpec.map_tol.offset + 8
    assert _lib.TsfSpec.changepoint_ns.offset == _lib.TsfSpec.changepoints_specified.offset + 8
    assert ctypes.sizeof(_lib.TsfSpec) == _lib.TsfSpec.changepoint_ns.offset + 8 * _lib.MAX_S
    s = _lib.default_spec()
    assert s.changepoints_specified == 0 and not any(s.changepoint_ns)
    c = fc.ModelSpec(growth='linear', seasonalities=[helpers.WEEKLY], changepoints=DATES).to_c()
    assert c.changepoints_specified == 1 and c.n_changepoints == 3 and list(c.changepoint_ns)[:4] == list(NS) + [0]
    assert L.tsf_theta_stride(ctypes.byref(c)) == 3 + 3 + 6
    assert fc.ModelSpec(growth='linear', seasonalities=[helpers.WEEKLY]).to_c().changepoints_specified == 0
    assert _lib.STATUS_NAMES[_lib.ST_CHANGEPOINT] == 'CHANGEPOINT' and _lib.ST_CHANGEPOINT == -12
