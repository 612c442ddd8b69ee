"""CPU tests of the fit route plan: tsf_fit_plan (include/tsf_dev.h; plan_fit in csrc/tsf_fit_plan.h) replayed against
tests/golden/fit_plan_cases.npz, which pins the decision as it stood when it was moved out of the fit driver unchanged
(tests/golden/make_fit_plan_cases.py).  Which route a call takes changes no result -- the GPU tests compare the routes
bit for bit -- so nothing but this says that a default call still takes the route it was measured on.  No GPU: the plan
is host code."""
import importlib.util
import os

import numpy as np
import pytest

from tests import helpers
from time_series_spark_amd import _lib

_spec = importlib.util.spec_from_file_location('make_fit_plan_cases',
                                               os.path.join(helpers.GOLDEN, 'make_fit_plan_cases.py'))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

# the message of every TSF_PLAN_* code, as run_fit returned it before the plan had a code for it
MESSAGES = {
    _lib.PLAN_NO_ROWS: 'no rows',
    _lib.PLAN_TOO_LONG: 'series too long (TSF_MAX_T rows per series)',
    _lib.PLAN_NEWTON_WIDE: 'Newton needs 3 + n_changepoints + K <= 128',
    _lib.PLAN_QUAD_FORM: 'eval_form QUADRATIC needs linear growth, additive columns only and history == 5',
    _lib.PLAN_QUAD_EVAL: 'the quadratic form needs an aligned panel, linear growth, additive columns only and '
                         '3 + n_changepoints + K <= 64',
    _lib.PLAN_MFMA_CHANGEPOINTS: 'residual_kernel MFMA does not take specified changepoints (changepoints_specified = 1)',
    _lib.PLAN_MFMA_SHAPE: 'residual_kernel MFMA needs an aligned panel, K <= 28 columns of one mode, 3+S+K <= 64 and S <= 28',
    _lib.PLAN_COOP_SHAPE: 'residual_kernel COOP needs a residual-form L-BFGS fit of series of at most 4096 rows',
}
# every model the plan can be asked about has at most TSF_MAX_P = 128 parameters (the spec check rejects wider ones
# first), which is all Newton's own limit asks: that message cannot be returned
UNREACHABLE = {_lib.PLAN_NEWTON_WIDE}
BOOLEANS = ['shared_grids', 'quad_ragged', 'mfma_on', 'coop', 'sparse_try', 'raw_y']


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(helpers.GOLDEN, 'fit_plan_cases.npz'))


def test_plan_library_exports(built):
    L = _lib.load()
    for sym in ('tsf_fit_plan', 'tsf_fit_plan_info_size', 'tsf_fit_plan_error', 'tsf_last_fit_plan'):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
    assert len(MESSAGES) == _lib.PLAN_COOP_SHAPE
    for code, text in MESSAGES.items():
        assert L.tsf_fit_plan_error(code).decode() == text
    assert L.tsf_fit_plan_error(_lib.PLAN_OK) == b''


def test_every_fixture_record_replays_exactly(built, fixture):
    g = fixture
    n = len(g['out_rc'])
    assert 10000 < n < 100000 and g['in_opt'].shape == (n, len(_lib.OPTIONS))
    ins = {k: g['in_' + k].tolist() for k in cases.IN_COLS}
    opts = g['in_opt'].tolist()
    want = {k: g['out_' + k].tolist() for k in ['rc'] + _lib.PLAN_FIELDS}
    bad = []
    for i in range(n):
        rec = {k: ins[k][i] for k in cases.IN_COLS}
        rc, plan = cases.run_record(rec, opts[i])
        diff = {k: (plan[k], want[k][i]) for k in _lib.PLAN_FIELDS if plan[k] != want[k][i]}
        if rc != want['rc'][i] or diff:
            bad.append((cases.MODELS[rec['model']][0], rec, opts[i], rc, want['rc'][i], diff))
    assert not bad, '%d of %d records differ (got, pinned); the first: %r' % (len(bad), n, bad[0])


def test_fixture_covers_every_route_flag_and_message(fixture):
    g = fixture
    ok = g['out_rc'] == 0
    assert set(g['out_rc'].tolist()) == {0, -1}
    assert np.all((g['out_err'] == _lib.PLAN_OK) == ok)
    assert set(g['out_route'][ok].tolist()) == set(range(_lib.ROUTE_WAVE + 1))
    for f in BOOLEANS:
        assert set(g['out_' + f][ok].tolist()) == {0, 1}, f
    for f in ('harm', 'gram_harm', 'resid_harm', 'map_harm', 'lat_U', 'quad_pre', 'bw_ns'):
        v = g['out_' + f][ok]
        assert (v == 0).any() and (v != 0).any(), f
    assert set(g['out_coop_after'][ok].tolist()) >= {-2, -1, 0}
    assert set(g['out_err'][~ok].tolist()) == set(MESSAGES) - UNREACHABLE
    # a failed plan says nothing else
    for f in _lib.PLAN_FIELDS:
        if f != 'err':
            assert not g['out_' + f][~ok].any(), f
    # the inputs the issue lists
    assert set(g['in_model'].tolist()) == set(range(len(cases.MODELS))) and len(cases.MODELS) >= 12
    assert set(g['in_call'].tolist()) == {_lib.CALL_FIT, _lib.CALL_EVAL, _lib.CALL_EVAL_QUADRATIC}
    for k, vals in (('algorithm', range(3)), ('eval_form', range(3)), ('residual_kernel', range(4)), ('converge', range(2)),
                    ('coop_after', (-1, 0)), ('n_cu', (256, 8)), ('N', (1, 3, 1000, 100000))):
        assert set(vals) <= set(g['in_' + k].tolist()), k
    assert set(cases.LENGTHS) <= set(g['in_Tm'].tolist())
    assert {1, 99, 100, 101, 768, 769, 1024, 1025, 4096, 4097, cases.MAX_T, cases.MAX_T + 1} <= set(cases.LENGTHS)
    mem = g['in_mem_avail']
    assert (mem < 0).any() and (mem >= 1 << 40).any() and ((mem >= 0) & (mem < 1 << 30)).any()
    for name, value in cases.OPTION_SETS[1:]:
        assert (g['in_opt'][:, _lib.OPTIONS.index(name)] == value).any(), (name, value)


def test_bad_arguments(built):
    s = cases.spec_for(0, 0, 0, 0, 0, -1)
    assert _lib.fit_plan(s, 0, 730)[0] == -1
    assert _lib.fit_plan(s, 5, 730, n_cu=0)[0] == -1
    bad = _lib.default_spec()           # no design column at all: the spec check's error, no plan error
    rc, plan = _lib.fit_plan(bad, 5, 730)
    assert rc == -1 and plan['err'] == _lib.PLAN_OK
