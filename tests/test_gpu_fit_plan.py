"""GPU test that ties the CPU-tested route plan to what launches: after each of a dozen small calls, the plan the
context's last fit launch used (tsf_last_fit_plan) is, field for field, what tsf_fit_plan returns on the host for the
same model, shape, route switches and device size.  tests/test_fit_plan.py pins tsf_fit_plan itself; results never
depend on a route (the other GPU tests compare them bit for bit), so this only checks the tie.

The expected shape of a call is worked out here the way the host entry points work it out: the longest series, the
calendar classes of a ragged call (identical timestamp vectors), its timestamp lattice (gcd of the offsets from the
first timestamp, at most 2^18 points).  Memory is passed as unknown: on calls this small the plan never asks."""
import math

import numpy as np
import pytest
# at collection, before anything loads libtsf_amd.so (see tests/test_gpu_dev_entries.py)
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

N, T, T_NEWTON = 5, 130, 40
SEAS = {'bench': [helpers.YEARLY, helpers.WEEKLY], 'weekly': [helpers.WEEKLY]}


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc, synth
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: the fit plan of a launch cannot be read back (product has no CPU fallback)')
    ctx = fc.get_context()
    n_cu = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    return fc, _lib, synth, ctx, n_cu


def model(fc, name, growth='linear', **kw):
    mode = 'multiplicative' if growth == 'logistic' else 'additive'
    return fc.ModelSpec(growth=growth, seasonality_mode=mode, seasonalities=SEAS[name], n_changepoints=3, **kw)


def check(env, spec, **shape):
    """the last launch's plan against the host's for this shape"""
    fc, _lib, synth, ctx, n_cu = env
    opt = [ctx.get_option(k) for k in _lib.OPTIONS]
    rc, want = _lib.fit_plan(spec.to_c(), opt=opt, n_cu=n_cu, mem_avail=-1, **shape)
    assert rc == 0, (rc, want)
    got = _lib.last_fit_plan(ctx)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    return got


def panel(env, growth, T_=T):
    synth = env[2]
    ds, y = synth.make_panel(N, T_, growth, seed=11)
    return ds, y, (y.max(axis=1) * 1.1 if growth == 'logistic' else None)


def ragged(ds, y, cuts, jitter=False):
    """series n: the first cuts[n] rows; jitter: every series on timestamps of its own, off any common lattice"""
    off = np.concatenate([[0], np.cumsum(cuts)]).astype(np.int64)
    dss = [ds[:c] + (np.arange(c) * (2 * n + 1) if jitter else 0) for n, c in enumerate(cuts)]
    return off, np.concatenate(dss), np.concatenate([y[n][:c] for n, c in enumerate(cuts)])


def ragged_shape(off, ds):
    """what the host entry finds: calendar classes, and the lattice the timestamps lie on"""
    vecs = {ds[a:b].tobytes() for a, b in zip(off[:-1], off[1:])}
    n = len(off) - 1
    nd = len(vecs) if len(vecs) < n else 0
    g = 0
    for v in np.unique(ds - ds.min()):
        g = math.gcd(g, int(v))
    U = (int(ds.max()) - int(ds.min())) // g + 1 if g > 0 else 0
    lat = (g, U) if 0 < U <= 1 << 18 else (0, 0)
    return dict(N=n, Tm=int(np.diff(off).max()), aligned=False, classes=nd > 0, n_distinct=nd, lat_step=lat[0], lat_U=lat[1])


@pytest.mark.parametrize('name', ['bench', 'weekly'])
def test_aligned_fit(env, name):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    spec = model(fc, name)
    fc.fit_aligned(spec, ds, y)
    p = check(env, spec, N=N, Tm=T, aligned=True)
    assert p['route'] == _lib.ROUTE_QUAD_LBFGS and p['raw_y'] == 1 and p['resid_harm'] != 0


def test_newton_by_auto(env):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear', T_NEWTON)
    spec = model(fc, 'bench', algorithm=_lib.ALGO_AUTO)
    fc.fit_aligned(spec, ds, y)
    assert check(env, spec, N=N, Tm=T_NEWTON, aligned=True)['route'] == _lib.ROUTE_NEWTON_QUAD


def test_ragged_calendar_per_series(env):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    off, rds, ry = ragged(ds, y, [T, T - 7, T - 13, T - 20, T - 31], jitter=True)
    shape = ragged_shape(off, rds)
    assert shape['n_distinct'] == 0 and shape['lat_U'] == 0
    spec = model(fc, 'bench')
    fc.fit_ragged(spec, off, rds, ry)
    p = check(env, spec, **shape)
    assert p['n_grids'] == N and p['quad_ragged'] == 1 and p['gram_harm'] != 0


def test_ragged_two_shared_calendars(env):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    off, rds, ry = ragged(ds, y, [T, T - 40, T, T - 40, T])
    shape = ragged_shape(off, rds)
    assert shape['n_distinct'] == 2
    spec = model(fc, 'bench')
    fc.fit_ragged(spec, off, rds, ry)
    p = check(env, spec, **shape)
    assert p['shared_grids'] == 1 and p['n_grids'] == 2 and p['quad_pre'] == 2


def test_ragged_on_a_lattice(env):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    off, rds, ry = ragged(ds, y, [T, T - 7, T - 13, T - 20, T - 31])
    shape = ragged_shape(off, rds)
    assert shape['lat_U'] == T and shape['n_distinct'] == 0
    spec = model(fc, 'bench', eval_form=_lib.EVAL_RESIDUAL)
    fc.fit_ragged(spec, off, rds, ry)
    p = check(env, spec, **shape)
    assert p['route'] == _lib.ROUTE_WAVE and p['lat_U'] == T and p['harm'] != 0


def test_eval_and_eval_quadratic(env):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    spec = model(fc, 'bench')
    theta = np.zeros((N, spec.theta_stride))
    theta[:, 2] = 1.0               # sigma_obs
    fc.eval_aligned(spec, ds, y, theta)
    assert check(env, spec, N=N, Tm=T, aligned=True, call=_lib.CALL_EVAL)['route'] == _lib.ROUTE_WAVE
    fc.eval_quadratic(spec, ds, y, theta, theta)
    assert check(env, spec, N=N, Tm=T, aligned=True, call=_lib.CALL_EVAL_QUADRATIC)['route'] == _lib.ROUTE_QUAD_EVAL


@pytest.mark.parametrize('case', ['map', 'coop', 'mfma'])
def test_logistic_routes(env, case):
    fc, _lib = env[0], env[1]
    ds, y, cap = panel(env, 'logistic')
    kw = {'map': dict(converge=_lib.CONVERGE_MAP), 'coop': dict(residual_kernel=_lib.RK_COOP),
          'mfma': dict(residual_kernel=_lib.RK_MFMA)}[case]
    spec = model(fc, 'bench', growth='logistic', **kw)
    fc.fit_aligned(spec, ds, y, floor=np.zeros(N), cap=cap)
    p = check(env, spec, N=N, Tm=T, aligned=True)
    if case == 'map':
        assert p['route'] == _lib.ROUTE_WAVE and p['map_harm'] != 0
    elif case == 'coop':
        assert p['route'] == _lib.ROUTE_WAVE and p['coop'] == 1 and p['coop_after'] == -2
    else:
        assert p['route'] == _lib.ROUTE_MFMA and p['mfma_on'] == 1


def test_residual_form_of_the_bench_model(env):
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    spec = model(fc, 'bench', eval_form=_lib.EVAL_RESIDUAL)
    fc.fit_aligned(spec, ds, y)
    p = check(env, spec, N=N, Tm=T, aligned=True)
    assert p['route'] == _lib.ROUTE_WAVE and p['coop'] == 1 and p['harm'] != 0


def test_cross_validation_last_launch(env):
    """Default algorithm: one launch over every fold, a ragged call whose folds of one cutoff share a calendar."""
    fc, _lib = env[0], env[1]
    ds, y, _ = panel(env, 'linear')
    spec = model(fc, 'bench')
    res = fc.cross_validate(spec, ds, y, 20 * fc.DAY_NS)
    folds = int(res.n_folds[0])
    assert folds >= 2 and list(res.n_folds) == [folds] * N
    p = check(env, spec, N=N * folds, Tm=int(res.hist_rows.max()), aligned=False, classes=True, n_distinct=folds)
    assert p['n_grids'] == folds and p['quad_pre'] == folds
    grids, launches = fc.last_cv_grids()
    assert (grids, launches) == (folds, 1)
