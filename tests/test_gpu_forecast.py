"""GPU tests of the forecast path (future_design_kernel, predict_kernel with its int post-step,
interval_sample_kernel, interval_percentile_kernel) on the shape matrix of tests/forecast_cases.py:
against the extended-precision reference (oracle/forecast_ref.py) within the tolerance calibrated on CPU
(tests/test_forecast_ref.py), and bit for bit against oracle cn_predict / cn_predict_intervals."""
import numpy as np
import pytest

from oracle import forecast_ref as fr
from tests import forecast_cases as fcs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU forecast tests cannot run (product has no CPU fallback)')
    from oracle import canon_lib as cl
    cl.lib()
    return fc, cl


def _predict(fc, c, fut=None, extra=None, want_int=True):
    return fc.predict(c.spec, c.theta, c.y_scale, c.grid, c.fut if fut is None else fut, floor=c.floor, cap=c.cap,
                      extra_future=c.extra if extra is None else extra, want_int=want_int)


@pytest.mark.parametrize('name', list(fcs.CASES))
def test_forecast_shape_matrix(env, name):
    """Per case: (1) yhat within the calibrated tolerance of the extended-precision reference, (2) identical
    bits to cn_predict, (3) for a shared future grid the per-series route (futures computed in place, no
    design table) gives the same bits for the same dates, (4) yhat_int equals the reference's post-step
    (trunc toward zero as int, floor clamp, int32) except where the reference lies within tolerance of an
    integer (counted, few)."""
    fc, cl = env
    c = fcs.make(name)
    yhat, yint = _predict(fc, c)
    yref, M, D = fcs.reference(c)
    tol = fr.tolerance(M, D)
    err = np.abs(yhat.astype(np.longdouble) - yref).astype(np.float64)
    r = err / tol
    bad = np.argwhere(r > 1.0)
    assert len(bad) == 0, (name, 'max err/tol %.3g' % r.max(), [tuple(b) for b in bad[:10]])
    print('%s: %d forecasts, max err/tol %.3g' % (name, yhat.size, r.max()))
    yo = fcs.cn_predict(c)
    assert np.array_equal(yhat.view(np.int64), yo.view(np.int64)), name
    if c.shared:
        futN = np.ascontiguousarray(np.broadcast_to(c.fut, (c.N, c.H)))
        exN = None if c.extra is None else np.ascontiguousarray(np.broadcast_to(c.extra, (c.N,) + c.extra.shape))
        y2, i2 = _predict(fc, c, futN, exN)
        assert np.array_equal(yhat.view(np.int64), y2.view(np.int64)) and np.array_equal(yint, i2), name
    near = np.abs(yref - np.round(yref)).astype(np.float64) <= tol
    want, outside = fr.int_post_step(yref.astype(np.float64), c.floor)
    assert not outside.any()
    assert near.sum() <= max(2, yhat.size // 1000), near.sum()
    mism = (yint != want) & ~near
    assert not mism.any(), (name, [tuple(b) for b in np.argwhere(mism)[:10]])


def test_int_post_step_edges(env):
    """yhat_int at the edges, on forecasts the kernel computes exactly (k = m = 0, y_scale 1, one additive
    column with coefficient 1: yhat is the column's value): negative values, (-1, 0), exact integers and their
    neighbours, floors of 0, 2.5, -2.5 and -1e10, values beyond +-2^31 (saturated: the reference's int32 cast
    would fail there), over more than one pass of 64 lanes."""
    fc, cl = env
    from time_series_spark_amd import _lib
    vals = np.array([-0.5, -1.0, -1.5, -2.5, -3.7, -0.0, 0.0, 2.0, np.nextafter(3.0, 0.0), 3.0,
                     np.nextafter(-3.0, 0.0), 7.25, 2.0 ** 31 + 5, -2.0 ** 31 - 5, 2.0 ** 31 - 1, -2.0 ** 31,
                     2147483647.5, -2147483648.5, 1e300, -1e300, -0.999999])
    H = 70
    floors = np.array([0.0, 2.5, -2.5, -1e10])
    N = len(floors)
    rng = np.random.default_rng(5)
    ex = np.stack([vals[rng.permutation(H) % len(vals)] for _ in range(N)])[:, None, :]
    spec = fc.ModelSpec(growth='linear', n_changepoints=0, extra=[{'name': 'v'}])
    theta = np.tile([0.0, 0.0, 0.0, 1.0], (N, 1))
    grid = np.zeros(N, dtype=_lib.GRID_DTYPE)
    grid['start_ns'], grid['t_scale_ns'], grid['T'] = 0, fcs.DAY_NS * 365, 100
    fut = np.tile(fcs.T0 + fcs.DAY_NS * np.arange(H), (N, 1))
    yhat, yint = fc.predict(spec, theta, np.ones(N), grid, fut, floor=floors, extra_future=ex, want_int=True)
    assert np.array_equal(yhat, ex[:, 0, :])
    want, outside = fr.int_post_step(ex[:, 0, :], floors)
    assert outside.any() and np.array_equal(yint, want)
    assert (yint[0][ex[0, 0] > 2.0 ** 31] == 2 ** 31 - 1).all()


def test_predict_entries_reject_bad_grids_before_any_launch(env):
    """tsf_predict / tsf_predict_intervals check the grids they are handed (caller data): S < 0, S above the
    spec's n_changepoints (the kernel would read beta as delta), S above TSF_MAX_S (past the kernel's LDS
    tables), t_scale_ns <= 0 -- an error return with a message, nothing launched; the context stays usable."""
    fc, cl = env
    from time_series_spark_amd import _lib
    c = fcs.make('h1')
    for field, value, why in (('S', -1, 'S < 0'), ('S', 26, "n_changepoints"), ('t_scale_ns', 0, 't_scale_ns'),
                              ('t_scale_ns', -5, 't_scale_ns')):
        g = c.grid.copy()
        g[field][1] = value
        with pytest.raises(_lib.TsfError, match=r'grid\[1\].*' + why):
            fc.predict(c.spec, c.theta, c.y_scale, g, c.fut, floor=c.floor)
        with pytest.raises(_lib.TsfError, match=r'grid\[1\].*' + why):
            fc.predict_intervals(c.spec, c.theta, c.y_scale, g, c.fut, floor=c.floor, uncertainty_samples=10)
    # a spec beyond TSF_MAX_S is refused later, by the spec check; the grid check comes first
    spec = fc.ModelSpec(growth='linear', n_changepoints=70, seasonalities=c.spec.seasonalities)
    th = np.zeros((c.N, spec.theta_stride))
    g = c.grid.copy()
    g['S'][2] = 61
    with pytest.raises(_lib.TsfError, match=r'grid\[2\].*TSF_MAX_S'):
        fc.predict(spec, th, c.y_scale, g, c.fut)
    yhat, _ = _predict(fc, c)
    assert np.array_equal(yhat, fcs.cn_predict(c))


@pytest.mark.parametrize('name,n_samples,width', [
    ('iv65', 2, 0.01), ('iv65', 3, 0.99), ('iv65', 1000, 0.8), ('iv65', 4096, 0.99),
    ('iv129', 2, 0.8), ('iv129', 3, 0.01), ('iv129', 1000, 0.99), ('iv129', 4096, 0.8)])
def test_intervals_on_the_shape_subset(env, name, n_samples, width):
    """tsf_predict_intervals: its yhat is tsf_predict's bit for bit; lower / upper are cn_predict_intervals'
    bit for bit (H 65 / 129, S 0 / 60, 2 .. 4096 samples, widths 0.01 .. 0.99, unsorted per-series futures:
    the sweep restarts); lower <= upper everywhere."""
    fc, cl = env
    c = fcs.make(name)
    keys = np.arange(c.N, dtype=np.int64) * 7919 + 3
    yhat, lo, hi = fc.predict_intervals(c.spec, c.theta, c.y_scale, c.grid, c.fut, floor=c.floor, cap=c.cap,
                                        extra_future=c.extra, series_key=keys, uncertainty_samples=n_samples,
                                        interval_width=width, seed=17)
    assert np.array_equal(yhat.view(np.int64), _predict(fc, c, want_int=False).view(np.int64))
    csp = fcs.oracle_spec(c)
    for n in range(c.N):
        fitres, fut, fl, cp, ex = fcs.series_args(c, n)
        lo_o, hi_o = cl.predict_intervals(csp, fitres, fut, fl, cp, ex, n_samples=n_samples, interval_width=width,
                                          seed=17, series_key=int(keys[n]))
        assert np.array_equal(lo[n], lo_o) and np.array_equal(hi[n], hi_o), n
    assert (lo <= hi).all()
