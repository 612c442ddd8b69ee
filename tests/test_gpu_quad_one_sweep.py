"""The one-sweep residual pass of the aligned quadratic-form kernels (ztr_sweep_harm, csrc/tsf_quad_kernels.h): rows read
as base pairs, the Fourier columns expanded in registers, the column sums accumulated in the row step that produced the
weight.  Same operands in the same order as the two-sweep table route, so every comparison here is bit for bit: the
default route against context option harm = 0 (the table route) on the same kernel variant, and against the oracle."""
import numpy as np
import pytest

from tests import helpers
from tests.helpers import n_bit_diff

pytestmark = pytest.mark.gpu

DAILY = {'name': 'daily', 'period': 1, 'fourier_order': 4}
# kernel variants of an aligned call with P <= 64 (context options): 12 waves per CU, 16 waves with n pooled table copies,
# Z^T Z in registers (what a small panel takes by default)
W12 = dict(quad_reg=0, quad_w4=0)
REG = dict(quad_reg=1)
FIELDS = ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval')


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU parity tests cannot run (product has no CPU fallback)')
    from oracle import canon_lib as cl
    cl.lib()
    return fc, cl


def _panel(N, T, seed, dtype=np.float64, step_ns=None):
    from time_series_spark_amd import synth
    ds, y = synth.make_panel(N, T, 'linear', seed=seed)
    if step_ns is not None:
        ds = synth.START_NS + step_ns * np.arange(T, dtype=np.int64)
    if dtype is np.int32:
        y = np.rint(y).astype(np.int32)
    else:
        y = y.astype(dtype)
    return ds, y


def _both_routes(fc, spec, ds, y, opts, extra=None, extra_future=None, H=20):
    """fit + predict on the default route and on the table route (harm = 0), same kernel variant -> (new, old)"""
    out = []
    step = int(ds[1] - ds[0])
    fut = ds[-1] + step * np.arange(1, H + 1)
    for o in (opts, dict(opts, harm=0)):
        with fc.get_context().options(**o):
            r = fc.fit_aligned(spec, ds, y, extra=extra)
            yhat = fc.predict(spec, r.theta, r.y_scale, r.grid, fut, extra_future=extra_future)
        out.append((r, yhat))
    return out


def _assert_same(new, old, tag):
    (r, yh), (r0, yh0) = new, old
    for name in FIELDS:
        assert np.array_equal(getattr(r, name), getattr(r0, name), equal_nan=True), (tag, name)
    assert r.grid.tobytes() == r0.grid.tobytes(), tag
    assert np.array_equal(yh, yh0, equal_nan=True), (tag, 'predict')


@pytest.mark.parametrize('n_cp', [25, 0])
@pytest.mark.parametrize('T', [730, 704, 45, 1095, 129])
def test_sweep_shapes_equal_the_table_route(env, T, n_cp):
    """Steps per lane NT = 12 with a padded last step (730), 64 x 11 exactly (704), one step with lanes that have no row
    (45), 18 steps -- the series whose weights went through global memory (1 095) --, and 129; 25 changepoints and the
    dummy changepoint of n_changepoints = 0; y as float32, int32 and float64.  On the 12-wave kernel and on the
    M-in-registers kernel."""
    fc, cl = env
    spec = fc.ModelSpec(growth='linear', n_changepoints=n_cp, seasonalities=[helpers.YEARLY, helpers.WEEKLY])
    assert helpers.uses_quadratic_form(spec)
    for dtype in (np.float32, np.int32, np.float64):
        ds, y = _panel(96, T, seed=300 + T, dtype=dtype)
        for vname, opts in (('w12', W12), ('reg', REG)):
            new, old = _both_routes(fc, spec, ds, y, opts)
            _assert_same(new, old, (T, n_cp, dtype.__name__, vname))
            assert (new[0].n_eval > 1).all(), (T, n_cp, vname)        # (every fit ran its passes)


MODELS = {
    # name -> (seasonalities, dense regressor columns, T, step between rows in hours)
    'yearly10_weekly3': ([helpers.YEARLY, helpers.WEEKLY], 0, 730, 24),
    'weekly3_daily4_subdaily': ([helpers.WEEKLY, DAILY], 0, 500, 6),
    'weekly3': ([helpers.WEEKLY], 0, 200, 24),
    'yearly10_weekly3_two_regressors': ([helpers.YEARLY, helpers.WEEKLY], 2, 730, 24),
    'weekly3_two_regressors': ([helpers.WEEKLY], 2, 200, 24),
    # no compiled harmonic shape: stays on the table route, and agrees
    'yearly5_weekly3_table_route': ([helpers.YEARLY5, helpers.WEEKLY], 0, 400, 24),
}


@pytest.mark.parametrize('model', list(MODELS))
def test_every_compiled_shape_on_every_kernel_variant(env, model):
    """Each compiled harmonic shape (28-, 16- and 8-column kernels), a Fourier model with two dense regressor columns
    behind the block (read from the table inside the sweep) and a model without a compiled shape, on the 12-wave kernel,
    the 16-wave pooled kernel with 8 / 12 / 16 table copies and the M-in-registers kernel.  The panel holds a constant
    series and a series with a non-finite value (status0 paths).  The pooled kernel on the 28-column tile (the two
    yearly10_weekly3 models) keeps the table route with either setting of harm -- 128 registers do not hold the sweep --
    so its pool8 / 12 / 16 legs compare that route with itself and with the 12-wave kernel: they pin the variant's
    results, they do not cover the new route.  From outside the library nothing tells which route a variant took."""
    fc, cl = env
    seas, n_x, T, hours = MODELS[model]
    N, H = 128, 20
    ds, y = _panel(N, T, seed=411, step_ns=hours * 3600 * 10 ** 9)
    y[5] = 7.0
    y[9, T // 2] = np.nan
    rng = np.random.default_rng(5)
    ex = rng.normal(0, 1, (n_x, T)) if n_x else None
    exf = rng.normal(0, 1, (n_x, H)) if n_x else None
    spec = fc.ModelSpec(growth='linear', seasonalities=seas, extra=[{'name': 'x%d' % e} for e in range(n_x)])
    assert helpers.uses_quadratic_form(spec)
    ref = None
    for vname, opts in (('w12', W12), ('pool8', dict(quad_reg=0, quad_w4=8)), ('pool12', dict(quad_reg=0, quad_w4=12)),
                        ('pool16', dict(quad_reg=0, quad_w4=16)), ('reg', REG)):
        new, old = _both_routes(fc, spec, ds, y, opts, extra=ex, extra_future=exf, H=H)
        _assert_same(new, old, (model, vname))
        if ref is None:
            ref = new
        _assert_same(new, ref, (model, vname, 'against the 12-wave kernel'))
    from time_series_spark_amd import _lib
    r = ref[0]
    assert r.status[5] == _lib.ST_CONSTANT and r.n_eval[5] == 0 and r.status[9] < 0
    assert (np.delete(r.n_eval, [5, 9]) > 1).all()


@pytest.mark.parametrize('variant', ['w12', 'pool16', 'reg'])
def test_many_recentrings(env, variant):
    """recenter_every = 3 and a small recenter_ratio: a fit of ~100 evaluations re-centres dozens of times, every one a
    pass over the rows."""
    fc, cl = env
    opts = {'w12': W12, 'pool16': dict(quad_reg=0, quad_w4=16), 'reg': REG}[variant]
    for seas, T in (([helpers.YEARLY, helpers.WEEKLY], 730), ([helpers.WEEKLY, DAILY], 300), ([helpers.WEEKLY], 129)):
        spec = fc.ModelSpec(growth='linear', seasonalities=seas, recenter_every=3, recenter_ratio=1e-6)
        ds, y = _panel(96, T, seed=77)
        new, old = _both_routes(fc, spec, ds, y, opts)
        _assert_same(new, old, (variant, T))
        plain = fc.fit_aligned(fc.ModelSpec(growth='linear', seasonalities=seas), ds, y)
        # (n_eval counts the passes too: a pass every third accepted iterate shows in the panel's total)
        assert new[0].n_eval.sum() > plain.n_eval.sum(), (variant, T)


@pytest.mark.parametrize('model', ['yearly10_weekly3', 'weekly3_daily4_subdaily', 'weekly3', 'yearly10_weekly3_two_regressors'])
def test_per_evaluation_new_route_against_old(env, model):
    """tsf_eval_quadratic: the residual pass at a random reference point (eval_quad_kernel takes the one-sweep route) and
    one quadratic-form evaluation at a random point around it."""
    fc, cl = env
    seas, n_x, T, hours = MODELS[model]
    N = 64
    ds, y = _panel(N, T, seed=90, step_ns=hours * 3600 * 10 ** 9)
    rng = np.random.default_rng(17)
    ex = rng.normal(0, 1, (n_x, T)) if n_x else None
    spec = fc.ModelSpec(growth='linear', seasonalities=seas, extra=[{'name': 'x%d' % e} for e in range(n_x)])
    r = fc.fit_aligned(spec, ds, y, extra=ex)
    for k in range(3):
        refs = r.theta + rng.normal(0, 0.05, r.theta.shape)
        pts = refs + rng.normal(0, 0.02 * (1 + 4 * k), refs.shape)
        f, g = fc.eval_quadratic(spec, ds, y, refs, pts, extra=ex)
        with fc.get_context().options(harm=0):
            f0, g0 = fc.eval_quadratic(spec, ds, y, refs, pts, extra=ex)
        assert np.isfinite(f).all()
        assert n_bit_diff(f, f0) == 0 and n_bit_diff(g, g0) == 0, (model, k)


def test_first_series_of_the_cfg2_shape_against_the_oracle(env):
    """T = 730, yearly 10 + weekly 3, 25 changepoints: the first 16 series on the 12-wave kernel and on the M-in-registers
    kernel against oracle.canon_lib, with the equality the parity tests use."""
    fc, cl = env
    spec = fc.ModelSpec(growth='linear', seasonalities=[helpers.YEARLY, helpers.WEEKLY])
    ds, y = _panel(96, 730, seed=300 + 730)
    csp = helpers.oracle_spec(spec)
    fut = ds[-1] + int(ds[1] - ds[0]) * np.arange(1, 21)
    oracle = [cl.fit(csp, ds, y[n], 0.0, 0.0) for n in range(16)]
    for vname, opts in (('w12', W12), ('reg', REG)):
        with fc.get_context().options(**opts):
            r = fc.fit_aligned(spec, ds, y)
            yhat = fc.predict(spec, r.theta, r.y_scale, r.grid, fut)
        for n, o in enumerate(oracle):
            assert (r.n_iter[n], r.n_eval[n], r.status[n]) == (o['n_iter'], o['n_eval'], o['status']), (vname, n)
            P = len(o['theta'])
            assert n_bit_diff(r.theta[n][:P], o['theta']) == 0 and n_bit_diff(r.fval[n], o['f']) == 0, (vname, n)
            yo, _ = cl.predict(csp, o, fut, 0.0, 0.0)
            assert np.max(np.abs(yhat[n] - yo) / np.abs(yo)) <= 1e-4, (vname, n)
