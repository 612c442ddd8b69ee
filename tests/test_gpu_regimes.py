"""The fit kernels on the regime panel (tests/regime_cases.py): histories of the kinds synth.make_panel never makes,
whose fits end in ABSX and at the iteration cap, re-centre the quadratic form 40 .. 90 times and drive sigma to 4e-8.
Everything the oracle is relied on for here is established on the oracle alone in tests/test_regime_cases.py (CPU); the
constants of the conditioned bound are measured there and imported from there.  Every panel is small."""
import numpy as np
import pytest

from tests import helpers, regime_cases as rc, regime_ref as rr, test_regime_cases as trc
from tests.helpers import n_bit_diff

pytestmark = pytest.mark.gpu

N_PANEL = 1500
H = trc.H
FIELDS = ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval')
ABSX, RELGRAD, MAXIT = 10, 31, 40


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU parity tests cannot run (product has no CPU fallback)')
    from oracle import canon_lib as cl
    cl.lib()
    return fc, cl


def _positions(n, N, seed):
    """Where n regime series go in a panel of N: 0, 63, 64, N - 1 (first and last lane of a wave, first lane of the next,
    the last work-queue slot) and scattered."""
    fixed = [0, 63, 64, N - 1]
    rest = np.setdiff1d(np.arange(N), fixed)
    pos = fixed + sorted(np.random.default_rng(seed).choice(rest, n - len(fixed), replace=False).tolist())
    return np.array(pos[:n])


_cache = {}


def _panel(T, N=N_PANEL, extra_names=()):
    """(names, positions, ds, y [N][T], spec kwargs): the linear regime series of length T embedded in a filler panel of
    synth.make_panel."""
    key = (T, N, tuple(extra_names))
    if key not in _cache:
        from time_series_spark_amd import synth
        names = rc.names(T) + list(extra_names)
        ds, y = synth.make_panel(N, T, 'linear', seed=1201 + T)
        pos = _positions(len(names), N, 5)
        for p, name in zip(pos, names):
            y[p] = rc.linear(name, T)[1]
        assert np.array_equal(ds, rc.daily_grid(T))
        _cache[key] = (names, pos, ds, y)
    return _cache[key]


def _same(a, b, tag, sub=None):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        if sub is not None:
            x, y = x[sub[0]], y[sub[1]]
        assert np.array_equal(x, y, equal_nan=True), (tag, name, np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))[:8])


def _against_oracle(fc, spec, r, names, pos, T, eval_mode, newton=False, tag=''):
    """Every regime series: theta, objective, counts, status, y_scale and the forecast, bit for bit."""
    fut = rc.daily_grid(T)[-1] + rc.DAY_NS * np.arange(1, H + 1)
    grid = r.grid if len(r.grid) == 1 else r.grid[pos]
    yh = fc.predict(spec, r.theta[pos], r.y_scale[pos], grid, fut)
    for i, (p, name) in enumerate(zip(pos, names)):
        o, yo = trc.fit(name, T, eval_mode, newton=newton)
        assert (r.status[p], r.n_iter[p], r.n_eval[p]) == (o['status'], o['n_iter'], o['n_eval']), (tag, name)
        assert n_bit_diff(r.theta[p], o['theta']) == 0 and n_bit_diff(r.fval[p], o['f']) == 0, (tag, name)
        assert r.y_scale[p] == o['info'].y_scale, (tag, name)
        assert n_bit_diff(yh[i], yo) == 0, (tag, name)


def _walks_the_branches(names, T, eval_mode):
    """The oracle's outcomes on these series (what every leg is then compared with bit for bit): a fit that ends in each
    of ABSX, RELGRAD and MAXIT, and -- quadratic form -- one that re-centred >= 40 times."""
    fits = [trc.fit(name, T, eval_mode)[0] for name in names]
    assert {ABSX, RELGRAD, MAXIT} <= {o['status'] for o in fits}
    if eval_mode == 1:
        assert max(o['n_resid'] for o in fits) >= 40


# ---- bits against the oracle, every route -----------------------------------------------------------------------------

QUAD_LEGS = {'default': {}, 'reg': dict(quad_reg=1), 'w12': dict(quad_reg=0, quad_w4=0), 'pool16': dict(quad_reg=0, quad_w4=16),
             'pool_one_copy': dict(quad_reg=0, quad_w4=1), 'w12_global_weights': dict(quad_reg=0, quad_w4=0, quad_rreg=0)}


def _spec(fc, T, **kw):
    return fc.ModelSpec(growth='linear', seasonalities=rc.seasonalities(T), **kw)


def _leg(fc, T, leg, extra_names=()):
    key = ('leg', T, leg, tuple(extra_names))
    if key not in _cache:
        names, pos, ds, y = _panel(T, extra_names=extra_names)
        with fc.get_context().options(**QUAD_LEGS[leg]):
            _cache[key] = fc.fit_aligned(_spec(fc, T), ds, y)
    return _cache[key]


@pytest.mark.parametrize('T', [rc.T_LONG, rc.T_SHORT])
@pytest.mark.parametrize('leg', list(QUAD_LEGS))
def test_quadratic_routes_on_the_regime_panel(env, leg, T):
    """The regime series among 1 500 ordinary ones on every aligned quadratic-form route (the register-M kernel, the
    12-wave kernels with the weights in registers and through global memory, the pooled 16-wave kernel with every copy
    and with one): every regime series equals the oracle bit for bit, forecast included, and every series of the panel
    equals the register-M leg.  Not every leg is a kernel of its own: at 1 500 series `default` is `reg` (the register-M
    kernel takes every call of up to 6 144 series), and at T = 90 the weights of a residual pass fit in LDS, so the launcher
    never reads quad_rreg and `w12_global_weights` is `w12` -- four distinct routes at T = 90, five at T = 730.  The
    duplicates stay: they cost 40 ms and pin the library's own choice."""
    fc, cl = env
    extra = tuple(rc.POW2_OF) if T == rc.T_LONG else ()
    names, pos, ds, y = _panel(T, extra_names=extra)
    _walks_the_branches(names, T, 1)
    r = _leg(fc, T, leg, extra)
    assert helpers.uses_quadratic_form(_spec(fc, T))
    _against_oracle(fc, _spec(fc, T), r, names, pos, T, 1, tag=leg)
    _same(r, _leg(fc, T, 'reg', extra), leg)


@pytest.mark.parametrize('T', [rc.T_LONG, rc.T_SHORT])
def test_ragged_entry_point_on_the_regime_panel(env, T):
    """fit_ragged on the same rows: the aligned fit's bits for every series, the oracle's for the regime series."""
    fc, cl = env
    names, pos, ds, y = _panel(T)
    N = len(y)
    off = T * np.arange(N + 1, dtype=np.int64)
    r = fc.fit_ragged(_spec(fc, T), off, np.tile(ds, N), y.reshape(-1))
    _against_oracle(fc, _spec(fc, T), r, names, pos, T, 1, tag='ragged')
    _same(r, _leg(fc, T, 'reg'), 'ragged')


@pytest.mark.parametrize('T', [rc.T_LONG, rc.T_SHORT])
def test_residual_form_on_the_regime_panel(env, T):
    """eval_form = RESIDUAL (the one-wave residual kernel, and the matrix-core kernel on request): the oracle's residual-form
    trajectories -- other fits than the quadratic form's: MAXIT and ABSX on other series."""
    fc, cl = env
    from time_series_spark_amd import _lib
    names, pos, ds, y = _panel(T)
    _walks_the_branches(names, T, 0)
    spec = _spec(fc, T, eval_form=_lib.EVAL_RESIDUAL, residual_kernel=_lib.RK_WAVE)
    r = fc.fit_aligned(spec, ds, y)
    _against_oracle(fc, spec, r, names, pos, T, 0, tag='residual')
    _same(fc.fit_aligned(_spec(fc, T, eval_form=_lib.EVAL_RESIDUAL, residual_kernel=_lib.RK_MFMA), ds, y), r, 'mfma')
    # the regime series alone: a small call (AUTO hands its stragglers to the cooperative kernel)
    small = fc.fit_aligned(_spec(fc, T, eval_form=_lib.EVAL_RESIDUAL), ds, y[pos])
    _same(small, r, 'residual, small call', sub=(slice(None), pos))


def test_newton_on_the_short_regime_panel(env):
    """Stan's Newton (what fbprophet runs below 100 rows) on the 90-row regimes, every regime series against
    cn_fit_newton bit for bit on both Newton kernels for this model, with the iteration cap of the CPU test, which
    const_then_ramp reaches (MAXIT inside the Newton kernels):
    * one series per wave (tsf_newton_quad.h): a call of the 32 regime series alone;
    * several series per wave (tsf_newton_batch.h): the regime series among 20 480 ordinary ones.  newton_batch_shape
      takes that kernel, with option newton_batch = 2, only from 2 x (resident workgroups per CU) x n_cu series on and
      quietly runs the other kernel below; a CU holds at most 40 one-wave workgroups and an MI355X has 256 CUs, so
      tests.test_gpu_newton._n_tiled() = 2 x 40 x 256 is above that bound whatever the occupancy (1 500 series are not);
      and once more with a 50-entry rotation list, which every decomposition overflows.
    The power-of-two scaling holds for Newton too (tests/test_regime_cases.py): fit(2^-20 y) is fit(y) with y_scale scaled.
    The negation is left out: the Newton oracle does not have it (NEWTON_HAS_NEGATION_SYMMETRY there, with the cause)."""
    fc, cl = env
    from time_series_spark_amd import _lib, synth
    from tests.test_gpu_newton import _n_tiled
    T, N = rc.T_SHORT, _n_tiled()
    assert N == 20480
    names, _, ds, _ = _panel(T)
    pos = _positions(len(names), N, 7)
    _, y = synth.make_panel(N, T, 'linear', seed=1291)
    y[pos] = np.array([rc.linear(name, T)[1] for name in names])
    spec = _spec(fc, T, algorithm=_lib.ALGO_NEWTON, max_iter=trc.NEWTON_MAX_ITER)
    assert {trc.fit(name, T, 1, newton=True)[0]['status'] for name in names} == {60, MAXIT}
    one = fc.fit_aligned(spec, ds, y[pos])
    _against_oracle(fc, spec, one, names, np.arange(len(pos)), T, 1, newton=True, tag='newton, one per wave')
    with fc.get_context().options(newton_batch=2):
        big = fc.fit_aligned(spec, ds, y)
        with fc.get_context().options(newton_lcap=50):
            over = fc.fit_aligned(spec, ds, y)
    _against_oracle(fc, spec, big, names, pos, T, 1, newton=True, tag='newton, batched')
    _same(over, big, 'newton, batched, list overflow')
    _same(one, big, 'newton, one per wave / batched', sub=(slice(None), pos))
    scaled = fc.fit_aligned(spec, ds, y[pos] * 2.0 ** -20)
    for name in ('theta', 'fval', 'status', 'n_iter', 'n_eval'):
        assert np.array_equal(getattr(scaled, name), getattr(one, name)), ('newton, scaled', name)
    fut = ds[-1] + rc.DAY_NS * np.arange(1, H + 1)
    assert np.array_equal(scaled.y_scale, one.y_scale * 2.0 ** -20)
    assert n_bit_diff(fc.predict(spec, scaled.theta, scaled.y_scale, scaled.grid, fut),
                      fc.predict(spec, one.theta, one.y_scale, one.grid, fut) * 2.0 ** -20) == 0


# ---- logistic growth, multiplicative seasonality ------------------------------------------------------------------------

def _logistic_panel():
    if 'logistic' not in _cache:
        names = rc.logistic_names()
        rows = [rc.logistic(n) for n in names]
        _cache['logistic'] = (names, rows[0][0], np.array([r[1] for r in rows]), np.array([r[2] for r in rows]),
                              np.array([r[3] for r in rows]))
    return _cache['logistic']


def _logistic_oracle(cl, n, ds=None):
    names, ds0, y, floor, cap = _logistic_panel()
    key = ('logistic oracle', n, ds is None)
    if key not in _cache:
        _cache[key] = cl.fit(rc.oracle_spec(growth='logistic'), ds0 if ds is None else ds, y[n], floor[n], cap[n])
    return _cache[key]


def test_logistic_regimes_on_every_residual_kernel(env):
    """y clipped at the cap, y above the cap, counts from zero under multiplicative seasonality, a negative floor, a
    noiseless sigmoid: the one-wave kernel, the matrix-core kernel, the cooperative kernel from the first evaluation, after
    25 and after 300 (noiseless_sigmoid is the straggler that is handed over) and the default rule -- the oracle's bits."""
    fc, cl = env
    from time_series_spark_amd import _lib
    names, ds, y, floor, cap = _logistic_panel()
    kw = dict(growth='logistic', seasonality_mode='multiplicative', seasonalities=rc.seasonalities(rc.T_LONG))
    fut = ds[-1] + rc.DAY_NS * np.arange(1, H + 1)
    sp = rc.oracle_spec(growth='logistic')
    r_w = fc.fit_aligned(fc.ModelSpec(residual_kernel=_lib.RK_WAVE, **kw), ds, y, floor=floor, cap=cap)
    yh = fc.predict(fc.ModelSpec(**kw), r_w.theta, r_w.y_scale, r_w.grid, fut, floor=floor, cap=cap)
    for n, name in enumerate(names):
        o = _logistic_oracle(cl, n)
        assert (r_w.status[n], r_w.n_iter[n], r_w.n_eval[n]) == (o['status'], o['n_iter'], o['n_eval']), name
        assert n_bit_diff(r_w.theta[n], o['theta']) == 0 and n_bit_diff(r_w.fval[n], o['f']) == 0, name
        assert n_bit_diff(yh[n], cl.predict(sp, o, fut, floor[n], cap[n])[0]) == 0, name
    assert int(np.argmax(r_w.n_eval)) == names.index('noiseless_sigmoid')
    for o in (dict(residual_kernel=_lib.RK_MFMA), dict(residual_kernel=_lib.RK_COOP), dict(residual_kernel=_lib.RK_AUTO),
              dict(coop_after=25), dict(coop_after=300)):
        _same(fc.fit_aligned(fc.ModelSpec(**dict(kw, **o)), ds, y, floor=floor, cap=cap), r_w, o)


def test_logistic_regimes_with_a_calendar_per_series(env):
    """The same series in a ragged call, every series off the daily lattice by seconds of its own, so that each has a
    table of its own: read as base pairs (with and without the row prefetch) and from the tables -- the same bits, and the
    oracle's on the shifted timestamps."""
    fc, cl = env
    names, ds, y, floor, cap = _logistic_panel()
    N, T = y.shape
    spec = fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=rc.seasonalities(T))
    dsn = [ds + (17 + 101 * n) * 10 ** 9 for n in range(N)]
    off = T * np.arange(N + 1, dtype=np.int64)
    res = {}
    for tag, h in (('prefetch', 2), ('plain', 1), ('tables', 0)):
        with fc.get_context().options(harm=h):
            res[tag] = fc.fit_ragged(spec, off, np.concatenate(dsn), y.reshape(-1), floor=floor, cap=cap)
    _same(res['plain'], res['prefetch'], 'plain')
    _same(res['tables'], res['prefetch'], 'tables')
    r = res['prefetch']
    for n, name in enumerate(names):
        o = _logistic_oracle(cl, n, dsn[n])
        assert (r.status[n], r.n_iter[n], r.n_eval[n]) == (o['status'], o['n_iter'], o['n_eval']), name
        assert n_bit_diff(r.theta[n], o['theta']) == 0 and n_bit_diff(r.fval[n], o['f']) == 0, name


# ---- an independent judge, and one evaluation ---------------------------------------------------------------------------

def test_objective_at_the_returned_point_against_the_long_double_literal_model(env):
    """No oracle: fval of every regime series against prophet.stan's log-posterior in long double at the returned theta,
    within 1e-9 |f| (the bound of test_hip_fit_and_predict_against_the_literal_prophet; the CPU trajectories stay under
    2e-10).  y x 2^-996 and y x 2^996: theta of the unscaled series bit for bit, y_scale scaled exactly."""
    fc, cl = env
    extra = tuple(rc.POW2_OF)
    names, pos, ds, y = _panel(rc.T_LONG, extra_names=extra)
    r = _leg(fc, rc.T_LONG, 'default', extra)
    worst = 0.0
    for p, name in zip(pos, names):
        dat, th0 = rr.literal_dat(name)
        f_ld, _ = rr.ld_eval(rr.to_ld(dat), r.theta[p])
        rel = float(abs(rr.LD(r.fval[p]) - f_ld) / abs(f_ld))
        worst = max(worst, rel)
        assert rel <= 1e-9, (name, rel)
    print('largest |fval - f_ld| / |f_ld| over the regime series: %.2e' % worst)
    base = pos[names.index('sign_crossing#0')]
    for name, (src, sc) in rc.POW2_OF.items():
        p = pos[names.index(name)]
        assert n_bit_diff(r.theta[p], r.theta[base]) == 0 and r.y_scale[p] == sc * r.y_scale[base], name
        assert (r.fval[p], r.n_iter[p], r.n_eval[p], r.status[p]) == (r.fval[base], r.n_iter[base], r.n_eval[base], r.status[base])


@pytest.mark.parametrize('T', [rc.T_LONG, rc.T_SHORT])
def test_one_quadratic_form_evaluation_within_the_conditioned_bound(env, T):
    """fc.eval_quadratic (one gram_eval_q around a reference point) at the (reference, point) pairs of the CPU test --
    the oracle's 50th iterate and end point of each regime, points 1e-5 and 1e-3 away: within both bounds of
    tests/regime_ref.py of the long-double literal model, with the constants recorded in tests/test_regime_cases.py
    (C_STATED = 2^19, C_ROUNDED = 8), and cn_eval_quadratic_at's bits."""
    fc, cl = env
    names = rc.names(T)
    ds = rc.daily_grid(T)
    y = np.array([rc.linear(n, T)[1] for n in names])
    sp = rc.oracle_spec(T)
    pts = [trc.bound_points(n, T)[2] for n in names]
    worst = np.zeros(2)
    for k in range(4):
        refs = np.array([p[k][0] for p in pts])
        ths = np.array([p[k][1] for p in pts])
        f, g = fc.eval_quadratic(_spec(fc, T), ds, y, refs, ths)
        for n, name in enumerate(names):
            fo, go, code = cl.eval_quadratic_at(sp, ds, y[n], refs[n], ths[n])
            assert code == 0 and n_bit_diff(f[n], fo) == 0 and n_bit_diff(g[n], go) == 0, (name, k)
            ratio = rr.ratios(f[n], g[n], pts[n][k][2])
            worst = np.maximum(worst, ratio)
            assert ratio[0] <= trc.C_STATED and ratio[1] <= trc.C_ROUNDED, (name, k, ratio)
    print('largest ratio: stated %.3g (C = %g), rounded %.3g (C = %g)' % (worst[0], trc.C_STATED, worst[1], trc.C_ROUNDED))


# ---- symmetries on every series, no oracle --------------------------------------------------------------------------------

SYM_LEGS = {'default': {}, 'reg': dict(quad_reg=1), 'pool16': dict(quad_reg=0, quad_w4=16), 'w12': dict(quad_reg=0, quad_w4=0)}


@pytest.mark.parametrize('leg', list(SYM_LEGS))
def test_negation_and_power_of_two_scaling_of_a_whole_panel(env, leg):
    """Linear growth has two exact symmetries (asserted on the oracle in tests/test_regime_cases.py): fit(-y) is
    (-k, -m, log sigma, -delta, -beta) with the same objective, counts and status and predict gives -yhat; fit(2^-20 y)
    is fit(y) with y_scale and the forecast scaled.  Bit for bit for EVERY series of a 7 000 x 730 panel with the regime
    series spliced in -- where the oracle can only sample -- on the three aligned quadratic-form kernels: the register-M
    kernel (quad_reg = 1: what every call of up to 3 x 8 x n_cu = 6 144 series takes by default, the N = 1 500 panels of
    this module among them), the pooled 16-wave kernel (quad_w4 = 16: the default from 8 x 16 x n_cu = 32 768 series on)
    and the 12-wave kernel (quad_reg = 0, quad_w4 = 0).  `default` at 7 000 series IS the 12-wave kernel: the leg checks
    that the library's own choice at this size is covered, not a fourth kernel.  A lane reduction with an asymmetric
    identity, a max where a max of magnitudes is meant or a sign test on a residual breaks the symmetry."""
    fc, cl = env
    T, N = rc.T_LONG, 7000
    names, pos, ds, y = _panel(T, N)
    spec = _spec(fc, T)
    fut = ds[-1] + rc.DAY_NS * np.arange(1, H + 1)
    res = {}
    with fc.get_context().options(**SYM_LEGS[leg]):
        for tag, sc in (('y', 1.0), ('neg', -1.0), ('scaled', 2.0 ** -20)):
            r = fc.fit_aligned(spec, ds, y * sc)
            res[tag] = (r, fc.predict(spec, r.theta, r.y_scale, r.grid, fut))
    (r, yh), (rn, yhn), (rs, yhs) = res['y'], res['neg'], res['scaled']
    assert (r.status > 0).all() and {ABSX, RELGRAD, MAXIT} <= set(r.status[pos].tolist())
    sign = -np.ones(r.theta.shape[1])
    sign[2] = 1.0
    for name in FIELDS[1:]:
        assert np.array_equal(getattr(rn, name), getattr(r, name)), (leg, 'negated', name)
    assert n_bit_diff(rn.theta, r.theta * sign) == 0, (leg, 'negated theta')
    assert n_bit_diff(yhn, -yh) == 0, (leg, 'negated forecast')
    for name in ('theta', 'fval', 'status', 'n_iter', 'n_eval'):
        assert np.array_equal(getattr(rs, name), getattr(r, name)), (leg, 'scaled', name)
    assert np.array_equal(rs.y_scale, r.y_scale * 2.0 ** -20) and n_bit_diff(yhs, yh * 2.0 ** -20) == 0, (leg, 'scaled')


def test_noise_free_pair_on_every_route(env):
    """The noise-free pair of test_odd_shapes_against_oracle (120 rows, weekly model; there on the small-panel route and
    compared in theta and counts) at the two ends of a 1 500-series panel: every quadratic-form route and the residual
    form, theta, objective, counts, status and forecast against the oracle."""
    fc, cl = env
    from time_series_spark_amd import _lib, synth
    ds, pair = rc.noise_free_pair()
    T = len(ds)
    _, y = synth.make_panel(N_PANEL, T, 'linear', seed=1321)
    pos = np.array([0, N_PANEL - 1])
    y[pos] = pair
    fut = ds[-1] + rc.DAY_NS * np.arange(1, H + 1)
    ref = None
    for tag, opts, kw, em in [(k, v, {}, 1) for k, v in QUAD_LEGS.items()] + [('residual', {}, dict(eval_form=_lib.EVAL_RESIDUAL), 0)]:
        spec = _spec(fc, T, **kw)
        with fc.get_context().options(**opts):
            r = fc.fit_aligned(spec, ds, y)
        yh = fc.predict(spec, r.theta[pos], r.y_scale[pos], r.grid, fut)
        sp = rc.oracle_spec(T, eval_mode=em)
        for i, p in enumerate(pos):
            o = cl.fit(sp, ds, pair[i])
            assert (r.status[p], r.n_iter[p], r.n_eval[p]) == (o['status'], o['n_iter'], o['n_eval']), (tag, i)
            assert n_bit_diff(r.theta[p], o['theta']) == 0 and n_bit_diff(r.fval[p], o['f']) == 0, (tag, i)
            assert n_bit_diff(yh[i], cl.predict(sp, o, fut)[0]) == 0, (tag, i)
        if em == 1:
            ref = ref or r
            _same(r, ref, tag)


# ---- downstream of a degenerate fit ---------------------------------------------------------------------------------------

def test_cross_validation_across_the_constant_stretch(env):
    """cross_validate on const_then_ramp (constant for 400 rows), one_nonconstant (7 everywhere, 8 on row 486) and
    intermittent among ordinary series, horizon 60 d, period 60 d, initial 150 d: nine cutoffs on rows 189 .. 669, of
    which the early ones see only the constant part and come back TSF_ST_CONSTANT.  Every fold is fit_ragged + predict
    on its explicitly cut prefix bit for bit (the existing contract: tests/test_gpu_cv.py), the metrics are
    oracle/cv_metrics_ref.py's."""
    fc, cl = env
    from time_series_spark_amd import _lib, synth
    from tests.test_gpu_cv import _assert_metrics, _assert_same_folds, _by_hand
    T, DAY = rc.T_LONG, rc.DAY_NS
    names = ['const_then_ramp', 'one_nonconstant', 'intermittent#0']
    ds, y = synth.make_panel(7, T, 'linear', seed=1401)
    where = [1, 3, 6]
    for p, name in zip(where, names):
        y[p] = rc.linear(name)[1]
    spec = _spec(fc, T)
    cv = fc.cross_validate(spec, ds, y, 60 * DAY, 60 * DAY, 150 * DAY, intervals=True, uncertainty_samples=100, seed=3)
    assert list(cv.n_folds) == [9] * 7 and (cv.status == _lib.CV_OK).all()
    fo = cv.fold_offsets
    for p, last_constant_row in ((1, rc.CONST_ROWS - 1), (3, (2 * T) // 3 - 1)):
        hist, st = cv.hist_rows[fo[p]:fo[p + 1]], cv.fit.status[fo[p]:fo[p + 1]]
        early = hist <= last_constant_row + 1
        assert early.sum() >= 4 and (st[early] == _lib.ST_CONSTANT).all() and (st[~early] != _lib.ST_CONSTANT).all(), (p, hist, st)
        assert (st > 0).all()
    assert (cv.fit.status[fo[6]:fo[7]] != _lib.ST_CONSTANT).all()
    res, yh, lo, hi = _by_hand(fc, _lib, spec, cv, ds, y, intervals=True, n_samples=100, seed=3)
    _assert_same_folds(cv, res, yh, lo, hi)
    _assert_metrics(_lib, cv, 0.1)


def test_intervals_and_quantiles_of_degenerate_fits(env):
    """predict_intervals / predict_quantiles downstream of a sigma ~ 4e-8 fit (offset_1e8), a CONSTANT fit and the
    intermittent fit: the oracle's cn_predict_intervals bit for bit, and the contract's expression on the returned draws
    (tests/test_gpu_quantiles.py) bit for bit."""
    fc, cl = env
    from time_series_spark_amd import _lib
    from tests.test_gpu_quantiles import LEVELS, _contract
    T = rc.T_LONG
    ds = rc.daily_grid(T)
    y = np.array([rc.linear('offset_1e8#0')[1], np.full(T, 7.0), rc.linear('intermittent#0')[1]])
    spec = _spec(fc, T)
    r = fc.fit_aligned(spec, ds, y)
    assert r.status[1] == _lib.ST_CONSTANT and np.exp(r.theta[0, 2]) < 1e-7
    fut = ds[-1] + rc.DAY_NS * np.arange(1, 66)
    keys = np.array([11, 12, 13], dtype=np.int64)
    kw = dict(series_key=keys, seed=42)
    yhat, lo, hi = fc.predict_intervals(spec, r.theta, r.y_scale, r.grid, fut, uncertainty_samples=1000, interval_width=0.8, **kw)
    sp = rc.oracle_spec(T)
    for n in range(3):
        o = cl.fit(sp, ds, y[n])
        assert o['status'] == r.status[n]
        lo_o, hi_o = cl.predict_intervals(sp, o, fut, n_samples=1000, interval_width=0.8, seed=42, series_key=int(keys[n]))
        assert n_bit_diff(lo[n], lo_o) == 0 and n_bit_diff(hi[n], hi_o) == 0, n
        assert n_bit_diff(yhat[n], cl.predict(sp, o, fut)[0]) == 0, n
    for S in (257, 1000):
        q = fc.predict_quantiles(spec, r.theta, r.y_scale, r.grid, fut, LEVELS, uncertainty_samples=S, trend=True, **kw)
        draws = fc.predictive_samples(spec, r.theta, r.y_scale, r.grid, fut, uncertainty_samples=S, **kw)
        assert n_bit_diff(q.q, np.moveaxis(_contract(draws['yhat'], LEVELS), -1, 1)) == 0, S
        assert n_bit_diff(q.trend_q, np.moveaxis(_contract(draws['trend'], LEVELS), -1, 1)) == 0, S
        assert np.isfinite(q.q).all() and (np.diff(q.q, axis=1) >= 0).all(), S
    # the constant history (fbprophet: k = 0, m = y / y_scale, sigma_obs = 1e-9, no delta): the observation noise of a draw
    # is 1e-9 y_scale and its simulated trend changes are Laplace(1e-8) slopes over a future of 65 / 729 of the history --
    # both orders of magnitude below 1e-6 of the constant
    assert np.max(np.abs(draws['yhat'][1] - 7.0)) <= 7e-6


# ---- converge = MAP ---------------------------------------------------------------------------------------------------------

MAP_REGIMES = ['intermittent#0', 'single_spike#0', 'step#0', 'sign_crossing#0']
MAP_LEFT_OUT = 'offset_1e6#0'


def test_map_mode_on_the_regimes(env, tmp_path):
    """converge = MAP (computed directly for this model: map_quad_kernel; and the continuation, map_direct = 0) on
    intermittent, single_spike, step and sign_crossing against the INDEPENDENT solver (oracle/true_map.py through
    tools/true_map_solve.py --panel, in processes of its own), by test_map_mode_fit_reaches_the_true_map's criterion and
    constants: the forecasts over 90 days within 1e-4, the objectives within 1e-7 of the largest |f|, every series at the
    KKT tolerance within that test's iteration and evaluation caps, downhill from the Stan-rule fit, and the direct
    estimate no worse than the continuation's.

    LEFT OUT of the comparison with the solver: offset_1e6.  The independent solver does not meet its own KKT report on
    it: it stops with a projected gradient of 2.2e9 (its target is 1e-7) at f = -4696, where the Stan-rule fit of the
    oracle already stands at -9690 (sigma = 1e-6).  Asserted below (> 1), so that the omission ends when the solver is
    mended.  The device's MAP fit of offset_1e6 is still run and held to everything that needs no solver: downhill from
    the Stan-rule fit, within the caps, no worse than the continuation -- and ended by the KKT test or by the
    function-value test (ST_MAP_FTOL), which is what it can end by: map_tol is an ABSOLUTE 1e-7 on a gradient whose data
    term carries 1 / sigma^2 = 1e12, and a float64 gradient there is known only to u |Z_j| |a| / sigma^2 ~ 0.1 (the
    ROUNDED bound of tests/regime_ref.py, which the oracle attains within a factor 1.7), so the KKT residual cannot be
    told from zero at 1e-7.  (Measured: FTOL after 3 rounds at f = -9707.03; the Stan rule stops at -9690.65, the
    continuation in a failed line search at -9705.36.)  On the four
    regimes kept the solver reports 9e-8 .. 2e-6; as in the test this one follows, no condition is put on that report:
    a solver that stopped short shows as a forecast or an objective out of the bounds above."""
    import os
    import subprocess
    import sys
    fc, cl = env
    from time_series_spark_amd import _lib
    T, Hm = rc.T_LONG, 90
    ds = rc.daily_grid(T)
    names = MAP_REGIMES + [MAP_LEFT_OUT]
    y = np.array([rc.linear(n)[1] for n in names])
    np.savez(str(tmp_path / 'panel.npz'), ds=ds, y=y)
    out = str(tmp_path / 'true_map.npz')
    subprocess.check_call([sys.executable, os.path.join(helpers.ROOT, 'tools', 'true_map_solve.py'), 'cfg2', str(len(names)), out,
                           '--panel', str(tmp_path / 'panel.npz')], cwd=helpers.ROOT)
    z = np.load(out)
    print('projected gradient the independent solver reports:', dict(zip(names, z['kkt'])))
    assert z['kkt'][-1] > 1.0, z['kkt']
    n = len(MAP_REGIMES)
    th_true, f_true = z['theta_map'][:n], z['f_map'][:n]
    fut = ds[-1] + rc.DAY_NS * np.arange(1, Hm + 1)
    stan = fc.fit_aligned(_spec(fc, T), ds, y)
    mapf = fc.fit_aligned(_spec(fc, T, converge=_lib.CONVERGE_MAP), ds, y)
    with fc.get_context().options(map_direct=0):
        cont = fc.fit_aligned(_spec(fc, T, converge=_lib.CONVERGE_MAP), ds, y)
    print('status', mapf.status, 'n_iter', mapf.n_iter, 'n_eval', mapf.n_eval, 'continuation: status', cont.status, 'n_eval',
          cont.n_eval, 'Stan rule: n_eval', stan.n_eval)
    print('fval: Stan rule', stan.fval, 'direct', mapf.fval, 'continuation', cont.fval)
    # what needs no solver, on all five
    assert (mapf.status[:len(MAP_REGIMES)] == _lib.ST_MAP_KKT).all(), mapf.status
    assert mapf.status[-1] in (_lib.ST_MAP_KKT, _lib.ST_MAP_FTOL), mapf.status
    assert (mapf.fval <= stan.fval + 1e-9).all(), mapf.fval - stan.fval
    assert mapf.n_iter.max() <= 80 and mapf.n_eval.max() <= 400, (mapf.n_iter, mapf.n_eval)
    assert (cont.n_eval > stan.n_eval).all() and (mapf.fval <= cont.fval + 1e-7 * np.abs(cont.fval)).all(), mapf.fval - cont.fval

    def pred(th, r):
        return fc.predict(_spec(fc, T), th, r.y_scale[:n], r.grid, fut)
    y_true = pred(th_true, mapf)
    for tag, r in (('direct', mapf), ('continuation', cont)):
        rel = np.max(np.abs(pred(r.theta[:n], r) - y_true) / np.abs(y_true), axis=1)
        print(tag, 'largest relative forecast difference per regime:', dict(zip(MAP_REGIMES, rel)))
        assert rel.max() <= 1e-4, (tag, dict(zip(MAP_REGIMES, rel)))
    assert np.max(np.abs(mapf.fval[:n] - f_true)) <= 1e-7 * np.max(np.abs(f_true)), mapf.fval[:n] - f_true
