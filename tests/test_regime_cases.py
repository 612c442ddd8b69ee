"""The CPU oracle ALONE on the regime panel (tests/regime_cases.py): what tests/test_gpu_regimes.py relies on the oracle
for is established here first -- the statuses the regimes end in, that the panel walks the branches it is for (ABSX,
RELGRAD, MAXIT, >= 40 re-centrings), the quadratic form against the residual form on every evaluation of these
trajectories (measured and recorded, not the 5 %-noise constants), one quadratic-form evaluation against the long-double
literal model within a conditioned bound whose constant is measured here, and the exact symmetries of linear growth
(negation, power-of-two scaling) bit for bit.  No GPU, no library under test."""
import numpy as np
import pytest

from oracle import canon_lib as cl
from tests import regime_cases as rc, regime_ref as rr
from tests.helpers import n_bit_diff

ABSX, RELF, RELGRAD, MAXIT, CONSTANT = 10, 21, 31, 40, 50
H = 30

_fits = {}


NEWTON_MAX_ITER = 300        # Newton fits are run with this cap: const_then_ramp would take 9 022 iterations (6 s); every
#                              other 90-row regime converges within 240, so the panel has Newton's MAXIT outcome too


def fit(name, T=rc.T_LONG, eval_mode=1, scale=1.0, newton=False):
    """The oracle's fit of a linear regime series (cached): (fit dict, forecast over H days)."""
    key = (name, T, eval_mode, scale, newton)
    if key not in _fits:
        ds, y = rc.linear(name, T)
        sp = rc.oracle_spec(T, eval_mode=eval_mode, **(dict(max_iter=NEWTON_MAX_ITER) if newton else {}))
        o = (cl.fit_newton if newton else cl.fit)(sp, ds, y * scale)
        yh = cl.predict(sp, o, ds[-1] + rc.DAY_NS * np.arange(1, H + 1))[0] if o['status'] > 0 else None
        _fits[key] = (o, yh)
    return _fits[key]


def test_the_grid_is_the_synthetic_panels():
    from time_series_spark_amd import synth
    assert rc.START_NS == synth.START_NS and np.array_equal(rc.daily_grid(17), synth.daily_grid(17))
    nm, ds, y = rc.linear_panel()
    assert len(nm) == len(set(nm)) == 53 and y.shape == (53, rc.T_LONG)
    assert len(rc.names(rc.T_SHORT)) == 32
    # deterministic, and counts where the schema holds counts
    assert np.array_equal(y, rc.linear_panel()[2])
    for n, name in enumerate(nm):
        if name.split('#')[0] in ('intermittent', 'small_counts', 'binary', 'single_spike', 'one_nonconstant', 'sign_crossing',
                                  'negative', 'step', 'const_then_ramp', 'offset_1e4', 'offset_1e6', 'offset_1e8', 'heavy_tail'):
            assert np.array_equal(y[n], np.round(y[n])), name
    z = np.mean([np.mean(rc.linear('intermittent#%d' % s)[1] == 0) for s in rc.SEEDS])
    assert 0.82 <= z <= 0.90, z


def test_every_regime_fits_in_both_forms_and_the_panel_walks_its_branches():
    """Status in {ABSX, RELF, RELGRAD, MAXIT} for every regime and both evaluation forms at both lengths, forecasts
    finite; on the quadratic form at T = 730 at least one series ends in each of ABSX, RELGRAD and MAXIT and at least
    one re-centres >= 40 times -- otherwise the panel does not exercise what it is for."""
    for T in (rc.T_LONG, rc.T_SHORT):
        for em in (1, 0):
            got = {}
            for name in rc.names(T):
                o, yh = fit(name, T, em)
                assert o['status'] in (ABSX, RELF, RELGRAD, MAXIT), (T, em, name, o['status'])
                assert np.isfinite(yh).all() and np.isfinite(o['theta']).all() and np.isfinite(o['f']), (T, em, name)
                got.setdefault(o['status'], []).append(name)
            if em == 1:
                assert {ABSX, RELGRAD, MAXIT} <= set(got), (T, sorted(got))
    rec = {name: fit(name)[0]['n_resid'] for name in rc.names()}
    assert max(rec.values()) >= 40 and sum(v >= 40 for v in rec.values()) >= 5, rec
    assert all(fit('offgrid_kink_rel_1e-6#%d' % s)[0]['status'] == MAXIT for s in rc.SEEDS)
    assert all(fit('offset_1e8#%d' % s)[0]['status'] == ABSX for s in rc.SEEDS)
    assert np.exp(max(fit('offset_1e8#%d' % s)[0]['theta'][2] for s in rc.SEEDS)) < 1e-7        # sigma ~ 4e-8 .. 8e-8
    # a constant history never reaches the optimiser
    o = cl.fit(rc.oracle_spec(), rc.daily_grid(rc.T_LONG), np.full(rc.T_LONG, 7.0))
    assert o['status'] == CONSTANT and o['n_eval'] == 0


def test_logistic_regimes_fit():
    sp = rc.oracle_spec(growth='logistic')
    long_fit = 0
    for name in rc.logistic_names():
        ds, y, floor, cap = rc.logistic(name)
        o = cl.fit(sp, ds, y, floor, cap)
        assert o['status'] in (ABSX, RELF, RELGRAD, MAXIT), (name, o['status'])
        yh = cl.predict(sp, o, ds[-1] + rc.DAY_NS * np.arange(1, H + 1), floor, cap)[0]
        assert np.isfinite(yh).all() and np.isfinite(o['theta']).all(), name
        long_fit = max(long_fit, o['n_eval'] if name == 'noiseless_sigmoid' else 0)
    # noiseless_sigmoid is the straggler of the panel (what the cooperative tail is for)
    assert long_fit >= 2000, long_fit


# cn_fit_checked on every linear regime at T = 730: the largest relative difference between the quadratic and the residual
# form along the trajectory, in f and in the gradient (2-norm).  MEASURED on this oracle, per regime the largest of its
# seeds -- recorded, not asserted against the 1e-11 / 1e-8 of the 5 %-noise family (test_oracle.py): the gradient of
# the quadratic form loses accuracy as 1 / sigma^2 grows.  The oracle is deterministic; the test allows 2 x the record.
CHECKED_DF_DG = {       # regime: (df, dg)
    'intermittent':            (3.5e-16, 4.3e-14),
    'small_counts':            (9.9e-16, 1.9e-13),
    'binary':                  (4.4e-15, 2.8e-14),
    'single_spike':            (6.3e-16, 2.2e-13),
    'one_nonconstant':         (9.9e-13, 3.2e-10),
    'sign_crossing':           (1.1e-14, 9.1e-12),
    'negative':                (1.3e-13, 3.7e-11),
    'step':                    (1.5e-12, 3.9e-12),
    'const_then_ramp':         (2.7e-12, 1.1e-08),
    'offset_1e4':              (4.1e-12, 5.2e-08),
    'offset_1e6':              (9.0e-11, 4.3e-06),
    'offset_1e8':              (6.8e-10, 3.0e-05),
    'in_model_rel_1e-3':       (1.3e-12, 7.7e-09),
    'in_model_rel_1e-5':       (2.3e-12, 9.3e-08),
    'in_model_rel_1e-7':       (3.4e-12, 7.7e-08),
    'in_model_rel_1e-9':       (2.4e-12, 1.2e-07),
    'in_model_rel_0':          (5.3e-11, 8.8e-08),
    'offgrid_kink_rel_1e-6':   (2.8e-13, 4.6e-08),
    'heavy_tail':              (1.1e-14, 9.8e-12),
    'tiny_1e-300':             (5.3e-15, 1.1e-11),
    'huge_1e300':              (4.2e-15, 7.0e-12),
}


def test_quadratic_against_residual_form_along_every_regime_trajectory():
    worst = {}
    for name in rc.names():
        ds, y = rc.linear(name)
        o, df, dg = cl.fit_checked(rc.oracle_spec(), ds, y)
        ref = fit(name)[0]
        assert (o['status'], o['n_iter'], o['n_eval']) == (ref['status'], ref['n_iter'], ref['n_eval']), name
        assert n_bit_diff(o['theta'], ref['theta']) == 0, name
        reg = name.split('#')[0]
        w = worst.setdefault(reg, [0.0, 0.0])
        w[0], w[1] = max(w[0], df), max(w[1], dg)
    print({k: ('%.1e' % v[0], '%.1e' % v[1]) for k, v in worst.items()})
    for reg, (df, dg) in worst.items():
        rdf, rdg = CHECKED_DF_DG[reg]
        assert df <= 2 * rdf and dg <= 2 * rdg, (reg, df, dg)
    # the statement DESIGN.md makes: 1e-11 / 1e-8 do NOT hold here
    assert worst['offset_1e8'][1] > 1e-6


# The constants of the two bounds of tests/regime_ref.py, MEASURED on cn_eval_quadratic_at over every (reference point,
# evaluation point) of every linear regime at T = 730 and T = 90 (test_conditioned_bound_constants_measured re-measures
# them): the largest ratio and the constant, the next power of two at least 4 x above it -- the margin
# forecast_ref.TOL_C was given, for a different but sound operation order.
RATIO_STATED, C_STATED = 1.10017e5, 2.0 ** 19          # (offset_1e8 at T = 90: the gradient, 1e-5 from the 50th iterate)
RATIO_ROUNDED, C_ROUNDED = 1.70108, 8.0
LOW_SIGMA = ('const_then_ramp', 'in_model_rel_1e-5#0', 'in_model_rel_1e-7#0', 'in_model_rel_1e-9#0', 'in_model_rel_0',
             'offgrid_kink_rel_1e-6#0')

_points = {}


def bound_points(name, T=rc.T_LONG):
    """[(theta_ref, theta, terms)] of a regime series: 2 reference points x 2 evaluation points (cached)."""
    if (name, T) not in _points:
        dat, th0 = rr.literal_dat(name, T)
        dl = rr.to_ld(dat)
        Z = rr.jacobian(dl)
        _points[(name, T)] = (dat, th0, [(ref, th, rr.bound_terms(dl, Z, ref, th))
                                         for ref in rr.reference_points(name, T) for th in rr.eval_points(name, ref)])
    return _points[(name, T)]


def _pow2_above(x):
    return 2.0 ** int(np.ceil(np.log2(4.0 * x)))


def test_conditioned_bound_constants_measured():
    assert np.finfo(rr.LD).eps < 1e-18           # the judge needs an extended long double
    worst = np.zeros(2)
    resid = np.zeros(2)
    for T in (rc.T_LONG, rc.T_SHORT):
        sp = rc.oracle_spec(T)
        for name in rc.names(T):
            ds, y = rc.linear(name, T)
            for ref, th, terms in bound_points(name, T)[2]:
                f, g, code = cl.eval_quadratic_at(sp, ds, y, ref, th)
                assert code == 0
                worst = np.maximum(worst, rr.ratios(f, g, terms))
                f, g, code = cl.eval_at(sp, ds, y, th)
                resid = np.maximum(resid, rr.ratios(f, g, terms))
    print('quadratic form: stated %.3g rounded %.3g; residual form: stated %.3g rounded %.3g' % (*worst, *resid))
    assert worst[0] <= 1.001 * RATIO_STATED and worst[1] <= 1.001 * RATIO_ROUNDED, worst
    assert C_STATED == _pow2_above(RATIO_STATED) and C_ROUNDED == _pow2_above(RATIO_ROUNDED)
    # a different but sound order -- the oracle's own residual form -- passes the rounded bound with the same constant
    assert resid[1] <= C_ROUNDED, resid


def test_conditioned_bound_is_not_vacuous():
    """The same quadratic form in float64 numpy around fbprophet's INITIAL point (never re-centred) misses both bounds
    on the low-sigma regimes, at the point 1e-5 from the fit's end point."""
    for name in LOW_SIGMA:
        dat, th0, pts = bound_points(name)
        ref, th, terms = pts[2]
        f, g = rr.numpy_quadratic_form(dat, th0, th)
        r = rr.ratios(f, g, terms)
        print(name, 'never re-centred: stated %.3g rounded %.3g' % r)
        assert r[0] > C_STATED and r[1] > C_ROUNDED, (name, r)
        # ... and, re-centred at the reference point, the same numpy code passes
        f, g = rr.numpy_quadratic_form(dat, ref, th)
        r = rr.ratios(f, g, terms)
        assert r[0] <= C_STATED and r[1] <= C_ROUNDED, (name, r)


def _negated(o):
    th = -o['theta']
    th[2] = o['theta'][2]
    return th


SYMMETRY = [(rc.T_LONG, 1, False), (rc.T_LONG, 0, False), (rc.T_SHORT, 1, False), (rc.T_SHORT, 1, True)]
# Newton (Stan's optimiser for histories below 100 rows; the T = 90 regimes): the oracle does NOT have the negation
# symmetry -- fit(-y) is an ulp or more from the negated fit(y) after the first iteration already (same counts on most
# regimes, not the same bits).  The cause is the finite-difference Hessian of cn_newton: it adds the four stencil points
# of a parameter in the fixed order -2e, -e, +e, +2e (acc = fma(w_i, -g_i, acc)), and negating a parameter maps that
# stencil onto itself REVERSED -- the same four terms summed in the opposite order round differently.  Checked on a
# scratch copy of the oracle that walks the stencil backwards for the negated parameters (all but log sigma) in the
# fit of -y: then the symmetry is exact on all 32 regime series.  The kernels add in the same order (they match the oracle bit for bit), so it stays, and
# tests/test_gpu_regimes.py leaves Newton out of its negation test.  The power-of-two scaling holds for Newton too and
# is asserted here and, on the one-series-per-wave kernel, there.
NEWTON_HAS_NEGATION_SYMMETRY = False


@pytest.mark.parametrize('T,em,newton', SYMMETRY, ids=['quadratic', 'residual', 'short_90', 'newton_90'])
def test_negation_and_power_of_two_scaling_are_exact(T, em, newton):
    """fit(-y) = (-k, -m, log sigma, -delta, -beta) with the same objective, counts and status, predict = -yhat; and
    fit(2^-20 y) = fit(y) with y_scale and the forecast scaled -- bit for bit, on every regime (IEEE negation is exact,
    fma is odd in its signed operands, absmax scaling and the priors are even; a power of two changes no mantissa)."""
    for name in rc.names(T):
        o, yh = fit(name, T, em, newton=newton)
        for scale in (-1.0, 2.0 ** -20):
            if newton and scale < 0 and not NEWTON_HAS_NEGATION_SYMMETRY:
                continue
            s, ys = fit(name, T, em, scale, newton=newton)
            assert (s['status'], s['n_iter'], s['n_eval']) == (o['status'], o['n_iter'], o['n_eval']), (name, scale)
            assert n_bit_diff(s['f'], o['f']) == 0, (name, scale)
            assert n_bit_diff(s['theta'], _negated(o) if scale < 0 else o['theta']) == 0, (name, scale)
            assert s['info'].y_scale == abs(scale) * o['info'].y_scale, (name, scale)
            assert n_bit_diff(ys, scale * yh) == 0, (name, scale)


def test_newton_oracle_negation_symmetry_is_as_recorded():
    same = True
    got = {fit(name, rc.T_SHORT, 1, newton=True)[0]['status'] for name in rc.names(rc.T_SHORT)}
    assert got == {60, MAXIT}, got                   # NEWTON_CONVERGED, and const_then_ramp at the cap
    for name in rc.names(rc.T_SHORT):
        o, _ = fit(name, rc.T_SHORT, 1, newton=True)
        s, _ = fit(name, rc.T_SHORT, 1, -1.0, newton=True)
        same = same and n_bit_diff(s['theta'], _negated(o)) == 0 and n_bit_diff(s['f'], o['f']) == 0
    assert same == NEWTON_HAS_NEGATION_SYMMETRY


def test_extreme_scales_are_the_unscaled_fit():
    """y x 2^-996 and y x 2^996 (the binades of 1e-300 and 1e300): theta of the unscaled regime bit for bit, y_scale
    scaled exactly.  tiny_1e-300 / huge_1e300 themselves are y x a power of TEN: every value is rounded once more, so
    they are fits of their own (a few ulp in y_scaled, another trajectory) -- asserted so, lest a GPU test rely on it."""
    base, _ = fit('sign_crossing#0')
    for name, (src, sc) in rc.POW2_OF.items():
        o, _ = fit(name)
        assert n_bit_diff(o['theta'], base['theta']) == 0 and o['info'].y_scale == sc * base['info'].y_scale, name
        assert (o['status'], o['n_iter'], o['n_eval']) == (base['status'], base['n_iter'], base['n_eval']) and o['f'] == base['f']
    for name in ('tiny_1e-300', 'huge_1e300'):
        o, _ = fit(name)
        assert o['status'] == RELGRAD and abs(o['f'] - base['f']) <= 1e-3 * abs(base['f'])
        assert np.max(np.abs(o['theta'] - base['theta'])) <= 0.05
