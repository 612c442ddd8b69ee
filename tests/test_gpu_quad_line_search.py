"""The line search of the quadratic-form L-BFGS wave (fit_one_quad, csrc/tsf_quad_kernels.h).  On the aligned one-slot
kernels the first trial of a line search is straight-line code -- step, trial point, evaluation, g.p, then Stan's three
tests in Stan's order -- and only a first trial that is not accepted builds the bracket state and enters the loop of the
later trials (zoom, expansion, non-finite restarts).  The same kernels take the first step from cubic_interp6s, which
skips the divisions by a previous step of exactly 1 and, where c2^2 - 2 c1 c3 is negative, the square root and the roots
(the arithmetic of that alone: tests/test_cubic_interp_shortcuts.py).  No operand and no comparison may change, so everything is
bit for bit -- theta, fval, status, n_iter, n_eval -- against the oracle (oracle.canon_lib, eval_mode = 1) on every series
and every route: the 12-wave shared-M kernel, the 16-wave pooled kernel, the M-in-registers kernel and whatever the
library picks by itself at this size.  A first-trial test that takes a wrong branch changes the count of evaluations of
that series, so the comparison of n_eval and n_iter series by series is the check of the branches.

Panel: synth.make_panel(256, 730, 'linear', seed=751), the first 256 series of the bench panel, the bench model (25
changepoints, yearly 10, weekly 3).  Counters in a scratch copy of the oracle (not kept: the oracle has no such output)
gave, over the first 1 500 series of that panel, 12 170 expansions, 90 566 zoom entries by the sufficient-decrease test,
6 122 by a non-negative slope and 44 935 first trials with a step below 1; 256 series keep about a sixth of each.
Small sizes: one series; 13 series on the 12-wave route (one workgroup of 12 waves: one wave takes a second series, whose
line-search state must start clean); fits that end in their first iteration (tests/regime_cases.py has no such series:
on the oracle every one of its 53 linear series runs more than three iterations under the default tolerances -- so the
tolerance of tests/test_gpu_quad_termination.py's 'sqrt_grad_at_once' ends them, and max_iter = 1)."""
import numpy as np
import pytest

from tests import helpers
from tests.helpers import n_bit_diff

pytestmark = pytest.mark.gpu

ROUTES = {'w12': dict(quad_reg=0, quad_w4=0),          # 12 waves per CU, Z^T Z shared in LDS (the bench kernel)
          'pool16': dict(quad_reg=0, quad_w4=16),      # 16 waves per CU, pooled trend tables
          'reg': dict(quad_reg=1),                     # Z^T Z in registers
          'default': dict()}                           # the library's own choice at this size
N_PANEL = 256


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc, synth
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU parity tests cannot run (product has no CPU fallback)')
    from oracle import canon_lib as cl
    cl.lib()
    ds, y = synth.make_panel(N_PANEL, 730, 'linear', seed=751)
    return fc, cl, ds, y


def _spec(fc, **opts):
    spec = fc.ModelSpec(growth='linear', seasonality_mode='additive', n_changepoints=25,
                        seasonalities=[helpers.YEARLY, helpers.WEEKLY], **opts)
    assert helpers.uses_quadratic_form(spec)
    return spec


_oracle = {}


def _oracle_fits(env, n, **opts):
    """The oracle's fits of the first n series under L-BFGS options `opts`: computed once, shared."""
    fc, cl, ds, y = env
    key = tuple(sorted(opts.items()))
    have = _oracle.setdefault(key, [])
    if len(have) < n:
        csp = helpers.oracle_spec(_spec(fc, **opts))
        have.extend(cl.fit(csp, ds, y[i], 0.0, 0.0) for i in range(len(have), n))
    return have[:n]


def _compare(env, route, n, **opts):
    fc, cl, ds, y = env
    oracle = _oracle_fits(env, n, **opts)
    with fc.get_context().options(**ROUTES[route]):
        r = fc.fit_aligned(_spec(fc, **opts), ds, y[:n])
    bad = []
    for i, o in enumerate(oracle):
        P = len(o['theta'])
        same = ((r.status[i], r.n_iter[i], r.n_eval[i]) == (o['status'], o['n_iter'], o['n_eval'])
                and n_bit_diff(r.theta[i][:P], o['theta']) == 0 and n_bit_diff(r.fval[i], o['f']) == 0)
        if not same:
            bad.append((i, (r.status[i], r.n_iter[i], r.n_eval[i]), (o['status'], o['n_iter'], o['n_eval'])))
    assert not bad, (route, n, opts, len(bad), bad[:5])
    return oracle


@pytest.mark.parametrize('route', list(ROUTES))
def test_panel_bit_for_bit_with_the_oracle(env, route):
    oracle = _compare(env, route, N_PANEL)
    ev, it = sum(o['n_eval'] for o in oracle), sum(o['n_iter'] for o in oracle)
    print(route, 'evaluations %d, iterations %d: %.2f evaluations per line search' % (ev, it, ev / it))
    # the panel must hold line searches that go past their first trial, and many that do not
    assert 1.2 < ev / it < 2.0 and all(o['n_iter'] > 20 for o in oracle)


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('n', [1, 13])
def test_one_series_and_a_second_series_on_one_wave(env, route, n):
    _compare(env, route, n)


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('opts', [dict(tol_obj=0.0, tol_rel_obj=0.0, tol_grad=1e160, tol_rel_grad=0.0, tol_param=0.0),
                                  dict(max_iter=1)], ids=['tol_grad', 'max_iter_1'])
def test_fits_that_end_in_their_first_iteration(env, route, opts):
    """One line search per fit, from -g with the initial step: the fit's first trial is also its last evaluation unless
    that line search goes on; then a second series starts on the wave (13 series on 12 waves)."""
    oracle = _compare(env, route, 13, **opts)
    assert all(o['n_iter'] == 1 for o in oracle)

