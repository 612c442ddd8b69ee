"""GPU tests of model-structure selection (run with `-m gpu` on an MI355X): tsf_select against the library's own
cross_validate (rolling_window=1) per candidate and fit_aligned / fit_ragged per refit group, bit for bit; the choice
against the numpy rule (tests/select_rule.py); the padding of the refit rows; tune on candidates that differ in prior
scales only; the shared fold panels; specified changepoints in one candidate; a split over two contexts; refusals; a
plain-C caller.  One small panel family: 8 series of 400 daily rows, horizon 30 d, period 90 d, initial 200 d, four
candidates of theta strides 50, 50, 50 and 24."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import select_rule

pytestmark = pytest.mark.gpu
DAY = 86400 * 10 ** 9
YEARLY = {'name': 'yearly', 'period': 365.25, 'fourier_order': 8}
WEEKLY = {'name': 'weekly', 'period': 7, 'fourier_order': 3}
FIT_KEYS = ('y_scale', 'fval', 'status', 'n_iter', 'n_eval')
CV = dict(period=90 * DAY, initial=200 * DAY)
H = 30 * DAY
METRICS = ('rmse', 'mse', 'mae', 'mape')


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _candidates(fc, **opt):
    """linear / additive; linear / multiplicative; logistic / multiplicative; linear / additive, yearly only, 5
    changepoints -- from simple-to-fit to the reference's model and back to the smallest."""
    return [fc.ModelSpec(growth='linear', seasonalities=[YEARLY, WEEKLY], **opt),
            fc.ModelSpec(growth='linear', seasonality_mode='multiplicative', seasonalities=[YEARLY, WEEKLY], **opt),
            fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=[YEARLY, WEEKLY], **opt),
            fc.ModelSpec(growth='linear', seasonalities=[YEARLY], n_changepoints=5, **opt)]


def _cv_column(cv, metric):
    """cross_validate(rolling_window=1)'s single metric row per series, NaN where a series has none."""
    mo = cv.metric_offsets
    assert (np.diff(mo) <= 1).all()
    has = np.diff(mo) == 1
    want = np.full(len(cv.status), np.nan)
    want[has] = getattr(cv, metric)[mo[:-1][has]]
    return want


@pytest.fixture(scope='module')
def aligned(env):
    """The aligned panel, its four candidates, one select_model per metric (rmse with the refit) and one cross_validate
    per candidate -- computed once, read by the tests."""
    fc, _lib = env
    from time_series_spark_amd import synth
    ds, y = synth.make_panel(8, 400, 'linear', seed=77)
    cap = 1.2 * y.max(axis=1)
    cands = _candidates(fc)
    assert [c.theta_stride for c in cands] == [50, 50, 50, 24]
    rs = {m: fc.select_model(cands, ds, y, H, cap=cap, metric=m, refit=(m == 'rmse'), **CV) for m in METRICS}
    cvs = [fc.cross_validate(c, ds, y, H, cap=cap, rolling_window=1.0, **CV) for c in cands]
    plan = fc.cv_plan(ds, H, CV['period'], CV['initial'], 1.0, N=8)
    assert set(plan['n_folds'].tolist()) <= {2, 3}
    return dict(ds=ds, y=y, cap=cap, cands=cands, rs=rs, cvs=cvs, plan=plan)


def _ragged_panel():
    """Eight series cut from one 400-day panel: daily ones, ones with every second / third day (folds of under 100 rows
    beside folds of 100 and more), one of 60 rows (too short for any fold) and one of a single row."""
    from time_series_spark_amd import synth
    ds0, y0 = synth.make_panel(8, 400, 'linear', seed=78)
    cuts = [slice(None), slice(None, None, 3), slice(50, None), slice(0, 60), slice(0, 1), slice(None, None, 2),
            slice(100, None, 3), slice(None)]
    parts = [(ds0[s], y0[n][s]) for n, s in enumerate(cuts)]
    off = np.concatenate([[0], np.cumsum([len(d) for d, _ in parts])]).astype(np.int64)
    return off, np.concatenate([d for d, _ in parts]).astype(np.int64), np.concatenate([v for _, v in parts])


@pytest.fixture(scope='module')
def ragged(env):
    fc, _lib = env
    off, ds, y = _ragged_panel()
    assert np.diff(off).min() == 1 and np.diff(off).max() == 400 and 60 in np.diff(off)
    cap = np.array([1.2 * y[off[n]:off[n + 1]].max() for n in range(8)])
    cands = _candidates(fc, algorithm=_lib.ALGO_AUTO)
    kw = dict(offsets=off, cap=cap, **CV)
    plan = fc.cv_plan(ds, H, CV['period'], CV['initial'], 1.0, offsets=off)
    assert (plan['hist_rows'] < 100).any() and (plan['hist_rows'] >= 100).any()
    assert plan['status'][3] != 0 and plan['status'][4] != 0 and (np.delete(plan['status'], [3, 4]) == 0).all()
    r = fc.select_model(cands, ds, y, H, fallback=2, **kw)
    return dict(off=off, ds=ds, y=y, cap=cap, cands=cands, r=r, plan=plan, kw=kw)


def test_scores_are_cross_validate_aligned(aligned):
    """Every column of score / cand_status is cross_validate's metric row and status, for each of the four metrics."""
    for m, r in aligned['rs'].items():
        assert r.score.shape == (8, 4)
        for c, cv in enumerate(aligned['cvs']):
            assert np.array_equal(r.cand_status[:, c], cv.status), (m, c)
            assert helpers.n_bit_diff(r.score[:, c], _cv_column(cv, m)) == 0, (m, c)


def test_scores_are_cross_validate_ragged(env, ragged):
    fc, _lib = env
    r = ragged['r']
    for c, sp in enumerate(ragged['cands']):
        cv = fc.cross_validate(sp, ragged['ds'], ragged['y'], H, rolling_window=1.0, **ragged['kw'])
        assert np.array_equal(r.cand_status[:, c], cv.status), c
        assert helpers.n_bit_diff(r.score[:, c], _cv_column(cv, 'rmse')) == 0, c
    assert np.isnan(r.score[[3, 4]]).all() and np.isfinite(r.score).any(axis=1).sum() == 6
    assert (r.cand_status[3] == ragged['plan']['status'][3]).all() and (r.cand_status[4] == ragged['plan']['status'][4]).all()


def test_choice_is_the_rule_and_tolerance_changes_it(env, aligned):
    """best / chosen / status are select_rule's on the returned scores; tolerances computed from the score matrix make
    the choice of at least one series move to an earlier candidate."""
    fc, _lib = env
    r0 = aligned['rs']['rmse']
    plan = aligned['plan']['status']
    sc = r0.score
    assert np.isfinite(sc).all()
    m = sc.min(axis=1)
    later = np.flatnonzero(r0.best > 0)
    assert later.size > 0                       # some series does not choose candidate 0 at tolerance 0
    # the relative excess of the best earlier candidate over the minimum, per such series
    need = np.array([sc[n, :r0.best[n]].min() / m[n] - 1.0 for n in later])
    tols = [0.0, float(need.min() * 1.001 + 1e-12), float(need.max() * 1.001 + 1e-12)]
    seen = []
    for tol in tols:
        r = r0 if tol == 0.0 else fc.select_model(aligned['cands'], aligned['ds'], aligned['y'], H, cap=aligned['cap'],
                                                  tolerance=tol, fallback=1, refit=False, **CV)
        assert helpers.n_bit_diff(r.score, sc) == 0
        best, chosen, st = select_rule.choose(r.score, plan, tol, 1 if tol else 0)
        assert np.array_equal(r.best, best) and np.array_equal(r.chosen, chosen) and np.array_equal(r.status, st), tol
        seen.append(r.best.copy())
    assert (seen[1] != seen[0]).any() and (seen[1] <= seen[0]).all()
    assert (seen[2][later] < seen[0][later]).all()


def test_choice_and_fallback_ragged(ragged):
    r = ragged['r']
    best, chosen, st = select_rule.choose(r.score, ragged['plan']['status'], 0.0, 2)
    assert np.array_equal(r.best, best) and np.array_equal(r.chosen, chosen) and np.array_equal(r.status, st)
    assert r.best[3] == -1 and r.best[4] == -1 and r.chosen[3] == 2 and r.chosen[4] == 2
    assert r.spec_of(3) is ragged['cands'][2]


def _assert_rows(r, c, sel, want, grid_want):
    """rows sel of the padded refit are FitResult want (candidate c's stride), the padding +0.0"""
    stride = r.candidates[c].theta_stride
    assert helpers.n_bit_diff(r.fit.theta[sel, :stride], want.theta) == 0, c
    pad = r.fit.theta[sel, stride:]
    assert (pad == 0.0).all() and not np.signbit(pad).any(), c
    for k in FIT_KEYS:
        g, w = getattr(r.fit, k)[sel], getattr(want, k)
        assert (helpers.n_bit_diff(g, w) == 0) if k in ('y_scale', 'fval') else np.array_equal(g, w), (c, k)
    assert grid_want.tobytes() == want.grid.tobytes(), c


def test_refit_aligned_rows_padding_and_grids(env, aligned):
    """Per candidate the rows of its series are fit_aligned of exactly those series; padding +0.0; a duplicate of
    candidate 0 put last is never chosen by the first-minimum rule and its grid stays all zero."""
    fc, _lib = env
    cands = aligned['cands'] + [aligned['cands'][0]]
    r = fc.select_model(cands, aligned['ds'], aligned['y'], H, cap=aligned['cap'], **CV)
    r4 = aligned['rs']['rmse']
    assert np.array_equal(r.best, r4.best) and helpers.n_bit_diff(r.score[:, :4], r4.score) == 0
    assert helpers.n_bit_diff(r.score[:, 4], r.score[:, 0]) == 0 and not (r.chosen == 4).any()
    assert r.fit.theta.shape == (8, 50) and len(r.fit.grid) == 5
    assert not any(r.fit.grid[4:5].tobytes())
    assert len(np.unique(r.chosen)) >= 2
    for c in range(4):
        sel = np.flatnonzero(r.chosen == c)
        if sel.size == 0:
            assert not any(r.fit.grid[c:c + 1].tobytes())
            continue
        want = fc.fit_aligned(cands[c], aligned['ds'], aligned['y'][sel], cap=aligned['cap'][sel])
        _assert_rows(r, c, sel, want, r.fit.grid[c:c + 1])
    # the four-candidate call's refit: the same rows
    assert helpers.n_bit_diff(r4.fit.theta, r.fit.theta) == 0 and r4.fit.grid.tobytes() == r.fit.grid[:4].tobytes()


def _fit_ragged_by_rule(fc, _lib, spec, p, sel):
    """fit_ragged of exactly the series sel with spec under algorithm AUTO's rule done by hand: Newton below 100 rows,
    L-BFGS otherwise and Newton once more after a failed L-BFGS ending.  -> FitResult over sel, in order."""
    off = p['off']

    def sub(idx, sp):
        rows = np.concatenate([np.arange(off[n], off[n + 1]) for n in idx])
        o = np.concatenate([[0], np.cumsum([off[n + 1] - off[n] for n in idx])]).astype(np.int64)
        return fc.fit_ragged(sp, o, p['ds'][rows], p['y'][rows], cap=p['cap'][idx])
    lens = np.diff(off)[sel]
    nw, lb = helpers.explicit_algorithm(spec, _lib.ALGO_NEWTON), helpers.explicit_algorithm(spec, _lib.ALGO_LBFGS)
    out = [None] * len(sel)
    short, rest = np.flatnonzero(lens < 100), np.flatnonzero(lens >= 100)
    parts = []
    if rest.size:
        f = sub(sel[rest], lb)
        retry = np.flatnonzero(np.isin(f.status, helpers.retry_statuses(_lib)))
        parts.append((rest, f))
        if retry.size:
            parts.append((rest[retry], sub(sel[rest[retry]], nw)))
    if short.size:
        parts.append((short, sub(sel[short], nw)))
    for pos, f in parts:
        for i, k in enumerate(pos):
            out[k] = (f, i)
    pick = lambda key: np.array([getattr(f, key)[i] for f, i in out])      # noqa: E731
    return fc.FitResult(spec, pick('theta'), pick('y_scale'), pick('fval'), pick('status'), pick('n_iter'), pick('n_eval'),
                        pick('grid'))


def test_refit_ragged_rows_padding_and_grids(env, ragged):
    """The ragged refit under algorithm AUTO: per candidate its series' rows are fit_ragged of exactly those series by
    the rule; grid [N]; the series without folds are fitted with the fallback."""
    fc, _lib = env
    r = ragged['r']
    assert r.fit.theta.shape == (8, 50) and len(r.fit.grid) == 8
    for c in np.unique(r.chosen):
        sel = np.flatnonzero(r.chosen == c)
        want = _fit_ragged_by_rule(fc, _lib, ragged['cands'][c], ragged, sel)
        _assert_rows(r, c, sel, want, r.fit.grid[sel])
    assert set(np.unique(r.chosen)) >= {2}


def test_predict_is_predict_per_group(env, aligned, ragged):
    fc, _lib = env
    from time_series_spark_amd import synth
    fut = synth.daily_grid(430)[400:]
    for p, r in ((aligned, aligned['rs']['rmse']), (ragged, ragged['r'])):
        yhat = r.predict(fut, cap=p['cap'])
        assert yhat.shape == (8, 30)
        groups = r.groups()
        assert sorted(np.concatenate([idx for _, idx, _ in groups]).tolist()) == list(range(8))
        for c, idx, f in groups:
            assert f.spec is r.candidates[c] and f.theta.shape[1] == f.spec.theta_stride
            # (a series no fit reached -- the single row of the ragged panel -- has an empty grid: NaN, not predicted)
            ok = np.arange(len(idx)) if r.aligned else np.flatnonzero(f.status != _lib.ST_TOO_FEW)
            want = fc.predict(f.spec, f.theta[ok], f.y_scale[ok], f.grid if r.aligned else f.grid[ok], fut,
                              cap=p['cap'][idx[ok]])
            assert helpers.n_bit_diff(yhat[idx[ok]], want) == 0, c
            assert np.isnan(np.delete(yhat[idx], ok, axis=0)).all()
    assert np.isnan(ragged['r'].predict(fut, cap=ragged['cap'])[4]).all() and ragged['r'].fit.status[4] == _lib.ST_TOO_FEW
    assert np.isfinite(aligned['rs']['rmse'].predict(fut, cap=aligned['cap'])).all()
    fr = aligned['rs']['rmse'].frame()
    assert list(fr.columns) == ['series', 'candidate', 'status', 'seasonality_mode', 'growth', 'n_changepoints',
                                'seasonalities', 'metric', 'score']


def test_agrees_with_tune_on_prior_scale_candidates(env, aligned):
    """Candidates that differ in prior scales only: score, cand_status and best (tolerance 0) are tune's, and so are the
    refit rows of the series with a choice."""
    fc, _lib = env
    spec = fc.ModelSpec(growth='linear', seasonalities=[WEEKLY])
    t = fc.tune(spec, aligned['ds'], aligned['y'], H, grid={'changepoint_prior_scale': [0.01, 0.5, 0.05]}, **CV)
    r = fc.select_model(t.candidates, aligned['ds'], aligned['y'], H, **CV)
    assert helpers.n_bit_diff(r.score, t.score) == 0
    assert np.array_equal(r.cand_status, t.cand_status) and np.array_equal(r.best, t.best)
    assert np.array_equal(r.status, t.status)
    has = np.flatnonzero(t.best >= 0)
    assert has.size == 8
    assert helpers.n_bit_diff(r.fit.theta[has], t.fit.theta[has]) == 0
    for k in FIT_KEYS:
        assert np.array_equal(getattr(r.fit, k)[has], getattr(t.fit, k)[has]), k
    for c in np.unique(t.best):
        assert r.fit.grid[c:c + 1].tobytes() == t.fit.grid.tobytes()


def test_fold_panels_are_shared(env, aligned):
    """last_tune_counts: four candidates cut the fold panels a one-candidate call cuts (algorithm L-BFGS: one group, no
    retries to add), and launch the sum of the candidates' fits."""
    fc, _lib = env
    kw = dict(cap=aligned['cap'], refit=False, **CV)
    ones = []
    for c in aligned['cands']:
        fc.select_model([c], aligned['ds'], aligned['y'], H, **kw)
        ones.append(fc.last_tune_counts())
    fc.select_model(aligned['cands'], aligned['ds'], aligned['y'], H, **kw)
    exp, fits = fc.last_tune_counts()
    retries = 0                                 # (L-BFGS only: the rule retries nothing)
    assert all(e == ones[0][0] for e, _ in ones) and exp == ones[0][0] + retries == 1
    assert fits == sum(f for _, f in ones) == 4
    r = fc.select_model(aligned['cands'], aligned['ds'], aligned['y'], H, cap=aligned['cap'], **CV)
    assert fc.last_tune_counts() == (1, 4 + len(np.unique(r.chosen)))


def test_specified_changepoints_in_one_candidate(env, aligned):
    """One candidate with specified changepoint dates, some behind the earlier cutoffs: its folds keep their own leading
    dates, and its scores are cross_validate's with it; the other candidate's are unchanged."""
    fc, _lib = env
    ds, y = aligned['ds'], aligned['y']
    dates = [int(ds[k]) for k in (40, 120, 200, 270, 300, 350)]
    cands = [aligned['cands'][0], fc.ModelSpec(growth='linear', seasonalities=[YEARLY, WEEKLY], changepoints=dates)]
    assert (aligned['plan']['cutoff'] < dates[-1]).any() and (aligned['plan']['cutoff'] >= dates[-2]).any()
    r = fc.select_model(cands, ds, y, H, refit=False, **CV)
    cv = fc.cross_validate(cands[1], ds, y, H, rolling_window=1.0, **CV)
    assert np.array_equal(r.cand_status[:, 1], cv.status) and (cv.status == 0).all()
    assert helpers.n_bit_diff(r.score[:, 1], _cv_column(cv, 'rmse')) == 0
    cv0 = fc.cross_validate(cands[0], ds, y, H, rolling_window=1.0, **CV)
    assert helpers.n_bit_diff(r.score[:, 0], _cv_column(cv0, 'rmse')) == 0
    assert fc.last_tune_counts()[0] == 2        # the two candidates keep different dates per fold: a panel each


def test_split_over_two_contexts(env):
    """devices=[0, 0]: the panel split by series over two contexts gives the single call's result."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N = 2 * fc.MIN_SERIES_PER_DEVICE
    ds, y = synth.make_panel(N, 160, 'linear', seed=8)
    cands = [fc.ModelSpec(growth='linear', seasonalities=[WEEKLY], n_changepoints=5),
             fc.ModelSpec(growth='linear', seasonality_mode='multiplicative', seasonalities=[WEEKLY])]
    kw = dict(period=28 * DAY, tolerance=0.01)
    one = fc.select_model(cands, ds, y, 14 * DAY, **kw)
    two = fc.select_model(cands, ds, y, 14 * DAY, devices=[0, 0], **kw)
    assert len(np.unique(one.chosen)) == 2
    assert helpers.n_bit_diff(one.score, two.score) == 0
    for k in ('cand_status', 'best', 'chosen', 'status'):
        assert np.array_equal(getattr(one, k), getattr(two, k)), k
    assert helpers.n_bit_diff(one.fit.theta, two.fit.theta) == 0
    for k in FIT_KEYS:
        assert np.array_equal(getattr(one.fit, k), getattr(two.fit, k)), k
    assert one.fit.grid.tobytes() == two.fit.grid.tobytes()


def test_refusals_leave_the_context_usable(env, aligned):
    """Every refusal is an error with a message, before any launch; the context fits afterwards."""
    fc, _lib = env
    ds, y, cap = aligned['ds'], aligned['y'], aligned['cap']
    c0, c1, c2, _ = aligned['cands']
    with_extra = fc.ModelSpec(growth='linear', seasonalities=[WEEKLY], extra=[{'name': 'x', 'prior_scale': 1.0}])
    other_opt = fc.ModelSpec(growth='linear', seasonalities=[WEEKLY], max_iter=77)
    bad_scale = fc.ModelSpec(growth='linear', seasonalities=[WEEKLY], changepoint_prior_scale=float('inf'))
    ctx = fc.get_context()

    def refused(match, cands, **kw):
        with pytest.raises(_lib.TsfError, match=match):
            fc.select_model(cands, ds, y, H, ctx=ctx, **dict(CV, **kw))
    refused('n_extra', [c0, with_extra], extra=np.zeros((1, 400)))
    refused('optimiser', [c0, other_opt])
    refused('needs cap', [c0, c2])
    refused('prior scales', [c0, bad_scale])
    for tol in (-0.01, float('nan'), float('inf')):
        refused('tolerance', [c0, c1], tolerance=tol)
    refused('fallback', [c0, c1], fallback=2)
    refused('fallback', [c0, c1], fallback=-1)
    refused('TSF_TUNE_MAX_CAND', [])
    with pytest.raises(ValueError):
        fc.select_model([c0] * (_lib.TUNE_MAX_CAND + 1), ds, y, H, **CV)
    # straight at the C entry: C = 257, NULL outputs, refit with an incomplete fit
    L = _lib.load()
    carr = (_lib.TsfSpec * 257)(*([c0.to_c(), c1.to_c()] * 128 + [c0.to_c()]))
    N = len(y)
    bufs = [np.zeros((N, 257)), np.zeros((N, 257), np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32),
            np.zeros(N, np.int32)]
    a = fc._cv_args(H, CV['period'], CV['initial'], 1.0)

    def raw(C, out, refit=0):
        rc = L.tsf_select(ctx.handle, carr, C, N, 400, None, ds.ctypes.data, y.ctypes.data, _lib.y_dtype_code(y), None,
                          cap.ctypes.data, None, ctypes.byref(a), _lib.TUNE_RMSE, 0.0, 0, refit,
                          None if out is None else ctypes.byref(out))
        return rc, L.tsf_last_error(ctx.handle)
    ptrs = [b.ctypes.data for b in bufs]
    full = _lib.TsfSelectOut(*ptrs, _lib.TsfFitOut())
    rc, msg = raw(257, full)
    assert rc != 0 and b'TSF_TUNE_MAX_CAND' in msg
    rc, msg = raw(0, full)
    assert rc != 0 and b'TSF_TUNE_MAX_CAND' in msg
    rc, msg = raw(2, None)
    assert rc != 0 and b'NULL' in msg
    for k in range(5):
        rc, msg = raw(2, _lib.TsfSelectOut(*[None if i == k else p for i, p in enumerate(ptrs)], _lib.TsfFitOut()))
        assert rc != 0 and b'NULL' in msg, k
    fout, _ = fc._alloc_out(N, 50, 2)
    fout.grid = None
    rc, msg = raw(2, _lib.TsfSelectOut(*ptrs, fout), refit=1)
    assert rc != 0 and b'tsf_select_out.fit' in msg
    f = fc.fit_aligned(c0, ds, y[:2], ctx=ctx)
    assert f.theta.shape == (2, 50) and np.isfinite(f.fval).all() and (f.n_iter > 0).all()


def test_abi_select_plain_c(env, tmp_path):
    """tests/c/abi_select.c drives tsf_select from plain C99 -- two candidates of different stride, the sizes and the
    padding checked there -- and writes what the binding returns."""
    fc, _lib = env
    from time_series_spark_amd import synth
    root = helpers.ROOT
    N, T = 4, 400
    ds, y = synth.make_panel(N, T, 'linear', seed=2)
    ds.astype(np.int64).tofile(str(tmp_path / 'ds.i64'))
    np.ascontiguousarray(y, np.float64).tofile(str(tmp_path / 'y.f64'))
    exe = str(tmp_path / 'abi_select')
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_select.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(N), str(T), str(tmp_path / 'ds.i64'), str(tmp_path / 'y.f64'), str(tmp_path / 'out.f64')])
    got = np.fromfile(str(tmp_path / 'out.f64'))
    cands = [fc.ModelSpec(growth='linear', seasonalities=[WEEKLY], n_changepoints=5),
             fc.ModelSpec(growth='linear', seasonality_mode='multiplicative', seasonalities=[WEEKLY])]
    assert [c.theta_stride for c in cands] == [14, 34]
    r = fc.select_model(cands, ds, y, H, tolerance=0.02, fallback=1)
    want = np.concatenate([r.score.ravel(), r.best.astype(np.float64), r.chosen.astype(np.float64), r.fit.theta.ravel()])
    assert helpers.n_bit_diff(got, want) == 0
