"""GPU tests of outlier screening (include/tsf.h, "outlier screening"): tsf_screen_rows against the numpy restatement
of its contract (tests/screen_ref.py) bit for bit, fc.screen and fc.fit_screened against the composition of the public
calls they stand for, the property the feature is for (injected spikes are flagged, clean panels are not, the screened
forecast lies nearer the clean series' forecast), refusals and statuses, the modeler job, and the entries from plain C."""
import ctypes
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import helpers, screen_cases as sc, screen_ref as sr

pytestmark = pytest.mark.gpu

FIELDS = ('flag', 'resid', 'center', 'scale', 'n_new', 'n_flagged', 'status')     # tsf_screen_out's member order
FIT_FIELDS = ('theta', 'y_scale', 'status', 'n_iter')
DAY = 86400 * 10 ** 9


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU screening tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _hip_runtime():
    """the HIP runtime libtsf_amd.so is linked against, for device blocks of the test's own"""
    for name in ('libamdhip64.so', os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'libamdhip64.so')):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            continue
    else:
        pytest.fail('libamdhip64.so not found')
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


def _same_screen(got, want, what=''):
    for k in FIELDS:
        assert sr.same(getattr(got, k), want[k]), (what, k)


def _same_fit(a, ia, b, ib, what=''):
    """series ia of FitResult a == series ib of FitResult b: theta, y_scale, status, n_iter and the grid, bit for bit"""
    for k in FIT_FIELDS:
        assert sr.same(getattr(a, k)[ia], getattr(b, k)[ib]), (what, k)
    ga = a.grid[[0] * len(ia)] if len(a.grid) == 1 else a.grid[ia]
    gb = b.grid[[0] * len(ib)] if len(b.grid) == 1 else b.grid[ib]
    assert ga.tobytes() == gb.tobytes(), (what, 'grid')


# ---- 1. the rule, bit for bit ------------------------------------------------------------------------------------------

def _rule_inputs(lengths, dtype, seed):
    """a ragged panel: per series integer-valued residuals with many ties (even series) or Gaussian ones (odd), a few
    far rows, exclusions at both ends and in the middle"""
    rng = np.random.default_rng(seed)
    ys, fs, es = [], [], []
    for n, m in enumerate(lengths):
        base = np.round(rng.normal(0, 3, m)) if n % 2 == 0 else rng.normal(0, 3, m)
        if m >= 8:
            base[rng.choice(m, max(1, m // 16), replace=False)] += rng.choice([-1.0, 1.0]) * 60.0
        fitted = np.round(rng.normal(50, 10, m)) if n % 2 == 0 else rng.normal(50, 10, m)
        y = fitted + base
        if dtype != np.float64:
            y = np.rint(y)
        e = np.zeros(m, np.uint8)
        if m >= 8 and n % 3 != 2:
            e[[0, m // 2, m - 1]] = 1
        ys.append(y.astype(dtype)); fs.append(fitted); es.append(e)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return off, np.concatenate(ys), np.concatenate(fs), np.concatenate(es)


@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32], ids=['f64', 'f32', 'i32'])
@pytest.mark.parametrize('T', [2, 63, 64, 65, 257, 1030])
def test_rule_aligned_bit_for_bit(env, T, dtype):
    fc, _lib = env
    N = 5
    off, y, f, e = _rule_inputs([T] * N, dtype, seed=T)
    ms = np.array([0.0, 0.0, 1.0, 1e-3, 40.0])
    kw = dict(threshold=3.0, max_share=0.1 if T > 2 else 0.5, min_rows=2)
    for excluded, min_scale in ((None, None), (e.reshape(N, T), ms)):
        got = fc.screen_rows(y.reshape(N, T), f.reshape(N, T), excluded=excluded, min_scale=min_scale, **kw)
        _same_screen(got, sr.screen(y.reshape(N, T), f.reshape(N, T), excluded=excluded, min_scale=min_scale, **kw), T)
    assert T < 8 or got.n_new.sum() > 0


@pytest.mark.parametrize('dtype', [np.float64, np.int32], ids=['f64', 'i32'])
def test_rule_ragged_lengths_together(env, dtype):
    """lengths 2 .. 1030 in one call (one launch per power-of-two class), an empty series and a one-row series among them"""
    fc, _lib = env
    lengths = [1030, 2, 63, 0, 64, 65, 257, 1, 3, 700, 129, 16, 2]
    off, y, f, e = _rule_inputs(lengths, dtype, seed=9)
    kw = dict(threshold=3.0, max_share=0.1, min_rows=2)
    for excluded in (None, e):
        got = fc.screen_rows(y, f, offsets=off, excluded=excluded, **kw)
        _same_screen(got, sr.screen(y, f, offsets=off, excluded=excluded, **kw))
    assert list(got.status[[3, 7]]) == [_lib.SCREEN_TOO_FEW] * 2 and got.n_new.sum() > 0


def test_rule_ragged_panel_without_rows(env):
    """offsets all zero: three series, no row at all -- nothing is copied either way, every series too short"""
    fc, _lib = env
    got = fc.screen_rows(np.zeros(0), np.zeros(0), offsets=np.zeros(4, np.int64), threshold=3.0, max_share=0.1, min_rows=5)
    assert got.flag.shape == (0,) and got.resid.shape == (0,)
    assert list(got.status) == [_lib.SCREEN_TOO_FEW] * 3 and _lib.SCREEN_TOO_FEW == -30
    assert np.isnan(got.center).all() and np.isnan(got.scale).all()
    assert list(got.n_new) == [0, 0, 0] and list(got.n_flagged) == [0, 0, 0]


def test_rule_longest_series_and_too_long(env):
    fc, _lib = env
    lengths = [_lib.SCREEN_MAX_ROWS, _lib.SCREEN_MAX_ROWS + 1, 100]
    off, y, f, e = _rule_inputs(lengths, np.float64, seed=11)
    kw = dict(threshold=3.0, max_share=0.05, min_rows=10)
    got = fc.screen_rows(y, f, offsets=off, excluded=e, **kw)
    _same_screen(got, sr.screen(y, f, offsets=off, excluded=e, **kw))
    assert list(got.status) == [_lib.SCREEN_OK, _lib.SCREEN_TOO_LONG, _lib.SCREEN_OK]
    s1 = slice(int(off[1]), int(off[2]))
    assert np.array_equal(got.flag[s1], e[s1]) and got.n_new[0] > 0
    # an aligned panel of the longest length: every series through the 128 KiB sort
    N, T = 2, _lib.SCREEN_MAX_ROWS
    off, y, f, e = _rule_inputs([T] * N, np.float32, seed=12)
    got = fc.screen_rows(y.reshape(N, T), f.reshape(N, T), **kw)
    _same_screen(got, sr.screen(y.reshape(N, T), f.reshape(N, T), **kw))


@pytest.mark.parametrize('ragged', [False, True], ids=['aligned', 'ragged'])
def test_rule_dev_variant_agrees(env, ragged):
    """tsf_screen_rows_dev on device pointers (plain hipMalloc blocks) == the host variant"""
    fc, _lib = env
    lengths = [257] * 4 if not ragged else [257, 2, 1030, 64]
    off, y, f, e = _rule_inputs(lengths, np.float64, seed=13)
    N = len(lengths)
    ms = np.full(N, 1e-3)
    kw = dict(threshold=3.0, max_share=0.1, min_rows=2)
    shape = (N, 257) if not ragged else y.shape
    want = fc.screen_rows(y.reshape(shape), f.reshape(shape), offsets=off if ragged else None, excluded=e.reshape(shape),
                          min_scale=ms, **kw)
    hip = _hip_runtime()
    R = len(y)
    bufs = []

    def dev(a_):
        a_ = np.ascontiguousarray(a_)
        p_ = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p_), max(a_.nbytes, 8)) == 0
        bufs.append(p_)
        assert hip.hipMemcpy(p_, a_.ctypes.data, a_.nbytes, 1) == 0             # hipMemcpyHostToDevice
        return p_
    host = dict(flag=np.full(R, 7, np.uint8), resid=np.zeros(R), center=np.zeros(N), scale=np.zeros(N),
                n_new=np.zeros(N, np.int32), n_flagged=np.zeros(N, np.int32), status=np.zeros(N, np.int32))
    try:
        d_y, d_f, d_e, d_ms, d_off = dev(y), dev(f), dev(e), dev(ms), dev(off)
        o = {k: dev(v) for k, v in host.items()}
        out = _lib.TsfScreenOut(*[o[k] for k in FIELDS])
        a = fc._screen_args(**kw)
        ctx = fc.get_context()
        ctx.check(_lib.load().tsf_screen_rows_dev(ctx.handle, N, 0 if ragged else 257, d_off if ragged else None, d_y, _lib.Y_F64,
                                                  d_f, d_e, d_ms, ctypes.byref(a), ctypes.byref(out), None))
        assert hip.hipDeviceSynchronize() == 0
        for k, v in host.items():
            assert hip.hipMemcpy(v.ctypes.data, o[k], v.nbytes, 2) == 0         # hipMemcpyDeviceToHost
    finally:
        for p_ in bufs:
            hip.hipFree(p_)
    for k in FIELDS:
        assert sr.same(host[k].reshape(getattr(want, k).shape), getattr(want, k)), k


# ---- the fitted panels: computed once, read-only -------------------------------------------------------------------------

@pytest.fixture(scope='module')
def fitted(env):
    """per (kind, layout): the case (8 spiked + 2 clean series), its spec, fit_screened's result and the call's arguments"""
    fc, _lib = env
    cache = {}

    def get(kind, ragged, passes=1):
        key = (kind, ragged, passes)
        if key not in cache:
            c = sc.make(kind, n_clean_extra=2)
            spec = fc.ModelSpec(**c.spec_kw)
            if ragged:
                off, ds, y = sc.ragged(c)
                args = dict(ds_ns=ds, y=y, offsets=off)
            else:
                args = dict(ds_ns=c.ds, y=c.y, offsets=None)
            args.update(floor=c.floor, cap=c.cap)
            cache[key] = (c, spec, args, fc.fit_screened(spec, passes=passes, **args, **sc.SCREEN))
        return cache[key]
    return get


def _plain_fit(fc, spec, args):
    if args['offsets'] is None:
        return fc.fit_aligned(spec, args['ds_ns'], args['y'], floor=args['floor'], cap=args['cap'], extra=args.get('extra'))
    return fc.fit_ragged(spec, args['offsets'], args['ds_ns'], args['y'], floor=args['floor'], cap=args['cap'],
                         extra=args.get('extra'))


def _refit_by_hand(fc, spec, args, flag, sel):
    """fc.fit_ragged on the numpy-cut panel of the series sel -> FitResult over sel"""
    off, ds, y, ex = sr.cut_panel(args['ds_ns'], args['y'], flag, args['offsets'], args.get('extra'))
    rows = np.concatenate([np.arange(off[n], off[n + 1]) for n in sel])
    o2 = np.concatenate([[0], np.cumsum(np.diff(off)[sel])]).astype(np.int64)
    pick = lambda a: None if a is None else np.asarray(a)[sel]      # noqa: E731
    return fc.fit_ragged(spec, o2, ds[rows], y[rows], floor=pick(args['floor']), cap=pick(args['cap']),
                         extra=None if ex is None else ex[:, rows])


# ---- 2. fc.screen is the composition --------------------------------------------------------------------------------------

@pytest.mark.parametrize('ragged', [False, True], ids=['aligned', 'ragged'])
def test_screen_is_predict_then_the_rule(env, ragged):
    fc, _lib = env
    c = sc.make('lin120')
    spec = fc.ModelSpec(**c.spec_kw)
    if ragged:
        # different lengths, so the padded future panel has padding
        lens = [120, 100, 120, 61, 120, 120, 33, 120]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ds = np.concatenate([c.ds[:m] for m in lens])
        y = np.concatenate([c.y[n, :m] for n, m in enumerate(lens)])
        fit = fc.fit_ragged(spec, off, ds, y)
        fut = np.stack([np.concatenate([c.ds[:m], np.full(120 - m, c.ds[m - 1])]) for m in lens])
        yh = fc.predict(spec, fit.theta, fit.y_scale, fit.grid, fut)
        want = np.concatenate([yh[n, :m] for n, m in enumerate(lens)])
        s = fc.screen(spec, fit, ds, y, offsets=off, **sc.SCREEN)
    else:
        y = c.y
        fit = fc.fit_aligned(spec, c.ds, y)
        want = fc.predict(spec, fit.theta, fit.y_scale, fit.grid, c.ds)
        s = fc.screen(spec, fit, c.ds, y, **sc.SCREEN)
    assert sr.same(s.fitted, want) and sr.same(s.resid, y - want)
    _same_screen(s, sr.screen(y, want, offsets=off if ragged else None, min_scale=1e-8 * fit.y_scale, **sc.SCREEN))
    assert s.n_new.sum() > 0


# ---- 3. fit_screened is the composition -------------------------------------------------------------------------------------

def _check_composition(fc, c, spec, args, sf):
    first = _plain_fit(fc, spec, args)
    N = c.N
    every = np.arange(N)
    _same_fit(sf.first, every, first, every, 'first')
    assert sr.same(sf.first.fval, first.fval) and sr.same(sf.first.n_eval, first.n_eval)
    assert len(sf.first.grid) == len(first.grid) and len(sf.fit.grid) == N
    s = fc.screen(spec, first, args['ds_ns'], args['y'], offsets=args['offsets'], floor=args['floor'], cap=args['cap'],
                  extra=args.get('extra'), **sc.SCREEN)
    for k in FIELDS:
        assert sr.same(getattr(sf.screen, k), getattr(s, k)), k
    flagged = np.flatnonzero(s.n_new > 0)
    clean = np.flatnonzero(s.n_new == 0)
    assert len(flagged) >= sc.N_SPIKED and len(clean) >= 1
    assert np.array_equal(sf.rounds, (s.n_new > 0).astype(np.int32))
    _same_fit(sf.fit, clean, first, clean, 'never flagged')
    by_hand = _refit_by_hand(fc, spec, args, s.flag, flagged)
    _same_fit(sf.fit, flagged, by_hand, np.arange(len(flagged)), 'flagged')
    assert sr.same(sf.fit.fval[flagged], by_hand.fval)


@pytest.mark.parametrize('ragged', [False, True], ids=['aligned', 'ragged'])
@pytest.mark.parametrize('kind', list(sc.KINDS))
def test_fit_screened_is_fit_screen_cut_refit(env, fitted, kind, ragged):
    fc, _lib = env
    c, spec, args, sf = fitted(kind, ragged)
    _check_composition(fc, c, spec, args, sf)


def _fit_by_rule(fc, _lib, spec, rows, fit_group, one_grid=False):
    """fbprophet's optimiser rule for algorithm AUTO done by hand over series of `rows` rows each, with explicit
    ALGO_LBFGS / ALGO_NEWTON specs: L-BFGS from 100 rows on, Newton once more where it ended the way pystan raises on,
    Newton below 100 rows.  fit_group(spec, indices) -> FitResult over the indices.  Returns the FitResult over all
    series (one_grid: an aligned panel's single grid) and the L-BFGS statuses of the series of >= 100 rows."""
    rows = np.asarray(rows)
    idx = np.arange(len(rows))
    got = {}

    def put(sp, sel):
        if len(sel) == 0:
            return np.zeros(0, np.int32)
        f = fit_group(sp, sel)
        for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval', 'grid'):
            v = getattr(f, k)
            if k == 'grid' and one_grid:
                got[k] = v
                continue
            got.setdefault(k, np.zeros((len(rows),) + v.shape[1:], v.dtype))[sel] = v
        return f.status.copy()
    sp_l, sp_n = helpers.explicit_algorithm(spec, _lib.ALGO_LBFGS), helpers.explicit_algorithm(spec, _lib.ALGO_NEWTON)
    lb = idx[rows >= 100]
    st = put(sp_l, lb)
    put(sp_n, lb[np.isin(st, helpers.retry_statuses(_lib))])
    put(sp_n, idx[rows < 100])
    return fc.FitResult(spec, *[got[k] for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval', 'grid')]), st


@pytest.mark.parametrize('zero_tol', [False, True], ids=['default_tol', 'zero_tol'])
@pytest.mark.parametrize('ragged', [False, True], ids=['aligned', 'ragged'])
def test_fit_screened_auto_is_the_rule_by_hand(env, ragged, zero_tol):
    """algorithm AUTO: the first fit and the refit of the cut series are fbprophet's rule per series -- on the aligned
    120-row panel everything is L-BFGS; the ragged panel has a spiked series of 80 rows besides, so both optimiser groups
    occur in the first fit and in the refit; with every tolerance zero L-BFGS ends in a failed line search and the
    Newton retry is taken (asserted on the by-hand L-BFGS statuses)."""
    fc, _lib = env
    c = sc.make('lin120', n_clean_extra=2)
    spec = fc.ModelSpec(algorithm=_lib.ALGO_AUTO, **c.spec_kw, **(helpers.ZERO_TOL if zero_tol else {}))
    if ragged:
        off, ds, y = sc.ragged(c)
        short = int(np.flatnonzero((c.rows < 70).sum(axis=1) >= 1)[0])        # a spike within its first 70 rows
        off, ds, y = np.append(off, off[-1] + 80), np.concatenate([ds, c.ds[:80]]), np.concatenate([y, c.y[short, :80]])
        args = dict(ds_ns=ds, y=y, offsets=off, floor=None, cap=None)
        rows = np.diff(off)

        def fit_first(sp, sel):
            o2 = np.concatenate([[0], np.cumsum(rows[sel])]).astype(np.int64)
            pick = np.concatenate([np.arange(off[n], off[n + 1]) for n in sel])
            return fc.fit_ragged(sp, o2, ds[pick], y[pick])
    else:
        args = dict(ds_ns=c.ds, y=c.y, offsets=None, floor=None, cap=None)
        rows = np.full(c.N, c.T)

        def fit_first(sp, sel):
            return fc.fit_aligned(sp, c.ds, c.y[sel])
    N = len(rows)
    every = np.arange(N)
    sf = fc.fit_screened(spec, args['ds_ns'], args['y'], offsets=args['offsets'], **sc.SCREEN)
    first, st_first = _fit_by_rule(fc, _lib, spec, rows, fit_first, one_grid=not ragged)
    print('first fit: L-BFGS statuses', st_first)
    assert ((rows < 100).any() and (rows >= 100).any()) == ragged
    retry = helpers.retry_statuses(_lib)
    assert np.isin(st_first, retry).any() or not zero_tol
    _same_fit(sf.first, every, first, every, 'first')
    assert sr.same(sf.first.fval, first.fval) and sr.same(sf.first.n_eval, first.n_eval)
    assert len(sf.first.grid) == len(first.grid) and len(sf.fit.grid) == N
    s = fc.screen(spec, first, args['ds_ns'], args['y'], offsets=args['offsets'], **sc.SCREEN)
    for k in FIELDS:
        assert sr.same(getattr(sf.screen, k), getattr(s, k)), k
    flagged, clean = np.flatnonzero(s.n_new > 0), np.flatnonzero(s.n_new == 0)
    assert len(flagged) >= sc.N_SPIKED and len(clean) >= 1
    assert np.array_equal(sf.rounds, (s.n_new > 0).astype(np.int32))
    _same_fit(sf.fit, clean, first, clean, 'never flagged')
    kept = (rows - s.n_flagged)[flagged]
    assert ((kept < 100).any() and (kept >= 100).any()) == ragged
    by_hand, st_refit = _fit_by_rule(fc, _lib, spec, kept, lambda sp, sel: _refit_by_hand(fc, sp, args, s.flag, flagged[sel]))
    print('refit: L-BFGS statuses', st_refit)
    assert np.isin(st_refit, retry).any() or not zero_tol
    _same_fit(sf.fit, flagged, by_hand, np.arange(len(flagged)), 'flagged')
    assert sr.same(sf.fit.fval[flagged], by_hand.fval) and sr.same(sf.fit.n_eval[flagged], by_hand.n_eval)


@pytest.mark.parametrize('ragged', [False, True], ids=['aligned', 'ragged'])
def test_fit_screened_with_an_extra_column_and_int32_y(env, ragged):
    fc, _lib = env
    c = sc.make('lin120', n_clean_extra=2, dtype=np.int32)
    spec = fc.ModelSpec(extra=[{'name': 'promo'}], **c.spec_kw)
    x = (np.arange(c.T) % 11 == 3).astype(np.float64)[None, :]
    if ragged:
        off, ds, y = sc.ragged(c)
        args = dict(ds_ns=ds, y=y, offsets=off, extra=np.tile(x, (1, c.N)))
    else:
        args = dict(ds_ns=c.ds, y=c.y, offsets=None, extra=x)
    args.update(floor=None, cap=None)
    sf = fc.fit_screened(spec, args['ds_ns'], args['y'], offsets=args['offsets'], extra=args['extra'], **sc.SCREEN)
    _check_composition(fc, c, spec, args, sf)


# ---- 4. two passes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ragged', [False, True], ids=['aligned', 'ragged'])
def test_two_passes_are_the_loop_by_hand(env, fitted, ragged):
    fc, _lib = env
    c, spec, args, sf = fitted('lin120', ragged, passes=2)
    fit = _plain_fit(fc, spec, args)
    N = c.N
    if len(fit.grid) == 1:
        fit.grid = fit.grid[[0] * N]
    flag = np.zeros(np.asarray(args['y']).shape, np.uint8)
    rounds = np.zeros(N, np.int32)
    active = np.arange(N)
    last = {}
    for p in range(2):
        s = fc.screen(spec, fit, args['ds_ns'], args['y'], offsets=args['offsets'], excluded=flag, **sc.SCREEN)
        for n in active:
            last[int(n)] = (s, p)
        new = active[s.n_new[active] > 0]
        if p == 0:
            # a series at its budget (checked on the CPU oracle: 12 rows of series 6), others with budget to spare
            assert s.n_flagged.max() == int(np.floor(sc.SCREEN['max_share'] * c.T)) and len(new) >= sc.N_SPIKED
        if len(new) == 0:
            break
        rows = flag.reshape(N, -1)
        rows[new] = s.flag.reshape(N, -1)[new]
        rounds[new] += 1
        r = _refit_by_hand(fc, spec, args, flag, new)
        for k in FIT_FIELDS + ('fval', 'n_eval', 'grid'):
            getattr(fit, k)[new] = getattr(r, k)
        active = new
    assert max(p for _s, p in last.values()) == 1                           # round 2 screened the refitted series
    assert np.array_equal(sf.rounds, rounds) and np.array_equal(sf.screen.flag, flag)
    _same_fit(sf.fit, np.arange(N), fit, np.arange(N), 'two passes')
    for n, (s, p) in last.items():
        for k in ('center', 'scale', 'status'):
            assert sr.same(getattr(sf.screen, k)[n], getattr(s, k)[n]), (n, k)
        assert sr.same(sf.screen.resid.reshape(N, -1)[n], s.resid.reshape(N, -1)[n]), n
    assert np.array_equal(sf.screen.n_flagged, flag.reshape(N, -1).sum(axis=1))


# ---- 5. it helps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', list(sc.KINDS))
def test_screening_recovers_the_clean_forecast(env, fitted, kind):
    fc, _lib = env
    c, spec, args, sf = fitted(kind, False)
    n8 = np.arange(sc.N_SPIKED)
    flag = sf.screen.flag.astype(bool)
    assert flag[c.injected].all()                                           # every injected row is flagged
    fut = c.ds[-1] + DAY * np.arange(1, 31)
    kw = dict(floor=c.floor, cap=c.cap)
    cleanfit = fc.fit_screened(spec, c.ds, c.clean, **kw, **sc.SCREEN)
    assert not cleanfit.screen.flag.any() and (cleanfit.screen.status == _lib.SCREEN_OK).all()   # the clean panel: no flag
    _same_fit(cleanfit.fit, np.arange(c.N), cleanfit.first, np.arange(c.N), 'clean')
    pred = lambda f: fc.predict(spec, f.theta, f.y_scale, f.grid, fut, **kw)     # noqa: E731
    y_clean, y_first, y_screened = pred(cleanfit.first), pred(sf.first), pred(sf.fit)
    e_un = np.abs(y_first - y_clean).max(axis=1)[n8]
    e_sc = np.abs(y_screened - y_clean).max(axis=1)[n8]
    print(kind, 'max 30-day error, screened / unscreened:', np.round(e_sc / e_un, 4))
    assert (e_sc < e_un).all()


# ---- 6. refusals and statuses ----------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(env):
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    N, T = 3, 40
    rng = np.random.default_rng(2)
    y, f = rng.normal(size=(N, T)), rng.normal(size=(N, T))
    flag, status = np.zeros((N, T), np.uint8), np.zeros(N, np.int32)

    def call(y_=y, f_=f, flag_=flag, status_=status, out=True, dtype=_lib.Y_F64, **kw):
        a = _lib.TsfScreenArgs(5.0, 0.05, 10, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        o = _lib.TsfScreenOut(_lib._ptr(flag_), None, None, None, None, None, _lib._ptr(status_))
        return L.tsf_screen_rows(ctx.handle, N, T, None, _lib._ptr(y_), dtype, _lib._ptr(f_), None, None, ctypes.byref(a),
                                 ctypes.byref(o) if out else None)
    for bad in (dict(out=False), dict(flag_=None), dict(status_=None), dict(y_=None), dict(f_=None), dict(threshold=0.0),
                dict(threshold=-1.0), dict(threshold=float('inf')), dict(threshold=float('nan')), dict(max_share=-0.01),
                dict(max_share=0.51), dict(max_share=float('nan')), dict(min_rows=1), dict(max_passes=0),
                dict(max_passes=9), dict(dtype=3), dict(dtype=-1)):
        assert call(**bad) < 0, bad
        assert len(L.tsf_last_error(ctx.handle)) > 0
        assert call() == 0, bad                     # the next call on the same context succeeds
    assert L.tsf_screen_rows(ctx.handle, 0, T, None, _lib._ptr(y), _lib.Y_F64, _lib._ptr(f), None, None,
                             ctypes.byref(_lib.TsfScreenArgs(5.0, 0.05, 10, 1)),
                             ctypes.byref(_lib.TsfScreenOut(_lib._ptr(flag), None, None, None, None, None, _lib._ptr(status)))) == 0
    # fit_screened refuses the same arguments, and a NULL member of its fit output
    c = sc.make('lin120')
    spec = fc.ModelSpec(**c.spec_kw)
    with pytest.raises(_lib.TsfError):
        a = _lib.TsfScreenArgs(5.0, 0.7, 10, 1)
        cs = spec.to_c()
        fout, _ = fc._alloc_out(c.N, spec.theta_stride, c.N)
        sout, _ = fc._alloc_screen(c.y, c.N)
        ctx.check(L.tsf_fit_screened(ctx.handle, ctypes.byref(cs), c.N, c.T, None, c.ds.ctypes.data, c.y.ctypes.data, _lib.Y_F64,
                                     None, None, None, 1e-8, ctypes.byref(a), ctypes.byref(_lib.TsfFitScreenedOut(fout, None, sout, None))))
    with pytest.raises(_lib.TsfError, match='bad algorithm'):           # outside the enum: refused up front
        fc.fit_screened(fc.ModelSpec(algorithm=7, **c.spec_kw), c.ds, c.y, **sc.SCREEN)
    assert fc.fit_screened(spec, c.ds, c.y, **sc.SCREEN).screen.n_new.sum() >= sc.N_SPIKED * sc.N_SPIKES


def test_statuses_per_series(env):
    fc, _lib = env
    rng = np.random.default_rng(3)
    N, T = 4, 30
    y, f = rng.normal(size=(N, T)), rng.normal(size=(N, T))
    y[:, 7] += 1000.0
    ex = np.zeros((N, T), np.uint8)
    ex[1, :21] = 1                                  # 9 live rows < min_rows
    f[2, 3] = np.nan                                # a NaN in fitted: nothing flagged
    y[3, 4] = np.inf
    ex[3, 4] = 1                                    # ... but not looked at on an excluded row
    kw = dict(threshold=5.0, max_share=0.2, min_rows=10)
    got = fc.screen_rows(y, f, excluded=ex, **kw)
    _same_screen(got, sr.screen(y, f, excluded=ex, **kw))
    assert list(got.status) == [_lib.SCREEN_OK, _lib.SCREEN_TOO_FEW, _lib.SCREEN_NONFINITE, _lib.SCREEN_OK]
    assert np.array_equal(got.flag[1:3], ex[1:3]) and list(got.n_new) == [1, 0, 0, 1]
    assert np.isnan(got.center[1:3]).all() and np.isnan(got.scale[1:3]).all()


# ---- 7. the job ------------------------------------------------------------------------------------------------------------

def test_modeler_job_with_screening(env, tmp_path):
    fc, _lib = env
    from time_series_spark_amd.jobs import prophet_modeler as pm
    c = sc.make('lin120')
    N = 6
    y = np.rint(c.clean[:N]).astype(np.int64)
    y[[1, 4]] = np.rint(c.y[[1, 4]]).astype(np.int64)
    stamps = pd.DatetimeIndex(c.ds.astype('datetime64[ns]')).strftime('%Y-%m-%d %H:%M:%S').values
    for n in range(N):
        d = tmp_path / 'in' / ('series_id=%d' % (70 + n))
        d.mkdir(parents=True)
        (d / 'part-0.csv').write_text('\n'.join('1,%s,%d' % (s, v) for s, v in zip(stamps, y[n])) + '\n')
    prophet = {'growth': 'linear', 'seasonality_mode': 'additive', 'yearly_seasonality': False, 'daily_seasonality': False}

    def run(tag, screen, screened=None):
        cfg = {'io': {'input': str(tmp_path / 'in'), 'models': str(tmp_path / ('m_' + tag))},
               'model': {'floor': 0, 'cap_multiplier': 1.1, 'prophet': prophet}}
        if screen is not None:
            cfg['model']['screen'] = screen
        if screened:
            cfg['io']['screened'] = str(tmp_path / screened)
        pm.ProphetModeler.model(None, cfg, return_frame=False)
        part = os.path.join(cfg['io']['models'], 'part-00000.parquet')
        return pd.read_parquet(cfg['io']['models']).sort_values(['series_id', 'dim_id']), open(part, 'rb').read()
    plain, plain_bytes = run('plain', None)
    again, again_bytes = run('again', None)
    assert plain_bytes == again_bytes               # without model.screen the models parquet is what it was
    got, _ = run('screen', dict(sc.SCREEN, passes=1), 'removed')
    assert list(got['series_id']) == list(plain['series_id']) == [70 + n for n in range(N)]
    differs = [bytes(a) != bytes(b) for a, b in zip(got['model'], plain['model'])]
    assert differs == [n in (1, 4) for n in range(N)]
    removed = pd.read_parquet(str(tmp_path / 'removed'))
    assert list(removed.columns) == pm.SCREENED_COLUMNS
    spec = fc.ModelSpec(growth='linear', seasonality_mode='additive',
                        seasonalities=fc.ModelSpec.auto_seasonalities(c.ds, yearly=False, daily=False))
    sf = fc.fit_screened(spec, c.ds, y.astype(np.float64), **sc.SCREEN)
    n_idx, t_idx = np.nonzero(sf.screen.flag)
    assert set(n_idx) == {1, 4}
    assert list(removed['series_id']) == list(70 + n_idx) and list(removed['dim_id']) == [1] * len(n_idx)
    assert np.array_equal(removed['ds'].to_numpy().astype('datetime64[ns]').astype(np.int64), c.ds[t_idx])
    assert sr.same(removed['y'].to_numpy(), y[n_idx, t_idx].astype(np.float64))
    assert sr.same(removed['resid'].to_numpy(), sf.screen.resid[n_idx, t_idx])
    assert sr.same(removed['center'].to_numpy(), sf.screen.center[n_idx]) and sr.same(removed['scale'].to_numpy(), sf.screen.scale[n_idx])
    with pytest.raises(ValueError):
        run('bad', {'thresh': 5.0})
    with pytest.raises(ValueError):
        run('bad2', None, 'removed2')               # io.screened without model.screen


# ---- 8. plain C ------------------------------------------------------------------------------------------------------------

def test_abi_screen_plain_c(env, tmp_path):
    """tests/c/abi_screen.c drives tsf_screen_rows and tsf_fit_screened from plain C99 and writes what they return"""
    fc, _lib = env
    c = sc.make('lin120', n_clean_extra=2)
    d = str(tmp_path)
    spec = fc.ModelSpec(**c.spec_kw)
    rng = np.random.default_rng(5)
    fitted_ = c.y + rng.normal(0, 1, c.y.shape)
    fitted_[:, 9] -= 500.0
    c.ds.tofile(d + '/ds.i64')
    c.y.tofile(d + '/y.f64')
    fitted_.tofile(d + '/fitted.f64')
    exe = d + '/abi_screen'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_screen.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(c.N), str(c.T), d])
    got = np.fromfile(d + '/out.f64')
    s = fc.screen_rows(c.y, fitted_, **sc.SCREEN)
    sf = fc.fit_screened(spec, c.ds, c.y, passes=2, **sc.SCREEN)
    f64 = lambda a: np.asarray(a, dtype=np.float64).ravel()     # noqa: E731
    want = np.concatenate([f64(s.flag), f64(s.resid), f64(s.center), f64(s.scale), f64(s.n_new), f64(s.n_flagged), f64(s.status),
                           f64(sf.fit.theta), f64(sf.fit.y_scale), f64(sf.fit.status), f64(sf.fit.n_iter), f64(sf.first.theta),
                           f64(sf.screen.flag), f64(sf.screen.n_flagged), f64(sf.rounds)])
    assert sr.same(got, want)
    assert np.fromfile(d + '/grid.bin', dtype=_lib.GRID_DTYPE).tobytes() == sf.fit.grid.tobytes()
