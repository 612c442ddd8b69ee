"""GPU: conformal interval calibration (include/tsf.h) -- the rule and the apply kernel against their numpy restatement
(tests/calib_ref.py), bit for bit and with no row left out; fc.calibrate against cross_validate + calibrate_cv;
predict_calibrated; the refusals; the plain C ABI; the validator's and the scorer's options."""
import ctypes
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import calib_ref as cr, helpers

pytestmark = pytest.mark.gpu

DAY = 86400 * 10 ** 9
HZ = 20 * DAY


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU calibration tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _same_table(got, want, what=''):
    assert cr.same(got.n, want['n']), (what, 'n')
    assert cr.same(got.q, want['q']), (what, 'q')
    assert cr.same(got.status, want['status']), (what, 'status')


# ---- 1. the rule on synthetic rows -------------------------------------------------------------------------------------------

LENS = [1, 63, 64, 65, 255, 256, 257, 1000, 0, 50, cr.MAX_ROWS + 1, 300]      # 9: every row dead; 11: heavy ties
L_MAX = 3


@pytest.fixture(scope='module')
def rows():
    """12 series in one ragged set (horizon 30 d): random horizons from below 0 to beyond the horizon, every bucket edge
    of B = 4 in the 1000-row series, NaN y and infinite yhat sprinkled, bounds for three levels with NaN sprinkled"""
    rng = np.random.default_rng(11)
    H = 30 * DAY
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    R = int(off[-1])
    h = rng.integers(-DAY, H + 2 * DAY, size=R)
    y = rng.normal(0, 3, R)
    yhat = y + rng.normal(0, 1, R)
    s7 = int(off[7])
    w4 = cr.bucket_width(H, 4)
    edges = [0, 1, w4, w4 + 1, 2 * w4, 2 * w4 + 1, 3 * w4, 3 * w4 + 1, H, H + 1, H - 1, -1]
    h[s7:s7 + len(edges)] = edges
    y[rng.random(R) < 0.01] = np.nan
    yhat[rng.random(R) < 0.01] = np.inf
    h[off[9]:off[10]] = 0                                                    # series 9: no row is eligible
    t0, t1 = int(off[11]), int(off[12])                                      # series 11: four distinct scores
    y[t0:t1] = rng.integers(0, 4, t1 - t0).astype(np.float64)
    yhat[t0:t1] = 0.0
    wid = np.array([1.0, 1.5, 2.5])[:, None] * np.ones((1, R))
    lower, upper = yhat[None, :] - wid, yhat[None, :] + wid
    lower[:, t0:t1], upper[:, t0:t1] = -1.0, 1.0                             # (ties under CQR too)
    lower[rng.random((L_MAX, R)) < 0.01] = np.nan
    upper[rng.random((L_MAX, R)) < 0.01] = -np.inf
    return dict(off=off, h=h, y=y, yhat=yhat, lower=lower, upper=upper, H=H)


@pytest.mark.parametrize('mode', ['abs', 'cqr'])
@pytest.mark.parametrize('L', [1, 3])
@pytest.mark.parametrize('B', [1, 4, 64])
def test_rule_bit_for_bit(env, rows, B, L, mode):
    fc, _lib = env
    r = rows
    levels = [0.8, 0.5, 0.95][:L]
    kw = dict(n_buckets=B, min_scores=5)
    lw, up = (r['lower'][:L], r['upper'][:L]) if mode == 'cqr' else (None, None)
    got = fc.calibrate_rows(r['off'], r['h'], r['y'], r['yhat'], levels, lower=lw, upper=up, mode=mode, horizon=r['H'], **kw)
    want = cr.calibrate_rows(r['off'], r['h'], r['y'], r['yhat'], levels, lw, up, mode=_lib.CALIB_MODES[mode],
                             horizon=r['H'], **kw)
    _same_table(got, want, (B, L, mode))
    st = got.status.tolist()
    assert st[8] == st[9] == _lib.CALIB_NO_SCORES and st[10] == _lib.CALIB_TOO_LONG and st[7] == st[11] == _lib.CALIB_OK
    assert (got.n[10] == 0).all() and np.isnan(got.q[10]).all() and (got.n[9] == 0).all()


@pytest.mark.parametrize('mode', ['abs', 'cqr'])
def test_rule_ignores_row_order_and_the_rest_of_the_batch(env, rows, mode):
    fc, _lib = env
    r = rows
    levels, kw = [0.8, 0.5, 0.95], dict(mode=mode, horizon=r['H'], n_buckets=4, min_scores=5)
    cq = mode == 'cqr'
    base = fc.calibrate_rows(r['off'], r['h'], r['y'], r['yhat'], levels, lower=r['lower'] if cq else None,
                             upper=r['upper'] if cq else None, **kw)
    rng = np.random.default_rng(12)
    perm = np.concatenate([a + rng.permutation(b - a) for a, b in zip(r['off'][:-1], r['off'][1:])]).astype(np.int64)
    shuf = fc.calibrate_rows(r['off'], r['h'][perm], r['y'][perm], r['yhat'][perm], levels,
                             lower=r['lower'][:, perm] if cq else None, upper=r['upper'][:, perm] if cq else None, **kw)
    assert cr.same(shuf.q, base.q) and cr.same(shuf.n, base.n) and cr.same(shuf.status, base.status)
    for n in (3, 7, 11):                                # alone (another padded size, no list of series): the same bits
        s = slice(int(r['off'][n]), int(r['off'][n + 1]))
        one = fc.calibrate_rows([0, s.stop - s.start], r['h'][s], r['y'][s], r['yhat'][s], levels,
                                lower=r['lower'][:, s] if cq else None, upper=r['upper'][:, s] if cq else None, **kw)
        assert cr.same(one.q[0], base.q[n]) and cr.same(one.n[0], base.n[n]) and one.status[0] == base.status[n]


@pytest.mark.parametrize('mode', ['abs', 'cqr'])
def test_rule_without_rows(env, mode):
    """row_off[N] = 0: three series, no out-of-sample row -- nothing is copied in, every cell is empty"""
    fc, _lib = env
    none = np.zeros((2, 0))
    got = fc.calibrate_rows(np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0), [0.8, 0.95], mode=mode,
                            lower=none if mode == 'cqr' else None, upper=none if mode == 'cqr' else None, horizon=20 * DAY,
                            n_buckets=4, min_scores=3)
    assert got.q.shape == (3, 5, 2) and np.isnan(got.q).all() and not got.n.any()
    assert list(got.status) == [_lib.CALIB_NO_SCORES] * 3 and _lib.CALIB_NO_SCORES == -40


def test_rule_longest_series(env):
    """TSF_CALIB_MAX_ROWS rows and one row more than half of it: the launch class whose LDS goes beyond the default"""
    fc, _lib = env
    rng = np.random.default_rng(16)
    lens = [cr.MAX_ROWS, cr.MAX_ROWS // 2 + 1]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R = int(off[-1])
    h = rng.integers(-DAY, HZ + DAY, R)
    y = rng.normal(size=R)
    yhat = y + np.round(rng.normal(size=R), 2)          # (two decimals: ties)
    kw = dict(horizon=HZ, n_buckets=4, min_scores=5)
    got = fc.calibrate_rows(off, h, y, yhat, [0.8, 0.95], **kw)
    _same_table(got, cr.calibrate_rows(off, h, y, yhat, [0.8, 0.95], **kw))
    assert (got.status == _lib.CALIB_OK).all() and got.n[0, 4, 0] > 14000


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


def test_dev_variants_agree(env, rows):
    """tsf_calibrate_rows_dev and tsf_apply_calibration_dev on device pointers (plain hipMalloc blocks) == the host variants"""
    fc, _lib = env
    r = rows
    L = _lib.load()
    N, H = len(LENS), 5
    want = fc.calibrate_rows(r['off'], r['h'], r['y'], r['yhat'], [0.8, 0.95], horizon=r['H'], n_buckets=4, min_scores=5)
    rng = np.random.default_rng(17)
    fy, fut, org = rng.normal(size=(N, H)), DAY * np.array([-1, 1, 8, 16, 40], np.int64), np.zeros(N, np.int64)
    wlo, whi, wcell = want.apply(fy, fut, org, want_cell=True)
    hip = _hip_runtime()
    bufs = []

    def dev(a_):
        a_ = np.ascontiguousarray(a_)
        p_ = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p_), max(a_.nbytes, 8)) == 0
        bufs.append(p_)
        assert hip.hipMemcpy(p_, a_.ctypes.data, a_.nbytes, 1) == 0             # hipMemcpyHostToDevice
        return p_
    host = dict(q=np.zeros((N, 5, 2)), n=np.zeros((N, 5, 2), np.int32), status=np.zeros(N, np.int32),
                lo=np.zeros((N, 2, H)), hi=np.zeros((N, 2, H)), cell=np.zeros((N, 2, H), np.int8))
    try:
        d_off, d_h, d_y, d_yh = dev(r['off']), dev(r['h']), dev(r['y']), dev(r['yhat'])
        d_fy, d_fut, d_org = dev(fy), dev(fut), dev(org)
        o = {k: dev(v) for k, v in host.items()}
        tab = _lib.TsfCalibTable(o['q'], o['n'], o['status'])
        a = fc._calib_args([0.8, 0.95], 'abs', r['H'], 4, 5)
        ctx = fc.get_context()
        ctx.check(L.tsf_calibrate_rows_dev(ctx.handle, N, d_off, d_h, d_y, d_yh, None, None, ctypes.byref(a),
                                           ctypes.byref(tab), None))
        ctx.check(L.tsf_apply_calibration_dev(ctx.handle, N, H, d_fy, None, None, d_fut, 1, d_org, o['q'], o['n'],
                                              ctypes.byref(a), o['lo'], o['hi'], o['cell'], None))
        assert hip.hipDeviceSynchronize() == 0
        for k, v in host.items():
            assert hip.hipMemcpy(v.ctypes.data, o[k], v.nbytes, 2) == 0         # hipMemcpyDeviceToHost
    finally:
        for p_ in bufs:
            hip.hipFree(p_)
    for k, w in (('q', want.q), ('n', want.n), ('status', want.status), ('lo', wlo), ('hi', whi), ('cell', wcell)):
        assert cr.same(host[k], w), k


# ---- 2. apply ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['abs', 'cqr'])
def test_apply_bit_for_bit(env, mode):
    """H = 7 rows that straddle the origin, every bucket edge (w = 5 d) and the end of the horizon; a bucket below
    min_scores (the pooled cell), a series without scores (none), a NaN yhat; shared and per-series futures"""
    fc, _lib = env
    rng = np.random.default_rng(13)
    N, B, levels, ms = 3, 4, [0.8, 0.95], 6
    lens = [120, 4, 120]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R = int(off[-1])
    h = rng.integers(1, HZ + 1, size=R)
    h[:120][h[:120] > 15 * DAY] -= 15 * DAY             # series 0: the last bucket empty -> its rows take the pooled cell
    y, yhat = rng.normal(size=R), rng.normal(size=R)
    wid = np.array([6.0, 0.5])[:, None] * np.ones((1, R))         # (6.0: the scores of level 0 are negative under CQR)
    cq = mode == 'cqr'
    cal = fc.calibrate_rows(off, h, y, yhat, levels, lower=yhat - wid if cq else None, upper=yhat + wid if cq else None,
                            mode=mode, horizon=HZ, n_buckets=B, min_scores=ms)
    assert cal.status.tolist() == [_lib.CALIB_OK, _lib.CALIB_NO_SCORES, _lib.CALIB_OK] and (cal.n[0, 3] == 0).all()
    w = 5 * DAY
    ha = np.array([-DAY, 0, 1, w, w + 1, 2 * w, 2 * w + 1])
    hb = np.array([3 * w, 3 * w + 1, HZ, HZ + 1, 2 * HZ, 2 * w, 1])
    origin = np.array([1000 * DAY, 1010 * DAY, 990 * DAY + 7])
    H = 7
    fy = rng.normal(10, 1, (N, H))
    fy[2, 3] = np.nan
    flo = np.stack([fy - 6.0, fy - 0.5], axis=1)
    fhi = np.stack([fy + 6.0, fy + 0.5], axis=1)
    futures = {'per series': np.stack([origin[0] + ha, origin[1] + hb, origin[2] + hb]),
               'shared a': origin[0] + ha, 'shared b': origin[0] + hb}
    kw = dict(mode=_lib.CALIB_MODES[mode], horizon=HZ, n_buckets=B, min_scores=ms)
    cells = set()
    for what, fut in futures.items():
        lo, hi, cell = cal.apply(fy, fut, origin, lower=flo if cq else None, upper=fhi if cq else None, want_cell=True)
        wlo, whi, wcell = cr.apply(fy, fut, origin, cal.q, cal.n, levels, flo if cq else None, fhi if cq else None, **kw)
        assert cr.same(cell, wcell), what
        assert cr.same(lo, wlo) and cr.same(hi, whi), what
        cells |= set(cell[0].ravel().tolist())
        assert (cell[1] == -1).all() and np.isnan(lo[1]).all()
        lo2, hi2 = cal.apply(fy, fut, origin, lower=flo if cq else None, upper=fhi if cq else None)
        assert cr.same(lo2, lo) and cr.same(hi2, hi)
    assert cells == {0, 1, 2, 4}                          # every bucket with scores, and the pooled cell for the empty one
    if cq:
        assert (cal.q[0, :3, 0] < 0).all()                # the wide pair is narrowed, never past yhat
        lo, hi = cal.apply(fy, futures['shared a'], origin, lower=flo, upper=fhi)
        assert (lo[0, 0] <= fy[0]).all() and (hi[0, 0] >= fy[0]).all() and (lo[0, 0] > flo[0, 0]).all()


# ---- 3. the one call ---------------------------------------------------------------------------------------------------------

CV = dict(period=10 * DAY, initial=100 * DAY)
CV_FIELDS = ('status', 'n_folds', 'n_holdout', 'n_metric', 'fold_series', 'cutoff', 'hist_rows', 'hold_rows', 'row_fold',
             'row_index', 'ds', 'y', 'yhat', 'metric_series', 'horizon', 'mse', 'rmse', 'mae', 'mape')
FIT_FIELDS = ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval')


@pytest.fixture(scope='module')
def panels(env):
    """8 series x 200 daily rows (about 8 folds x 20 holdout rows each), and the same as a ragged panel: rows knocked out
    of series 1 and 4, series 6 too short for any cutoff"""
    fc, _lib = env
    from time_series_spark_amd import synth
    ds, y = synth.make_panel(8, 200, 'linear', seed=21)
    rng = np.random.default_rng(22)
    y = y + rng.normal(0, 0.02 * np.abs(y).mean(), y.shape)
    spec = fc.ModelSpec(growth='linear', seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3}])
    keep = np.ones((8, 200), bool)
    keep[1, rng.choice(np.arange(5, 195), 30, replace=False)] = False
    keep[4, 150:158] = False
    keep[6, 25:] = False
    lens = keep.sum(axis=1)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(spec=spec, ds=ds, y=y, off=off, ds_r=np.tile(ds, (8, 1))[keep], y_r=y[keep])


def _cv_ref(cv, levels, mode, _lib, lower=None, upper=None, **kw):
    t = cr.calibrate_rows(cv.row_offsets, cv.ds - cv.cutoff[cv.row_fold], cv.y, cv.yhat, levels, lower, upper,
                          mode=_lib.CALIB_MODES[mode], horizon=HZ, **kw)
    return cr.mask_series(t, np.asarray(cv.status) != 0)


@pytest.mark.parametrize('ragged', [False, True])
def test_calibrate_is_cross_validate_then_the_rule(env, panels, ragged):
    fc, _lib = env
    p = panels
    args = (p['spec'], p['ds_r'], p['y_r'], HZ) if ragged else (p['spec'], p['ds'], p['y'], HZ)
    kw = dict(offsets=p['off'] if ragged else None, **CV)
    levels, ckw = [0.8, 0.95], dict(n_buckets=4, min_scores=20)
    cal = fc.calibrate(*args, levels, want_cv=True, **ckw, **kw)
    cv = fc.cross_validate(*args, **kw)
    by_hand = fc.calibrate_cv(cv, levels, horizon=HZ, **ckw)
    assert cr.same(cal.q, by_hand.q) and cr.same(cal.n, by_hand.n) and cr.same(cal.status, by_hand.status)
    _same_table(cal, _cv_ref(cv, levels, 'abs', _lib, **ckw), 'ref')
    lean = fc.calibrate(*args, levels, **ckw, **kw)       # without the CV outputs: the same table
    assert lean.cv is None and cr.same(lean.q, cal.q) and cr.same(lean.n, cal.n) and cr.same(lean.status, cal.status)
    for k in CV_FIELDS:
        assert cr.same(np.asarray(getattr(cal.cv, k)), np.asarray(getattr(cv, k))), k
    for k in FIT_FIELDS:
        assert cr.same(getattr(cal.cv.fit, k), getattr(cv.fit, k)), k
    assert cal.cv.fit.grid.tobytes() == cv.fit.grid.tobytes() and cal.cv.yhat_lower is None
    good = [n for n in range(8) if not (ragged and n == 6)]
    assert (cal.status[good] == _lib.CALIB_OK).all() and (cal.n[good, 4, 0] >= 100).all()
    assert np.isfinite(cal.q[good]).all() and (cal.q[good, :, 1] >= cal.q[good, :, 0]).all()
    if ragged:                                            # too short for any cutoff
        assert cv.status[6] != 0 and cal.status[6] == _lib.CALIB_NO_SCORES and np.isnan(cal.q[6]).all() and (cal.n[6] == 0).all()
    # CQR with one level goes through the folds' own intervals
    ikw = dict(uncertainty_samples=200, interval_width=0.8, seed=5)
    cq = fc.calibrate(*args, [0.8], mode='cqr', want_cv=True, **ckw, **ikw, **kw)
    cvi = fc.cross_validate(*args, intervals=True, **ikw, **kw)
    for k in CV_FIELDS + ('yhat_lower', 'yhat_upper', 'coverage'):
        assert cr.same(np.asarray(getattr(cq.cv, k)), np.asarray(getattr(cvi, k))), k
    by_hand = fc.calibrate_cv(cvi, [0.8], mode='cqr', horizon=HZ, interval_width=0.8, **ckw)
    assert cr.same(cq.q, by_hand.q) and cr.same(cq.n, by_hand.n) and cr.same(cq.status, by_hand.status)
    _same_table(cq, _cv_ref(cvi, [0.8], 'cqr', _lib, cvi.yhat_lower[None], cvi.yhat_upper[None], **ckw), 'cqr ref')
    for bad in (dict(levels=[0.8, 0.9]), dict(levels=[0.9])):         # several levels, or not the interval's width
        with pytest.raises(ValueError):
            fc.calibrate(*args, bad['levels'], mode='cqr', **ckw, **ikw, **kw)


def test_calibrate_cv_cqr_with_two_levels(env, panels):
    fc, _lib = env
    p = panels
    cv = fc.cross_validate(p['spec'], p['ds'], p['y'], HZ, **CV)
    levels, ckw = [0.6, 0.9], dict(n_buckets=4, min_scores=20)
    cal = fc.calibrate_cv(cv, levels, mode='cqr', horizon=HZ, uncertainty_samples=200, seed=5, **ckw)
    s = fc.score_cv(cv, quantiles=fc.cv_interval_levels(levels), uncertainty_samples=200, seed=5)
    _same_table(cal, _cv_ref(cv, levels, 'cqr', _lib, s.q[:2], s.q[2:], **ckw))
    assert (cal.status == _lib.CALIB_OK).all() and np.isfinite(cal.q).all()


def test_predict_calibrated(env, panels):
    fc, _lib = env
    p = panels
    spec, ds, y = p['spec'], p['ds'], p['y']
    fit = fc.fit_aligned(spec, ds, y)
    fut = ds[-1] + DAY * np.arange(-2, 26)                # from inside the history to beyond the calibrated horizon
    origin = fc.model_origin_ns(fit.grid, len(y))
    assert (origin == ds[-1]).all()
    want_y = fc.predict(spec, fit.theta, fit.y_scale, fit.grid, fut)
    cal = fc.calibrate(spec, ds, y, HZ, [0.8, 0.95], n_buckets=4, **CV)
    yhat, lo, hi, cell = fc.predict_calibrated(spec, fit.theta, fit.y_scale, fit.grid, fut, cal, want_cell=True)
    assert cr.same(yhat, want_y)
    wlo, whi, wcell = cr.apply(want_y, fut, origin, cal.q, cal.n, cal.levels, mode=cr.ABS, horizon=HZ, n_buckets=4, min_scores=20)
    assert cr.same(lo, wlo) and cr.same(hi, whi) and cr.same(cell, wcell)
    assert (lo[:, 1] <= lo[:, 0]).all() and (hi[:, 1] >= hi[:, 0]).all() and (lo[:, 0] < want_y).all()
    cv = fc.cross_validate(spec, ds, y, HZ, **CV)
    calq = fc.calibrate_cv(cv, [0.6, 0.9], mode='cqr', horizon=HZ, n_buckets=4, uncertainty_samples=200, seed=5)
    yhat, lo, hi = fc.predict_calibrated(spec, fit.theta, fit.y_scale, fit.grid, fut, calq, uncertainty_samples=200, seed=9)
    pq = fc.predict_quantiles(spec, fit.theta, fit.y_scale, fit.grid, fut, fc.cv_interval_levels([0.6, 0.9]), uncertainty_samples=200, seed=9)
    assert cr.same(yhat, want_y) and cr.same(pq.yhat, want_y)
    wlo, whi, _ = cr.apply(want_y, fut, origin, calq.q, calq.n, calq.levels, np.ascontiguousarray(pq.q[:, :2]),
                           np.ascontiguousarray(pq.q[:, 2:]), mode=cr.CQR, horizon=HZ, n_buckets=4, min_scores=20)
    assert cr.same(lo, wlo) and cr.same(hi, whi)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(env):
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    N = 2
    off = np.array([0, 30, 60], np.int64)
    rng = np.random.default_rng(14)
    h = rng.integers(1, HZ, 60)
    y, yh = rng.normal(size=60), rng.normal(size=60)
    lo, hi = (yh - 1)[None, :].copy(), (yh + 1)[None, :].copy()
    q, cnt, st = np.zeros((N, 5, 1)), np.zeros((N, 5, 1), np.int32), np.zeros(N, np.int32)

    def call(off_=off, h_=h, y_=y, yh_=yh, lo_=None, hi_=None, q_=q, n_=cnt, st_=st, tab=True, args=True, **kw):
        a = fc._calib_args([0.8], 'abs', HZ, 4, 5)
        for k, v in kw.items():
            if k == 'level':
                a.levels[0] = v
            else:
                setattr(a, k, v)
        t = _lib.TsfCalibTable(_lib._ptr(q_), _lib._ptr(n_), _lib._ptr(st_))
        return L.tsf_calibrate_rows(ctx.handle, N, _lib._ptr(off_), _lib._ptr(h_), _lib._ptr(y_), _lib._ptr(yh_),
                                    _lib._ptr(lo_), _lib._ptr(hi_), ctypes.byref(a) if args else None,
                                    ctypes.byref(t) if tab else None)
    for bad in (dict(off_=None), dict(h_=None), dict(y_=None), dict(yh_=None), dict(q_=None), dict(n_=None), dict(st_=None),
                dict(tab=False), dict(args=False), dict(mode=2), dict(mode=-1), dict(n_levels=0), dict(n_levels=17),
                dict(level=0.0), dict(level=1.0), dict(level=float('nan')), dict(level=-0.1), dict(n_buckets=0),
                dict(n_buckets=65), dict(min_scores=0), dict(horizon_ns=0), dict(horizon_ns=-5),
                dict(mode=_lib.CALIB_CQR), dict(mode=_lib.CALIB_CQR, lo_=lo), dict(mode=_lib.CALIB_CQR, hi_=hi),
                dict(off_=np.array([0, 40, 30], np.int64)), dict(off_=np.array([1, 30, 60], np.int64))):
        assert call(**bad) < 0, bad
        assert len(L.tsf_last_error(ctx.handle)) > 0
        assert call() == 0, bad                         # the next call on the same context succeeds
    assert call(mode=_lib.CALIB_CQR, lo_=lo, hi_=hi) == 0
    a = fc._calib_args([0.8], 'abs', HZ, 4, 5)
    t = _lib.TsfCalibTable(_lib._ptr(q), _lib._ptr(cnt), _lib._ptr(st))
    assert L.tsf_calibrate_rows(ctx.handle, 0, _lib._ptr(off), _lib._ptr(h), _lib._ptr(y), _lib._ptr(yh), None, None,
                                ctypes.byref(a), ctypes.byref(t)) == 0         # no series: a legal no-op
    # apply refuses NULL inputs and CQR without bounds
    fy, fut, org = np.zeros((N, 3)), np.arange(3, dtype=np.int64), np.zeros(N, np.int64)
    olo, ohi = np.zeros((N, 1, 3)), np.zeros((N, 1, 3))

    def apply(fy_=fy, fut_=fut, org_=org, olo_=olo, mode=_lib.CALIB_ABS):
        a = fc._calib_args([0.8], mode, HZ, 4, 5)
        return L.tsf_apply_calibration(ctx.handle, N, 3, _lib._ptr(fy_), None, None, _lib._ptr(fut_), 1, _lib._ptr(org_),
                                       _lib._ptr(q), _lib._ptr(cnt), ctypes.byref(a), _lib._ptr(olo_), _lib._ptr(ohi), None)
    for bad in (dict(fy_=None), dict(fut_=None), dict(org_=None), dict(olo_=None), dict(mode=_lib.CALIB_CQR)):
        assert apply(**bad) < 0, bad
        assert apply() == 0, bad
    got = fc.calibrate_rows(off, h, y, yh, [0.8], horizon=HZ, n_buckets=4, min_scores=5)
    _same_table(got, cr.calibrate_rows(off, h, y, yh, [0.8], horizon=HZ, n_buckets=4, min_scores=5))


def test_calibrate_refuses_another_horizon(env, panels):
    fc, _lib = env
    p = panels
    L = _lib.load()
    ctx = fc.get_context()
    spec, N, T = p['spec'], 8, 200
    cs = spec.to_c()
    tab, _ = fc._alloc_calib(N, 4, 1)
    y = np.ascontiguousarray(p['y'])
    for cal_h, mode, ns, ok in ((HZ - 1, 'abs', 0, False), (HZ, 'cqr', 0, False), (HZ, 'abs', 0, True)):
        a = fc._calib_args([0.8], mode, cal_h, 4, 20)
        ca = fc._cv_args(HZ, CV['period'], CV['initial'], 0.1)
        rc = L.tsf_calibrate(ctx.handle, ctypes.byref(cs), N, T, None, p['ds'].ctypes.data, y.ctypes.data, _lib.Y_F64, None,
                             None, None, ctypes.byref(ca), None, ns, 0.8, 0, ctypes.byref(a), ctypes.byref(tab), None)
        assert (rc == 0) == ok, (cal_h, mode, rc)
    # an algorithm outside the enum is refused up front, by tsf_calibrate and by tsf_cross_validate (one path)
    bad = fc.ModelSpec(algorithm=7, **{k: v for k, v in spec.to_dict().items() if k != 'lbfgs'})
    for call in (lambda: fc.calibrate(bad, p['ds'], y, HZ, [0.8], **CV), lambda: fc.cross_validate(bad, p['ds'], y, HZ, **CV)):
        with pytest.raises(_lib.TsfError, match='bad algorithm'):
            call()


# ---- 5. plain C ----------------------------------------------------------------------------------------------------------------

def test_abi_calibrate_plain_c(env, panels, tmp_path):
    """tests/c/abi_calibrate.c drives tsf_calibrate_rows, tsf_apply_calibration and tsf_calibrate from plain C99"""
    fc, _lib = env
    p = panels
    d = str(tmp_path)
    rng = np.random.default_rng(15)
    N, T, H = 8, 200, 6
    lens = rng.integers(20, 90, N)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R = int(off[-1])
    h = rng.integers(-DAY, HZ + DAY, R)
    y, yh = rng.normal(size=R), rng.normal(size=R)
    fut = 500 * DAY + DAY * np.array([-1, 1, 5, 6, 20, 30], np.int64)
    origin = np.full(N, 500 * DAY, np.int64)
    fy = rng.normal(size=(N, H))
    for name, a in (('off.i64', off), ('h.i64', h), ('y.f64', y), ('yhat.f64', yh), ('fut.i64', fut), ('origin.i64', origin),
                    ('fyhat.f64', fy), ('ds.i64', p['ds']), ('panel.f64', p['y'])):
        np.ascontiguousarray(a).tofile(d + '/' + name)
    exe = d + '/abi_calibrate'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_calibrate.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(N), str(T), str(H), d])
    got = np.fromfile(d + '/out.f64')
    kw = dict(n_buckets=4, min_scores=5)
    rule = fc.calibrate_rows(off, h, y, yh, [0.8, 0.95], horizon=HZ, **kw)
    lo, hi, cell = rule.apply(fy, fut, origin, want_cell=True)
    spec = fc.ModelSpec(growth='linear', seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3}])
    one = fc.calibrate(spec, p['ds'], p['y'], HZ, [0.8, 0.95], **kw, **CV)
    f64 = lambda a: np.asarray(a, dtype=np.float64).ravel()     # noqa: E731
    want = np.concatenate([f64(rule.q), f64(rule.n), f64(rule.status), f64(lo), f64(hi), f64(cell), f64(one.q), f64(one.n),
                           f64(one.status)])
    assert got.shape == want.shape and cr.same(got, want)
    assert (one.status == 0).all() and (rule.status == 0).all()


# ---- 6. the jobs ---------------------------------------------------------------------------------------------------------------

def test_validator_then_scorer(env, tmp_path):
    """the validator writes io.calibration; the scorer's forecast.calibration columns are Calibration.apply on the float64
    forecast of every model, NaN for a model without a table row; with neither key set both jobs' outputs are what
    they are without the feature"""
    fc, _lib = env
    from time_series_spark_amd import panel as pk, synth
    from time_series_spark_amd.jobs import prophet_modeler as pm, prophet_scorer as ps, prophet_validator as pv
    N, T, H = 6, 200, 25
    ds, y = synth.make_panel(N, T, 'linear', seed=31)
    y = np.rint(y + np.random.default_rng(32).normal(0, 0.03 * np.abs(y).mean(), y.shape)).astype(np.int64)
    stamps = pd.DatetimeIndex(ds.astype('datetime64[ns]')).strftime('%Y-%m-%d %H:%M:%S').values
    for n in range(N):
        d = tmp_path / 'in' / ('series_id=%d' % (40 + n))
        d.mkdir(parents=True)
        (d / 'part-0.csv').write_text('\n'.join('1,%s,%d' % (s, v) for s, v in zip(stamps, y[n])) + '\n')
    prophet = {'growth': 'linear', 'seasonality_mode': 'additive', 'yearly_seasonality': False, 'daily_seasonality': False}
    model = {'floor': 0, 'cap_multiplier': 1.1, 'prophet': prophet}

    def vcfg(tag, calibrate):
        io = {'input': str(tmp_path / 'in'), 'metrics': str(tmp_path / ('m' + tag)), 'folds': str(tmp_path / ('f' + tag))}
        out = {'model': model, 'io': io, 'cv': {'horizon': '20 days', 'period': '10 days', 'initial': '100 days'}}
        if calibrate:
            io['calibration'] = str(tmp_path / ('c' + tag))
            out['calibrate'] = {'levels': [0.8, 0.95], 'n_buckets': 4, 'min_scores': 10}
        return out
    pv.ProphetValidator.validate(None, vcfg('0', False), return_frame=False)
    pv.ProphetValidator.validate(None, vcfg('1', True), return_frame=False)
    for k in ('m', 'f'):                                  # the other outputs are byte for byte those of a run without
        a, b = (open(str(tmp_path / (k + t) / 'part-00000.parquet'), 'rb').read() for t in '01')
        assert a == b, k
    assert not os.path.exists(str(tmp_path / 'c0'))
    table = pd.read_parquet(str(tmp_path / 'c1'))
    assert list(table.columns[:8]) == ['series_id', 'dim_id', 'bucket', 'horizon_upto', 'n_c80', 'n_c95', 'q_c80', 'q_c95']
    assert len(table) == N * 5 and table['series_id'].tolist() == list(np.repeat(40 + np.arange(N), 5))
    cal, keys = fc.Calibration.from_frame(table)
    assert (cal.status == 0).all() and (cal.mode, cal.horizon, cal.n_buckets, cal.min_scores) == (_lib.CALIB_ABS, HZ, 4, 10)
    with pytest.raises(ValueError):
        pv.ProphetValidator.validate(None, dict(vcfg('2', False), calibrate={'levels': [0.8]}), return_frame=False)
    # the table without series 43, then the scorer
    short = str(tmp_path / 'c_short')
    os.makedirs(short)
    table[table['series_id'] != 43].to_parquet(os.path.join(short, 'part-00000.parquet'), index=False)
    mcfg = {'io': {'input': str(tmp_path / 'in'), 'models': str(tmp_path / 'models')}, 'model': model}
    pm.ProphetModeler.model(None, mcfg, return_frame=False)
    models = pd.read_parquet(mcfg['io']['models']).sort_values(['series_id', 'dim_id']).reset_index(drop=True)
    base = {'forecast': {'periods': H, 'frequency': 'D'}}
    plain = ps.forecast_panel(base)(models)
    got = ps.forecast_panel({'forecast': dict(base['forecast'], calibration=short)})(models)
    new = ['yhat_lower_c80', 'yhat_lower_c95', 'yhat_upper_c80', 'yhat_upper_c95']
    assert list(got.columns) == list(plain.columns) + new and all(got[c].dtype == np.float64 for c in new)
    for c in plain.columns:
        assert np.array_equal(got[c].values, plain[c].values), c
    sids = models['series_id'].to_numpy()
    seen = 0
    for spec_dict, idx, rec in pk.load_models(models['model'].tolist()):
        spec = fc.ModelSpec.from_dict(spec_dict)
        theta = np.zeros((len(idx), spec.theta_stride))
        theta[:, :rec['theta'].shape[1]] = rec['theta']
        grid = pk.grid_from_records(rec)
        fut = pk.future_dates(rec['last_ds_ns'], H, 'D')
        yhat = fc.predict(spec, theta, rec['y_scale'], grid, fut, floor=models['floor'].to_numpy(np.float64)[idx],
                          cap=models['cap'].to_numpy(np.float64)[idx])
        for j, i in enumerate(idx):
            rows = got[got['series_id'] == sids[i]]
            assert len(rows) == H
            seen += 1
            if sids[i] == 43:
                assert rows[new].isna().all().all()
                continue
            at = int(np.flatnonzero(keys['series_id'].to_numpy() == sids[i])[0])
            one = fc.Calibration(cal.q[at:at + 1], cal.n[at:at + 1], cal.status[at:at + 1], cal.levels, cal.mode,
                                 cal.horizon, cal.n_buckets, cal.min_scores)
            lo, hi = one.apply(yhat[j:j + 1], fut[j], fc.model_origin_ns(grid, len(idx))[j:j + 1])
            for l, p_ in enumerate(('80', '95')):
                assert cr.same(rows['yhat_lower_c' + p_].to_numpy(), lo[0, l]) and cr.same(rows['yhat_upper_c' + p_].to_numpy(), hi[0, l])
            assert np.isfinite(lo).all() and (lo[0, 1] <= lo[0, 0]).all()
    assert seen == N
