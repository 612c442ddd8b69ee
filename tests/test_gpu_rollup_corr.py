"""GPU tests of the correlated group roll-ups (include/tsf.h "correlated group roll-ups"): tsf_residual_corr / _dev
(corr_scale_kernel, corr_rows_kernel, corr_group_kernel) bit for bit against tests/corr_ref.py, and
tsf_rollup_set_noise_corr's add route (rollup_noise_scale_kernel, rollup_add_corr_kernel) against the independent
roll-up, the restated factor term and the draw's laws.

The members of the draw tests are tests/sampler_cases.py's noise-only model ('no_cp': linear growth, no changepoint,
k = m = 0, one additive extra column, sigma = 0.05) on its first rows, with two y_scales (250 and 60, so sn = sigma *
y_scale is 12.5 and 3.0) alternating over the series.  Its sampled trend is the deviation itself at lam = 1e-8: of the
order 1e-9 * y_scale, nine orders below the noise, so a group's summed draw minus its summed yhat is its summed noise
for every statistic here.  Thresholds: tests/sampler_ref.py's Z_MAX = 5.5 and P_MIN = 1e-7."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import corr_ref as cr, helpers, sampler_cases as sc, sampler_ref as sr
from tests import test_gpu_rollup as tr

pytestmark = pytest.mark.gpu

SEED = tr.SEED
LEVELS = tr.LEVELS
_bits = tr._bits


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU roll-up tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _same(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the estimator, bit for bit ---------------------------------------------------------------------------------

EST_FIELDS = ('rho', 'rho_raw', 'n_pairs', 'n_used', 'status', 'scale')


def _estimator_panel(T, dtype, seed=21):
    """N = 37 series in G = 6 groups: 10, 9 and 8 members with a planted common factor, a singleton (group 3), an empty
    group (4), 7 members in group 5, two series with group -1; one series with NaN rows (in fitted, and in y where the
    dtype has a NaN), one constant-residual series, one zero-residual series -> (y, fitted, group)"""
    rng = np.random.default_rng(seed)
    group = np.array([0] * 10 + [1] * 9 + [2] * 8 + [3] + [5] * 7 + [-1, -1], dtype=np.int64)
    rng.shuffle(group)
    N = len(group)
    assert N == 37
    f = rng.normal(0, 1, (7, T))
    load = np.array([0.8, 0.3, 0.0, 0.5, 0.0, 0.6, 0.9])
    e = load[group, None] * f[group] + rng.normal(0, 1, (N, T))
    fitted = 100.0 + 10.0 * rng.normal(0, 1, (N, T))
    y = fitted + e * rng.uniform(1.0, 30.0, (N, 1))
    y = np.rint(y).astype(np.int32) if dtype == np.int32 else y.astype(dtype)
    i, j, k = (int(np.flatnonzero(group == g)[n]) for g, n in ((0, 1), (1, 0), (5, 2)))
    fitted[i, T // 3:T // 2 + 1] = np.nan
    if dtype != np.int32:
        y[i, -1] = np.nan
    fitted[j] = y[j].astype(np.float64) - 2.0           # a constant residual: scale 2, e = 1 on every row
    fitted[k] = y[k].astype(np.float64)                 # a zero residual: unused
    return y, fitted, group


@pytest.mark.parametrize('T', [70, 1, 129])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.int32], ids=['f64', 'f32', 'i32'])
def test_estimator_bit_for_bit(env, dtype, T):
    fc, _lib = env
    y, fitted, group = _estimator_panel(T, dtype)
    for kw in (dict(), dict(rho_max=0.4, min_rows=2)):
        want = cr.residual_corr(y, fitted, group, 6, **kw)
        got = fc.residual_correlation(y, fitted, group, 6, **kw)
        for k in EST_FIELDS:
            assert _same(getattr(got, k), want[k]), (k, kw, getattr(got, k), want[k])
    if T >= 8:
        assert list(got.status) == [0, 0, 0, _lib.CORR_NO_PAIRS, _lib.CORR_NO_PAIRS, 0]
        assert list(got.n_used) == [10, 9, 8, 1, 0, 6] and np.isnan(got.scale).sum() == 1
        assert got.rho[0] > 0.2 and got.rho.max() <= 0.4
    else:
        assert (got.status == _lib.CORR_NO_PAIRS).all() and np.isnan(got.scale).all()
    assert list(got.frame().columns) == ['group', 'rho', 'rho_raw', 'n_pairs', 'n_used', 'status']


def test_estimator_without_series(env):
    """N = 0: nothing is copied in, every group is without pairs, and scale has no element to copy back"""
    fc, _lib = env
    got = fc.residual_correlation(np.zeros((0, 40)), np.zeros((0, 40)), np.zeros(0, np.int64), 3)
    assert list(got.status) == [_lib.CORR_NO_PAIRS] * 3 and _lib.CORR_NO_PAIRS == -50
    assert list(got.rho) == [0.0] * 3 and np.isnan(got.rho_raw).all()
    assert list(got.n_pairs) == [0] * 3 and list(got.n_used) == [0] * 3 and got.scale.shape == (0,)


def test_estimator_dev_variant_agrees(env):
    """tsf_residual_corr_dev on device pointers (plain hipMalloc blocks; group on the host) == the host variant"""
    fc, _lib = env
    from tests.test_gpu_screen import _hip_runtime
    y, fitted, group = _estimator_panel(70, np.float64)
    N, T, G = 37, 70, 6
    want = fc.residual_correlation(y, fitted, group, G)
    hip = _hip_runtime()
    bufs = []

    def dev(a_):
        a_ = np.ascontiguousarray(a_)
        p_ = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p_), max(a_.nbytes, 8)) == 0
        bufs.append(p_)
        assert hip.hipMemcpy(p_, a_.ctypes.data, a_.nbytes, 1) == 0             # hipMemcpyHostToDevice
        return p_
    host = dict(rho=np.full(G, 7.0), rho_raw=np.zeros(G), n_pairs=np.zeros(G, np.int64), n_used=np.zeros(G, np.int32),
                status=np.full(G, 7, np.int32), scale=np.zeros(N))
    try:
        d_y, d_f = dev(y), dev(fitted)
        o = {k: dev(v) for k, v in host.items()}
        out = _lib.TsfCorrOut(*[o[k] for k in EST_FIELDS])
        ctx = fc.get_context()
        ctx.check(_lib.load().tsf_residual_corr_dev(ctx.handle, N, T, d_y, _lib.Y_F64, d_f, group.ctypes.data, G, None,
                                                    ctypes.byref(out), None))
        assert hip.hipDeviceSynchronize() == 0
        for k, v in host.items():
            assert hip.hipMemcpy(v.ctypes.data, o[k], v.nbytes, 2) == 0         # hipMemcpyDeviceToHost
    finally:
        for p_ in bufs:
            hip.hipFree(p_)
    for k in EST_FIELDS:
        assert _same(host[k], getattr(want, k)), k


# ---- the members of the draw tests -----------------------------------------------------------------------------------

def _noise_members(N, rows, key0=3):
    """N series of sampler_cases' noise-only model on the given rows of its calendar -> (Members, calendar, extra, sn)"""
    c = sc.make('no_cp')
    m = tr.Members()
    m.spec, m.N, m.cap = c.spec, N, None
    m.theta = np.tile(c.theta[:1], (N, 1))
    m.y_scale = np.where(np.arange(N) % 2 == 0, 250.0, 60.0)
    m.grid = np.repeat(c.grid, N)
    m.floor = np.zeros(N)
    m.keys = 7919 * np.arange(N, dtype=np.int64) + key0
    rows = np.asarray(rows)
    sn = np.exp(m.theta[:, 2]) * m.y_scale
    return m, np.ascontiguousarray(c.fut[rows]), np.ascontiguousarray(c.extra[:, rows]), sn


@pytest.fixture(scope='module')
def iv129(env):
    """test_gpu_rollup's members: 129 series of iv129's model on 2 rows, groups n % 5, series 128 alone in group 5,
    group 6 empty; the independent roll-up's samples, yhat and quantiles at 300 samples"""
    fc, _lib = env
    m, c = tr._tiled('iv129', 129, seed=11)
    d = dict(m=m, cal=np.ascontiguousarray(c.fut[:2]), extra=np.ascontiguousarray(c.extra[:, :2]), G=7, S=300)
    d['group'] = np.arange(129, dtype=np.int64) % 5
    d['group'][128] = 5
    with fc.Rollup(d['cal'], 7, uncertainty_samples=300, seed=SEED) as roll:
        tr._add(roll, m, d['group'], d['extra'])
        d['samples'], d['r'] = roll.samples(), roll.quantiles(LEVELS, cumulative=True)
    for v in (d['samples'], d['group']):
        v.setflags(write=False)
    return d


def _equal_to(roll, samples, r, groups=slice(None)):
    got = roll.quantiles(LEVELS, cumulative=True)
    return (_bits(roll.samples()[groups], samples[groups]) and _bits(got.yhat[groups], r.yhat[groups])
            and _bits(got.q[groups], r.q[groups]) and _bits(got.cum_q[groups], r.cum_q[groups])
            and np.array_equal(got.count[groups], r.count[groups]))


# ---- 2. rho = 0 is today's roll-up -------------------------------------------------------------------------------------

def test_rho_zero_is_the_independent_rollup(env, iv129):
    fc, _lib = env
    d = iv129
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=np.zeros(7)) as roll:
        tr._add(roll, d['m'], d['group'], d['extra'])
        assert _equal_to(roll, d['samples'], d['r'])
    rho = np.zeros(7)
    rho[0] = 0.5
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=rho) as roll:
        tr._add(roll, d['m'], d['group'], d['extra'])
        assert _equal_to(roll, d['samples'], d['r'], slice(1, None))
        got = roll.samples()
        assert _bits(roll.quantiles(LEVELS).yhat, d['r'].yhat)                    # ysum is carried as always
    assert (got[0] != d['samples'][0]).mean() > 0.99
    # 26 members, rho = 0.5: the spread of the total grows (variance factor 1 + 25 * 0.5 on the noise part)
    assert (got[0].std(axis=-1) > d['samples'][0].std(axis=-1)).all()


# ---- 3. the draw against the restatement -----------------------------------------------------------------------------

def test_draw_against_the_restatement(env):
    """acc_corr - acc_indep per cell against numpy's sum over the members of (a z_i + b w) sn_i, within 1e-12 * m *
    max sn: the tolerance with which test_sampler_ref.py ties the numpy streams to the oracle's deterministic recipes
    (libm against them), summed over the m members.  m = 5 with two scales, 3 unsorted rows, 300 samples; a second group
    with rho = 0 rides along."""
    fc, _lib = env
    m, cal, extra, sn = _noise_members(8, [2, 0, 1])
    assert cal[0] > cal[1] and len(set(sn[:5])) == 2
    group = np.array([0, 0, 0, 0, 0, 1, 1, 1], dtype=np.int64)
    gkey = np.array([1001, 1002], dtype=np.int64)
    acc = []
    for corr in (None, np.array([0.6, 0.0])):
        with fc.Rollup(cal, 2, uncertainty_samples=300, seed=SEED, noise_corr=corr, group_key=None if corr is None else gkey) as roll:
            tr._add(roll, m, group, extra)
            acc.append(roll.samples())
    want = cr.corr_term(SEED, m.keys[:5], 1001, 0.6, sn[:5], 300, 3)
    err = np.abs((acc[1][0] - acc[0][0]) - want).max()
    tol = 1e-12 * 5 * sn.max()
    print('largest deviation %.3g, tolerance %.3g, largest term %.3g' % (err, tol, np.abs(want).max()))
    assert np.abs(want).max() > 10.0
    assert err <= tol
    assert _bits(acc[1][1], acc[0][1])
    # the default group key is the group index
    with fc.Rollup(cal, 2, uncertainty_samples=300, seed=SEED, noise_corr=[0.6, 0.0]) as roll:
        tr._add(roll, m, group, extra)
        got = roll.samples()
    want0 = cr.corr_term(SEED, m.keys[:5], 0, 0.6, sn[:5], 300, 3)
    assert np.abs((got[0] - acc[0][0]) - want0).max() <= tol


# ---- 4. laws on the device ---------------------------------------------------------------------------------------------

NS, H = 4096, 8
LAW_GROUPS = [(8, 0.3), (8, 0.9), (2, 0.3), (2, 0.9), (1, 0.9), (1, 0.9)]       # (members, rho) per group


@pytest.fixture(scope='module')
def law_draws(env):
    """per seed (SEED, SEED + 1): the standardised summed noise [G][H][NS] of LAW_GROUPS' groups, and the variance laws"""
    fc, _lib = env
    sizes = [m for m, _ in LAW_GROUPS]
    rho = np.array([r for _, r in LAW_GROUPS])
    N, G = sum(sizes), len(sizes)
    m, cal, extra, sn = _noise_members(N, np.arange(H))
    group = np.repeat(np.arange(G, dtype=np.int64), sizes)
    var = np.array([cr.group_variance(rho[g], sn[group == g]) for g in range(G)])
    assert all(len(set(sn[group == g])) == 2 for g in range(4))                 # two scales within a group
    out = {'var': var}
    for seed in (SEED, SEED + 1):
        with fc.Rollup(cal, G, uncertainty_samples=NS, seed=seed, noise_corr=rho) as roll:
            roll.add(m.spec, m.theta, m.y_scale, m.grid, group, m.keys, floor=m.floor, extra_future=extra)
            x = roll.samples() - roll.quantiles([0.5]).yhat[:, :, None]
        out[seed] = x / np.sqrt(var)[:, None, None]
        out[seed].setflags(write=False)
    return out


def test_laws_on_the_device(env, law_draws):
    x = law_draws[SEED]
    res = []
    for g, (m, rho) in enumerate(LAW_GROUPS):
        # the sample variance over the 4096 draws, pooled over the rows: relative standard error sqrt(2 / (8 * 4095))
        v = x[g].var(axis=-1, ddof=1).mean()
        res.append(('variance[%d: m=%d rho=%.1f]' % (g, m, rho), 'z', (v - 1.0) / math.sqrt(2.0 / (H * (NS - 1)))))
        res.append(('ks[%d]' % g, 'p', sr.ks_normal(x[g])))
        res.append(sr.corr_stat('rows[%d]' % g, x[g][:-1], x[g][1:]))
        res.append(sr.corr_stat('samples[%d]' % g, x[g][:, :-1], x[g][:, 1:]))
    for a, b in ((0, 1), (0, 2), (1, 3), (4, 5)):
        res.append(sr.corr_stat('groups[%d, %d]' % (a, b), x[a], x[b]))
    # singleton groups with rho = 0.9: N(0, 1) noise (variance and KS above) and, against a second seed, no correlation
    for g in (4, 5):
        res.append(sr.corr_stat('seeds[%d]' % g, x[g], law_draws[SEED + 1][g]))
    for name, kind, val in res:
        print('%-32s %s %.4g' % (name, kind, val))
    assert not sr.failures(res)


def test_laws_reject_the_independent_rollup(env, law_draws):
    """the same statistic on a handle without a correlation: the groups of 8 and of 2 miss the law by far (a test that
    cannot fail shows nothing)"""
    fc, _lib = env
    sizes = [m for m, _ in LAW_GROUPS]
    N, G = sum(sizes), len(sizes)
    m, cal, extra, sn = _noise_members(N, np.arange(H))
    group = np.repeat(np.arange(G, dtype=np.int64), sizes)
    with fc.Rollup(cal, G, uncertainty_samples=NS, seed=SEED) as roll:
        roll.add(m.spec, m.theta, m.y_scale, m.grid, group, m.keys, floor=m.floor, extra_future=extra)
        x = (roll.samples() - roll.quantiles([0.5]).yhat[:, :, None]) / np.sqrt(law_draws['var'])[:, None, None]
    for g in range(4):
        v = x[g].var(axis=-1, ddof=1).mean()
        assert abs(v - 1.0) / math.sqrt(2.0 / (H * (NS - 1))) > sr.Z_MAX
    for g in (4, 5):                                    # a singleton's law does not depend on rho
        v = x[g].var(axis=-1, ddof=1).mean()
        assert abs(v - 1.0) / math.sqrt(2.0 / (H * (NS - 1))) <= sr.Z_MAX


# ---- 5. order and chunking -----------------------------------------------------------------------------------------------

def test_one_add_equals_two_adds_of_halves(env, iv129):
    fc, _lib = env
    d = iv129
    m, group = d['m'], d['group']
    rho = np.array([0.5, 0.0, 0.9, 0.1, 1.0, 0.3, 0.7])
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=rho) as roll:
        tr._add(roll, m, group, d['extra'])
        one, r1 = roll.samples(), roll.quantiles(LEVELS, cumulative=True)
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=rho) as roll:
        tr._add(roll, m.take(slice(0, 64)), group[:64], d['extra'])
        tr._add(roll, m.take(slice(64, 129)), group[64:], d['extra'])
        assert _equal_to(roll, one, r1)
    assert _bits(one[1], d['samples'][1]) and not _bits(one[0], d['samples'][0])
    # 40 unrelated series in the same call, in the spare group: the other groups do not see them
    other, _ = tr._tiled('iv129', 40, seed=99, key0=5 * 10 ** 6)
    both = tr.Members()
    both.spec, both.N, both.cap = m.spec, m.N + other.N, None
    for k in ('theta', 'y_scale', 'grid', 'floor', 'keys'):
        setattr(both, k, np.concatenate([getattr(m, k), getattr(other, k)]))
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=rho) as roll:
        tr._add(roll, both, np.concatenate([group, np.full(40, 6, dtype=np.int64)]), d['extra'])
        assert _bits(roll.samples()[:6], one[:6])


def test_groups_across_scratch_chunks(env):
    """test_gpu_rollup.test_groups_across_scratch_chunks' shape with a correlation set: 90 series x 960 rows x 1000
    samples run as 2 scratch chunks (69 + 21); group 3 = series 60 .. 71 straddles the boundary.  Against the same
    members added in two calls of 45 (one chunk each)."""
    fc, _lib = env
    m, c = tr._tiled('h960', 90, seed=9)
    m.keys = np.arange(90, dtype=np.int64) ^ 0x5555
    assert c.H == 960 and (512 << 20) // (8 * 960 * 1003) == 69
    group = np.arange(90, dtype=np.int64) % 3
    group[60:72] = 3
    rho = np.array([0.2, 0.0, 0.6, 0.8])
    with fc.Rollup(c.fut, 4, uncertainty_samples=1000, seed=SEED, noise_corr=rho) as roll:
        tr._add(roll, m, group)
        acc, yh = roll.samples(), roll.quantiles([0.5]).yhat
    with fc.Rollup(c.fut, 4, uncertainty_samples=1000, seed=SEED, noise_corr=rho) as roll:
        tr._add(roll, m.take(slice(0, 45)), group[:45])
        tr._add(roll, m.take(slice(45, 90)), group[45:])
        assert _bits(roll.samples(), acc) and _bits(roll.quantiles([0.5]).yhat, yh)
    with fc.Rollup(c.fut, 4, uncertainty_samples=1000, seed=SEED) as roll:
        tr._add(roll, m, group)
        indep = roll.samples()
    assert _bits(acc[1], indep[1]) and (acc[3] != indep[3]).mean() > 0.99


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

def test_refusals(env, iv129):
    """every refusal: < 0 with a message; the accumulators are bit for bit what they were, the handle goes on adding and
    the context goes on estimating"""
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    d = iv129
    m = d['m']

    def message():
        return L.tsf_last_error(ctx.handle).decode()

    y, fitted, group = _estimator_panel(70, np.float64)
    est0 = fc.residual_correlation(y, fitted, group, 6)
    # set_noise_corr: a bad rho on an empty handle, then a good one; after an add it is refused
    roll = fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED)
    for bad, why in (([0.1] * 6 + [1.5], 'rho[6]'), ([-0.1] + [0.1] * 6, 'rho[0]'), ([0.1, np.nan] + [0.1] * 5, 'rho[1]'),
                     ([np.inf] + [0.1] * 6, 'rho[0]')):
        a = np.array(bad, dtype=np.float64)
        rc = L.tsf_rollup_set_noise_corr(roll._h, a.ctypes.data, None)
        assert rc < 0 and why in message(), (why, message())
    assert L.tsf_rollup_set_noise_corr(roll._h, None, None) < 0 and 'rho' in message()
    tr._add(roll, d['m'], d['group'], d['extra'])
    assert _bits(roll.samples(), d['samples'])                 # the refused calls set nothing
    rho = np.full(7, 0.5)
    rc = L.tsf_rollup_set_noise_corr(roll._h, rho.ctypes.data, None)
    assert rc < 0 and 'after' in message()
    with pytest.raises(_lib.TsfError, match='after'):
        roll.set_noise_corr(rho)
    assert _bits(roll.samples(), d['samples'])
    roll.close()
    # the Python layer's own refusals
    for kw in (dict(noise_corr=[0.5] * 6), dict(noise_corr=[0.5] * 6 + [1.5]), dict(noise_corr=[0.5] * 6 + [np.nan]),
               dict(group_key=np.arange(7)), dict(noise_corr=[0.5] * 7, group_key=np.arange(6))):
        with pytest.raises(ValueError):
            fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, **kw)
    # set_totals / reconcile / reconciled_totals on a correlated handle
    roll = fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=rho)
    tr._add(roll, m.take(slice(0, 64)), d['group'][:64], d['extra'])
    before = roll.samples()
    tot = m.take(slice(0, 7))
    tkeys = 10 ** 9 + np.arange(7, dtype=np.int64)
    with pytest.raises(_lib.TsfError, match='noise correlation'):
        roll.set_totals(tot.spec, tot.theta, tot.y_scale, tot.grid, np.arange(7), tkeys, floor=tot.floor, extra_future=d['extra'])
    with pytest.raises(_lib.TsfError, match='noise correlation'):
        roll.reconcile(m.spec, m.theta, m.y_scale, m.grid, d['group'], m.keys, np.full(m.N, 0.5), quantiles=[0.5],
                       floor=m.floor, extra_future=d['extra'])
    with pytest.raises(_lib.TsfError, match='noise correlation'):
        roll.reconciled_totals(np.full(7, 0.5), [0.5])
    assert _bits(roll.samples(), before)
    # the handle is usable: the second half lands as in a handle that was never refused anything
    tr._add(roll, m.take(slice(64, 129)), d['group'][64:], d['extra'])
    after = roll.samples()
    roll.close()
    with fc.Rollup(d['cal'], d['G'], uncertainty_samples=d['S'], seed=SEED, noise_corr=rho) as ref:
        tr._add(ref, m, d['group'], d['extra'])
        assert _bits(ref.samples(), after)
    # the estimator's refusals
    p = lambda v: None if v is None else v.ctypes.data     # noqa: E731
    out_bufs = dict(rho=np.full(6, 7.0), rho_raw=np.zeros(6), n_pairs=np.zeros(6, np.int64), n_used=np.zeros(6, np.int32),
                    status=np.full(6, 7, np.int32), scale=np.zeros(37))

    def est(N=37, T=70, y=y, dtype=_lib.Y_F64, fitted=fitted, group=group, G=6, rho_max=0.95, min_rows=8, want=EST_FIELDS,
            out=True):
        a = _lib.TsfCorrArgs(rho_max, min_rows, 0)
        o = _lib.TsfCorrOut(**{k: out_bufs[k].ctypes.data for k in want})
        return L.tsf_residual_corr(ctx.handle, N, T, p(y), dtype, p(fitted), p(group), G, ctypes.byref(a),
                                   ctypes.byref(o) if out else None)

    hi, lo = group.copy(), group.copy()
    hi[30], lo[4] = 6, -2
    for kw, why in ((dict(group=hi), 'group[30]'), (dict(group=lo), 'group[4]'), (dict(rho_max=1.5), 'rho_max'),
                    (dict(rho_max=-0.1), 'rho_max'), (dict(rho_max=float('nan')), 'rho_max'), (dict(min_rows=1), 'min_rows'),
                    (dict(dtype=3), 'y_dtype'), (dict(dtype=-1), 'y_dtype'), (dict(T=0), 'T'), (dict(G=0), 'G'),
                    (dict(y=None), 'NULL'), (dict(fitted=None), 'NULL'), (dict(group=None), 'NULL'), (dict(out=False), 'NULL'),
                    (dict(want=('rho_raw', 'status')), 'rho'), (dict(want=('rho',)), 'status'), (dict(N=-1), 'N')):
        rc = est(**kw)
        assert rc < 0, why
        assert why in message(), (why, message())
    assert (out_bufs['rho'] == 7.0).all() and (out_bufs['status'] == 7).all()         # nothing was written
    assert est(N=0, y=None, fitted=None, group=None) == 0                      # a legal no-op: every group without pairs
    assert (out_bufs['status'] == _lib.CORR_NO_PAIRS).all() and not out_bufs['rho'].any() and np.isnan(out_bufs['rho_raw']).all()
    assert est(want=('rho', 'status')) == 0 and _same(out_bufs['rho'], est0.rho)
    with pytest.raises(ValueError, match='group'):
        fc.residual_correlation(y, fitted, hi, 6)
    with pytest.raises(ValueError, match='rho_max'):
        fc.residual_correlation(y, fitted, group, 6, rho_max=2.0)
    with pytest.raises(ValueError, match='fitted'):
        fc.residual_correlation(y, fitted[:, :-1], group, 6)
    # the context is usable: the same estimate as before the refusals
    est1 = fc.residual_correlation(y, fitted, group, 6)
    for k in EST_FIELDS:
        assert _same(getattr(est1, k), getattr(est0, k)), k


# ---- 7. plain C ----------------------------------------------------------------------------------------------------------

def test_abi_rollup_corr_plain_c(env, tmp_path):
    """tests/c/abi_rollup_corr.c drives tsf_residual_corr / create / set_noise_corr / add / quantiles / free from plain
    C99 and writes what they return"""
    fc, _lib = env
    N, G, Hc, T = 12, 3, 4, 70
    m, cal, extra, sn = _noise_members(N, np.arange(Hc))
    group = np.arange(N, dtype=np.int64) % G
    rng = np.random.default_rng(8)
    f = rng.normal(0, 1, (G, T))
    fitted = 50.0 + rng.normal(0, 5, (N, T))
    y = fitted + np.array([0.9, 0.5, 0.0])[group, None] * f[group] + rng.normal(0, 1, (N, T))
    p = str(tmp_path)
    for name, v in (('theta.f64', m.theta), ('ys.f64', m.y_scale), ('grid.bin', m.grid), ('extra.f64', extra),
                    ('fut.i64', cal), ('key.i64', m.keys), ('group.i64', group), ('y.f64', y), ('fitted.f64', fitted)):
        np.ascontiguousarray(v).tofile(os.path.join(p, name))
    exe = p + '/abi_rollup_corr'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_rollup_corr.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, str(N), str(Hc), str(G), str(T), p])
    got = np.fromfile(p + '/out.f64')
    est = fc.residual_correlation(y, fitted, group, G)
    assert est.rho[0] > est.rho[1] > 0.05
    lv = [0.1, 0.5, 0.9]
    with fc.Rollup(cal, G, uncertainty_samples=50, seed=5, noise_corr=est) as roll:
        roll.add(m.spec, m.theta, m.y_scale, m.grid, group, m.keys, floor=m.floor, extra_future=extra)
        r = roll.quantiles(lv)
        want = np.concatenate([est.rho, est.rho_raw, est.scale, r.yhat.ravel(), r.q.ravel(), roll.samples().ravel()])
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0
    assert np.array_equal(np.fromfile(p + '/ints.i64', dtype=np.int64),
                          np.concatenate([est.n_pairs, est.n_used, est.status, r.count]))


# ---- 8. end to end through forecaster ------------------------------------------------------------------------------------

def test_end_to_end(env):
    """64 series x 200 days in 8 groups with a planted common shock per group: fit_aligned -> fit_residual_correlation
    -> Rollup(noise_corr=...).  The direction only: every group reports rho > 0 and its total's P10-P90 is wider than the
    independent roll-up's on every row; no coverage number is asserted."""
    fc, _lib = env
    from time_series_spark_amd import synth
    N, T, G, Hf = 64, 200, 8, 14
    rng = np.random.default_rng(31)
    ds = synth.daily_grid(T)
    group = np.arange(N, dtype=np.int64) % G
    t = np.arange(T)
    shock = rng.normal(0, 1, (G, T))
    y = (100.0 + rng.uniform(0.0, 0.1, (N, 1)) * t + 5.0 * np.sin(2 * np.pi * t / 7.0 + rng.uniform(0, 6, (N, 1)))
         + 3.0 * shock[group] + 3.0 * rng.normal(0, 1, (N, T)))
    spec = fc.ModelSpec(growth='linear', n_changepoints=5,
                        seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3, 'mode': 'additive'}])
    res = fc.fit_aligned(spec, ds, y)
    # a series whose fit failed (a few line-search failures on this noisy panel: Prophet would raise) takes no part, in
    # the estimate (group -1) or in the roll-up, as a caller would treat it
    ok = res.status > 0
    members = np.bincount(group[ok], minlength=G)
    print('fitted', int(ok.sum()), 'of', N, 'members per group', members)
    assert (members >= 4).all()
    nc = fc.fit_residual_correlation(spec, res, ds, y, np.where(ok, group, -1), G)
    print('rho', np.round(nc.rho, 3))
    assert (nc.status == _lib.CORR_OK).all() and (nc.rho > 0).all() and np.array_equal(nc.n_used, members)
    fut = ds[-1] + synth.DAY_NS * np.arange(1, Hf + 1)
    keys = np.arange(N, dtype=np.int64) + 1000
    width = []
    for corr in (None, nc):
        uniq, r = fc.predict_rollup(spec, res.theta[ok], res.y_scale[ok], res.grid, fut, group[ok], [0.1, 0.9], keys[ok],
                                    uncertainty_samples=1000, seed=3, noise_corr=corr)
        assert np.array_equal(uniq, np.arange(G)) and np.array_equal(r.count, members)
        width.append(r.q[:, 1] - r.q[:, 0])
    assert width[0].shape == (G, Hf) and (width[1] > width[0]).all()
