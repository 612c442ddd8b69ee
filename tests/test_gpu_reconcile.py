"""GPU tests of reconciliation in group roll-ups (tsf_rollup_set_totals / _reconcile / _reconciled_totals:
reconcile_member_kernel and reconcile_total_kernel behind the draw loop of the roll-ups, rollup_cumsum_kernel and
quantile_kernel on what they write).

The reference in every test is numpy on fc.predictive_samples and fc.predict of the same members and totals, keys, seed
and sample count, through the restatement of the contract in tests/reconcile_ref.py (include/tsf.h "reconciliation"):
zeros, acc = acc + x over the members in call order, top = 0.0 + t, d = top - acc (+0.0 without a total),
x + share * d, acc + share_total * d.  Every comparison is bit for bit on the int64 view, except coherence, whose bound
is derived in reconcile_ref.coherence_bound.

The members are tests/forecast_cases.py's cases tiled the way tests/test_gpu_rollup.py tiles them: the case's models
repeated, theta's seasonal block, sigma and y_scale perturbed per series by a seeded generator, no fitting.  A sample
does not depend on the sample count (pinned by test_gpu_quantiles.test_prefix_property), so the reference draws are
taken once at 300 samples and cut."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import forecast_cases as fcs, helpers, reconcile_ref as rr

pytestmark = pytest.mark.gpu

SEED = 17
LEVELS = np.array([0, 0.1, 0.5, 0.975, 1])


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU reconciliation tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Members(object):
    """N series of one spec: spec, theta, y_scale, grid [N], floor, cap (or None), keys"""

    def take(self, sl):
        m = Members()
        m.spec, m.N = self.spec, len(self.theta[sl])
        m.theta, m.y_scale, m.grid, m.floor, m.keys = self.theta[sl], self.y_scale[sl], self.grid[sl], self.floor[sl], self.keys[sl]
        m.cap = None if self.cap is None else self.cap[sl]
        return m

    def args(self):
        return self.spec, self.theta, self.y_scale, self.grid

    def kw(self):
        return dict(floor=self.floor, cap=self.cap)


def _tiled(name, N, seed, key0):
    """case `name` repeated to N series, theta's seasonal block, sigma and y_scale perturbed per series -> (Members, case)"""
    c = fcs.make(name)
    rng = np.random.default_rng(seed)
    rep = -(-N // c.N)
    ncp = c.spec.n_changepoints
    m = Members()
    m.spec, m.N = c.spec, N
    m.theta = np.tile(c.theta, (rep, 1))[:N].copy()
    m.theta[:, 3 + ncp:] *= rng.uniform(0.5, 1.5, (N, 1))
    m.theta[:, 2] += rng.normal(0, 0.3, N)
    m.y_scale = np.tile(c.y_scale, rep)[:N] * rng.uniform(0.5, 2.0, N)
    m.grid = c.grid[np.arange(N) % len(c.grid)].copy()
    m.floor = np.tile(c.floor, rep)[:N].copy()
    m.cap = None if c.cap is None else np.tile(c.cap, rep)[:N].copy()
    m.keys = np.arange(N, dtype=np.int64) * 7919 + key0
    return m, c


def _draws(fc, m, cal, S):
    """(draws [N][H][S], yhat [N][H]) of the series on the calendar: fc.predictive_samples and fc.predict"""
    ps = fc.predictive_samples(*m.args(), cal, series_key=m.keys, uncertainty_samples=S, seed=SEED, **m.kw())
    return ps['yhat'], fc.predict(*m.args(), cal, **m.kw())


def _accumulate(G, adds):
    """adds: (group [n], draws [n][H][S], yhat [n][H]) per call, in call order -> (acc [G][H][S], ysum [G][H]) from zeros"""
    _, H, S = adds[0][1].shape
    acc, ysum = np.zeros((G, H, S)), np.zeros((G, H))
    for group, x, y in adds:
        for n in range(len(group)):
            g = int(group[n])
            acc[g] = acc[g] + x[n]
            ysum[g] = ysum[g] + y[n]
    return acc, ysum


def _add(roll, m, group):
    roll.add(*m.args(), group, m.keys, **m.kw())


def _totals(roll, t, group):
    roll.set_totals(*t.args(), group, t.keys, **t.kw())


def _reconcile(roll, m, group, share, **kw):
    return roll.reconcile(*m.args(), group, m.keys, share, **dict(m.kw(), **kw))


G = 6
SPLIT = 30
HAS_TOP = np.array([1, 1, 1, 0, 1, 0])
T_GROUP = np.array([2, 0, 4, 1], dtype=np.int64)


@pytest.fixture(scope='module')
def case(env):
    """65 series of iv65's model (logistic, floor, cap) on the first three future rows of its series 0, in 5 groups of 6
    indices: n % 4 for the first 64, series 64 alone in group 4, index 5 empty; four totals of the same model with their
    own key family for groups 2, 0, 4, 1 (in that order): group 3 has none.  The reference at 300 samples: the draws, the
    two accumulators, the shares from unequal weights and the reconciled draws."""
    fc, _lib = env
    m, c = _tiled('iv65', 65, seed=12, key0=10 ** 7)
    t, _ = _tiled('iv65', 4, seed=13, key0=9 * 10 ** 9)
    assert m.spec.growth == 'logistic' and m.cap is not None and not set(m.keys) & set(t.keys)
    cal = np.ascontiguousarray(c.fut[0, :3])
    group = np.arange(65, dtype=np.int64) % 4
    group[64] = 4
    x, y = _draws(fc, m, cal, 300)
    tx, ty = _draws(fc, t, cal, 300)
    rng = np.random.default_rng(77)
    v = np.where(HAS_TOP == 1, rng.uniform(0.5, 20.0, G), np.nan)
    share, share_total = fc.reconcile_shares(group, G, weight=rng.uniform(0.2, 5.0, 65), total_weight=v)
    assert share_total[3] == 0 and share_total[5] == 0 and (share[group == 3] == 0).all() and share[64] == share_total[4] > 0
    d = dict(m=m, t=t, cal=cal, group=group, x=x, y=y, tx=tx, ty=ty, share=share, share_total=share_total)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _reference(d, S, share=None, share_total=None):
    """the contract at S samples -> dict of the members' and the totals' yhat, samples, q, cum_q (numpy)"""
    share = d['share'] if share is None else share
    share_total = d['share_total'] if share_total is None else share_total
    x, tx, group = d['x'][:, :, :S], d['tx'][:, :, :S], d['group']
    acc, ysum = _accumulate(G, [(group[:SPLIT], x[:SPLIT], d['y'][:SPLIT]), (group[SPLIT:], x[SPLIT:], d['y'][SPLIT:])])
    top, ytop = _accumulate(G, [(T_GROUP, tx, d['ty'])])
    dd, dy = rr.incoherence(top, acc, HAS_TOP), rr.incoherence(ytop, ysum, HAS_TOP)
    r = dict(acc=acc, ysum=ysum, top=top, ytop=ytop)
    r['samples'], r['yhat'] = rr.members(x, group, share, dd), rr.members(d['y'], group, share, dy)
    r['t_samples'], r['t_yhat'] = rr.totals(acc, share_total, dd), rr.totals(ysum, share_total, dy)
    r['q'], r['cum_q'] = rr.q_and_cum_q(r['samples'], LEVELS)
    r['t_q'], r['t_cum_q'] = rr.q_and_cum_q(r['t_samples'], LEVELS)
    return r


def _filled(fc, d, S):
    """a roll-up with the case's members (two add calls) and totals"""
    roll = fc.Rollup(d['cal'], G, uncertainty_samples=S, seed=SEED)
    _add(roll, d['m'].take(slice(0, SPLIT)), d['group'][:SPLIT])
    _add(roll, d['m'].take(slice(SPLIT, 65)), d['group'][SPLIT:])
    _totals(roll, d['t'], T_GROUP)
    return roll


# ---- 1. the contract --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [300, 2])
def test_members_and_totals_are_the_contract(env, case, S):
    """S = 300: a tail block of 44 samples behind a full one; S = 2: the smallest"""
    fc, _lib = env
    d = case
    want = _reference(d, S)
    with _filled(fc, d, S) as roll:
        r = _reconcile(roll, d['m'], d['group'], d['share'], quantiles=LEVELS, cumulative=True, samples=True)
        tq, ts = roll.reconciled_totals(d['share_total'], LEVELS, cumulative=True, samples=True)
    assert r.samples.shape == (65, 3, S) and r.q.shape == (65, len(LEVELS), 3)
    assert _bits(r.samples, want['samples']) and _bits(r.yhat, want['yhat'])
    assert _bits(r.q, want['q']) and _bits(r.cum_q, want['cum_q']) and _bits(r.cum_q[:, :, 0], r.q[:, :, 0])
    assert _bits(ts, want['t_samples']) and _bits(tq.yhat, want['t_yhat'])
    assert _bits(tq.q, want['t_q']) and _bits(tq.cum_q, want['t_cum_q'])
    assert list(tq.count) == [16, 16, 16, 16, 1, 0]
    # the group without a total: its members and its sum untouched; the empty index: +0.0
    no = d['group'] == 3
    assert _bits(r.samples[no], d['x'][no][:, :, :S]) and _bits(r.yhat[no], d['y'][no]) and _bits(ts[3], want['acc'][3])
    assert _bits(ts[5], np.zeros((3, S))) and _bits(tq.q[5], np.zeros((len(LEVELS), 3)))
    # everything else moved
    assert (r.samples[~no] != d['x'][~no][:, :, :S]).mean() > 0.99
    f = r.frame(1, d['cal'])
    assert list(f.columns) == ['ds', 'yhat'] + fc.quantile_columns(LEVELS) + fc.quantile_columns(LEVELS, 'yhat_cum_q')
    assert np.array_equal(f['yhat_cum_q97.5'].values, r.cum_q[1, 3])


# ---- 2. the neutral element ---------------------------------------------------------------------------------------------

def test_zero_shares_and_untouched_accumulators(env, case):
    fc, _lib = env
    d = case
    m, S = d['m'], 300
    with fc.Rollup(d['cal'], G, uncertainty_samples=S, seed=SEED) as roll:
        _add(roll, m.take(slice(0, SPLIT)), d['group'][:SPLIT])
        _add(roll, m.take(slice(SPLIT, 65)), d['group'][SPLIT:])
        before = (roll.quantiles(LEVELS, cumulative=True), roll.samples())
        _totals(roll, d['t'], T_GROUP)
        r0 = _reconcile(roll, m, d['group'], np.zeros(65), quantiles=LEVELS, cumulative=True, samples=True)
        t0, ts0 = roll.reconciled_totals(np.zeros(G), LEVELS, cumulative=True, samples=True)
        _reconcile(roll, m, d['group'], d['share'], quantiles=LEVELS, cumulative=True, samples=True)
        roll.reconciled_totals(d['share_total'], LEVELS, cumulative=True)
        after = (roll.quantiles(LEVELS, cumulative=True), roll.samples())
    p = fc.predict_quantiles(*m.args(), d['cal'], LEVELS, series_key=m.keys, uncertainty_samples=S, seed=SEED,
                             cumulative=True, **m.kw())
    assert _bits(r0.yhat, p.yhat) and _bits(r0.q, p.q) and _bits(r0.cum_q, p.cum_q) and _bits(r0.samples, d['x'])
    for a in (t0, after[0]):
        assert _bits(a.yhat, before[0].yhat) and _bits(a.q, before[0].q) and _bits(a.cum_q, before[0].cum_q)
        assert np.array_equal(a.count, before[0].count)
    assert _bits(ts0, before[1]) and _bits(after[1], before[1])


# ---- 3. coherence on the device -----------------------------------------------------------------------------------------

def test_members_sum_to_the_total(env, case):
    """sum over a group's members of the reconciled samples (and yhat) = the reconciled total's, within
    reconcile_ref.coherence_bound: the bound derived there from the operation count"""
    fc, _lib = env
    d = case
    with _filled(fc, d, 300) as roll:
        r = _reconcile(roll, d['m'], d['group'], d['share'], samples=True)
        tq, ts = roll.reconciled_totals(d['share_total'], [0.5], samples=True)
    top, ytop = _accumulate(G, [(T_GROUP, d['tx'], d['ty'])])
    for g in np.flatnonzero(HAS_TOP):
        idx = np.flatnonzero(d['group'] == g)
        tot, ytot = np.zeros((3, 300)), np.zeros(3)
        for n in idx:
            tot, ytot = tot + r.samples[n], ytot + r.yhat[n]
        bound = rr.coherence_bound(len(idx), np.abs(d['x'][idx]).sum(axis=0), np.abs(top[g]))
        ybound = rr.coherence_bound(len(idx), np.abs(d['y'][idx]).sum(axis=0), np.abs(ytop[g]))
        err, yerr = np.abs(tot - ts[g]), np.abs(ytot - tq.yhat[g])
        print('group %d (%d members): max error / bound: samples %.3f, yhat %.3f' % (g, len(idx), (err / bound).max(),
                                                                                    (yerr / ybound).max()))
        assert (err <= bound).all() and (yerr <= ybound).all()
        # (the pair it started from is incoherent by far more)
        assert np.abs(d['x'][idx].sum(axis=0) - top[g]).mean() > 1e9 * bound.max()


# ---- 4. chunk independence ----------------------------------------------------------------------------------------------

def test_chunk_independence(env):
    """20 members x 960 rows x 4096 samples with cum_q: 8 * 960 * (3 + 2 * 4096) bytes of scratch per series, 8 series per
    chunk, so one call runs 3 chunks (8 + 8 + 4); the same members reconciled in calls of 7, 6 and 7 (one chunk each)"""
    fc, _lib = env
    m, c = _tiled('h960', 20, seed=9, key0=5)
    t, _ = _tiled('h960', 3, seed=10, key0=10 ** 12)
    assert c.H == 960 and (512 << 20) // (8 * 960 * (3 + 2 * 4096)) == 8
    group = np.arange(20, dtype=np.int64) % 3
    share, share_total = fc.reconcile_shares(group, 3, total_weight='ols')
    lv = [0.1, 0.5, 0.9]
    with fc.Rollup(c.fut, 3, uncertainty_samples=4096, seed=SEED) as roll:
        _add(roll, m, group)
        _totals(roll, t, np.arange(3, dtype=np.int64))
        one = _reconcile(roll, m, group, share, quantiles=lv, cumulative=True)
        parts = [_reconcile(roll, m.take(sl), group[sl], share[sl], quantiles=lv, cumulative=True)
                 for sl in (slice(0, 7), slice(7, 13), slice(13, 20))]
    for k in ('yhat', 'q', 'cum_q'):
        assert _bits(getattr(one, k), np.concatenate([getattr(p, k) for p in parts])), k
    assert _bits(one.cum_q[:, :, 0], one.q[:, :, 0]) and (one.q[:, 1] != one.q[:, 0]).all()


# ---- 5. output independence -----------------------------------------------------------------------------------------------

def test_output_independence(env, case):
    """q alone (one sample buffer), q with cum_q (two: another scratch layout), q with samples, samples alone"""
    fc, _lib = env
    d = case
    with _filled(fc, d, 300) as roll:
        full = _reconcile(roll, d['m'], d['group'], d['share'], quantiles=LEVELS, cumulative=True, samples=True)
        q = _reconcile(roll, d['m'], d['group'], d['share'], quantiles=LEVELS)
        qc = _reconcile(roll, d['m'], d['group'], d['share'], quantiles=LEVELS, cumulative=True)
        qs = _reconcile(roll, d['m'], d['group'], d['share'], quantiles=LEVELS, samples=True)
        s = _reconcile(roll, d['m'], d['group'], d['share'], samples=True)
        tq = roll.reconciled_totals(d['share_total'], LEVELS)
        tqc = roll.reconciled_totals(d['share_total'], LEVELS, cumulative=True)
    assert q.cum_q is None and q.samples is None and qc.samples is None and qs.cum_q is None and s.q is None
    for r in (q, qc, qs):
        assert _bits(r.q, full.q) and _bits(r.yhat, full.yhat)
    assert _bits(qc.cum_q, full.cum_q) and _bits(qs.samples, full.samples) and _bits(s.samples, full.samples)
    assert _bits(s.yhat, full.yhat)
    assert _bits(tq.q, tqc.q) and _bits(tq.yhat, tqc.yhat) and tq.cum_q is None


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals(env, case):
    """each < 0 with a message before any launch; the handle stays usable, and a later valid call is bit-identical to
    the same call on a fresh handle"""
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    d = case
    m, t, S = d['m'], d['t'], 10
    cs = m.spec.to_c()

    def message():
        return L.tsf_last_error(ctx.handle).decode()

    arr = dict(theta=m.theta, ys=m.y_scale, grid=m.grid, floor=m.floor, cap=m.cap, keys=m.keys, group=d['group'],
               share=d['share'])
    arr = {k: np.ascontiguousarray(a) for k, a in arr.items()}
    tarr = dict(theta=t.theta, ys=t.y_scale, grid=t.grid, floor=t.floor, cap=t.cap, keys=t.keys, group=T_GROUP)
    tarr = {k: np.ascontiguousarray(a) for k, a in tarr.items()}
    bufs = dict(yhat=np.zeros((65, 3)), q=np.zeros((65, 65, 3)), cum_q=np.zeros((65, 65, 3)), samples=np.zeros((65, 3, S)))
    p = lambda a: None if a is None else a.ctypes.data             # noqa: E731

    def reconcile(roll, levels=(0.1, 0.9), want=('yhat', 'q'), N=65, n_q=None, **kw):
        a = dict(arr, **kw)
        levels = np.ascontiguousarray(levels, dtype=np.float64)
        out = _lib.TsfReconcileOut(**{k: bufs[k].ctypes.data for k in want})
        return L.tsf_rollup_reconcile(roll._h, ctypes.byref(cs), N, p(a['theta']), p(a['ys']), p(a['grid']), 65,
                                      p(a['floor']), p(a['cap']), None, 1, p(a['keys']), p(a['group']), p(a['share']),
                                      len(levels) if n_q is None else n_q, levels.ctypes.data, ctypes.byref(out))

    def set_totals(roll, sl=slice(None), **kw):
        a = dict({k: np.ascontiguousarray(v[sl]) for k, v in tarr.items()}, **kw)   # (an override is given already cut)
        return L.tsf_rollup_set_totals(roll._h, ctypes.byref(cs), len(a['theta']), p(a['theta']), p(a['ys']), p(a['grid']),
                                       len(a['grid']), p(a['floor']), p(a['cap']), None, 1, p(a['keys']), p(a['group']))

    def bad(a, i, x):
        a = a.copy()
        a[i] = x
        return a

    roll = fc.Rollup(d['cal'], G, uncertainty_samples=S, seed=SEED)
    _add(roll, m.take(slice(0, SPLIT)), d['group'][:SPLIT])
    _add(roll, m.take(slice(SPLIT, 65)), d['group'][SPLIT:])
    # before any set_totals: a refusal, not silent zeros
    assert reconcile(roll) < 0 and 'before any tsf_rollup_set_totals' in message()
    with pytest.raises(_lib.TsfError, match='before any tsf_rollup_set_totals'):
        roll.reconciled_totals(d['share_total'], [0.5])
    # a group twice in one call; then the totals of groups 2 and 0, and a second total for group 0
    assert set_totals(roll, group=np.array([2, 0, 2, 1])) < 0 and 'group[2]' in message() and 'already' in message()
    assert set_totals(roll, sl=slice(0, 2)) == 0
    assert set_totals(roll, sl=slice(1, 3)) < 0 and 'group[0] = 0' in message()
    assert set_totals(roll, sl=slice(2, 4), keys=None) < 0 and 'series_key' in message()
    assert set_totals(roll, sl=slice(2, 4), group=np.array([4, G])) < 0 and 'group[1]' in message()
    assert set_totals(roll, sl=slice(2, 4)) == 0
    before = (roll.samples(), roll.reconciled_totals(d['share_total'], LEVELS, cumulative=True, samples=True))
    for kw, why in ((dict(share=bad(arr['share'], 9, 1.0000001)), 'share[9]'), (dict(share=bad(arr['share'], 0, -1e-9)), 'share[0]'),
                    (dict(share=bad(arr['share'], 64, np.nan)), 'share[64]'), (dict(share=None), 'share'),
                    (dict(keys=None), 'series_key'), (dict(group=bad(arr['group'], 3, G)), 'group[3]'),
                    (dict(cap=None), 'cap'), (dict(levels=[0.5, 1.5]), 'quantiles[1]'),
                    (dict(levels=[float('nan')]), 'quantiles[0]'), (dict(levels=np.linspace(0, 1, 65)), 'n_q'),
                    (dict(want=('yhat',)), 'nothing requested'), (dict(levels=[], want=('yhat', 'q')), 'n_q = 0'),
                    (dict(want=('q',)), 'yhat'), (dict(N=-1), 'N')):
        rc = reconcile(roll, **kw)
        assert rc < 0, why
        assert why in message(), (why, message())
    assert reconcile(roll, N=0) == 0                                # a legal no-op
    mu = np.ascontiguousarray(d['share_total'])
    tout = _lib.TsfRollupOut(yhat=bufs['yhat'].ctypes.data, q=bufs['q'].ctypes.data)
    lv = np.array([0.5])
    for share_total, why in ((bad(mu, 1, 2.0), 'share_total[1]'), (bad(mu, 5, np.nan), 'share_total[5]')):
        assert L.tsf_rollup_reconciled_totals(roll._h, share_total.ctypes.data, 1, lv.ctypes.data, ctypes.byref(tout)) < 0
        assert why in message()
    none = _lib.TsfRollupOut(yhat=bufs['yhat'].ctypes.data)
    assert L.tsf_rollup_reconciled_totals(roll._h, mu.ctypes.data, 1, lv.ctypes.data, ctypes.byref(none)) < 0
    assert 'nothing requested' in message()
    # the Python layer: ValueError before the library is touched
    for kw in (dict(share=bad(arr['share'], 2, 1.5)), dict(share=arr['share'][:-1]), dict(quantiles=[0.5, -0.1]), dict(),
               dict(cumulative=True, samples=True), dict(quantiles=[0.5], keys=None)):
        kw = dict(kw)
        keys, share = kw.pop('keys', m.keys), kw.pop('share', d['share'])
        with pytest.raises(ValueError):
            roll.reconcile(*m.args(), d['group'], keys, share, **dict(m.kw(), **kw))
    with pytest.raises(ValueError):
        roll.reconciled_totals(bad(mu, 0, -0.5), [0.5])
    with pytest.raises(ValueError):
        roll.reconciled_totals(mu, [])
    with pytest.raises(ValueError, match='twice'):
        roll.set_totals(*t.args(), np.array([3, 3, 5, 5]), t.keys, **t.kw())
    # usable afterwards, and what a fresh handle gives
    got = _reconcile(roll, m, d['group'], d['share'], quantiles=LEVELS, cumulative=True, samples=True)
    after = (roll.samples(), roll.reconciled_totals(d['share_total'], LEVELS, cumulative=True, samples=True))
    roll.close()
    with pytest.raises(ValueError, match='closed'):
        _reconcile(roll, m, d['group'], d['share'], samples=True)
    with _filled(fc, d, S) as fresh:
        want = _reconcile(fresh, m, d['group'], d['share'], quantiles=LEVELS, cumulative=True, samples=True)
        wt = fresh.reconciled_totals(d['share_total'], LEVELS, cumulative=True, samples=True)
    for k in ('yhat', 'q', 'cum_q', 'samples'):
        assert _bits(getattr(got, k), getattr(want, k)), k
    for r in (before[1], after[1]):
        assert _bits(r[1], wt[1]) and _bits(r[0].q, wt[0].q) and _bits(r[0].cum_q, wt[0].cum_q) and _bits(r[0].yhat, wt[0].yhat)
    assert _bits(before[0], after[0])


# ---- 7. end to end with real fits -----------------------------------------------------------------------------------------

def test_end_to_end(env):
    fc, _lib = env
    from time_series_spark_amd import synth
    H, S, lv = 7, 256, [0.1, 0.5, 0.9]
    ds, y = synth.make_panel(12, 128, 'linear', seed=6)
    labels = 40 + 10 * (np.arange(12) // 3)
    uniq, group = fc.rollup_groups(labels)
    assert list(uniq) == [40, 50, 60, 70]
    tot = fc.aggregate_aligned(y, group, 4)
    assert _bits(tot[1], (y[3] + y[4]) + y[5])
    spec = fc.ModelSpec(growth='linear', n_changepoints=5,
                        seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3, 'mode': 'additive'}])
    fm, ft = fc.fit_aligned(spec, ds, y), fc.fit_aligned(spec, ds, tot)
    fut = ds[-1] + synth.DAY_NS * np.arange(1, H + 1)
    keys, tkeys = np.arange(12, dtype=np.int64), (np.int64(1) << 40) + np.arange(4, dtype=np.int64)
    u, rm, rt = fc.predict_reconciled(spec, fm.theta, fm.y_scale, fm.grid, fut, labels, lv, keys, ft.theta, ft.y_scale,
                                      ft.grid, tkeys, uncertainty_samples=S, seed=3, cumulative=True)
    assert list(u) == list(uniq) and rm.q.shape == (12, 3, H) and rt.q.shape == (4, 3, H) and list(rt.count) == [3] * 4
    share, share_total = fc.reconcile_shares(group, 4, total_weight='struct')
    assert _bits(share, np.full(12, 1.0 / 6.0)) and _bits(share_total, np.full(4, 0.5))
    with fc.Rollup(fut, 4, uncertainty_samples=S, seed=3) as roll:
        roll.add(spec, fm.theta, fm.y_scale, fm.grid, group, keys)
        roll.set_totals(spec, ft.theta, ft.y_scale, ft.grid, np.arange(4), tkeys)
        em = roll.reconcile(spec, fm.theta, fm.y_scale, fm.grid, group, keys, share, quantiles=lv, cumulative=True)
        et = roll.reconciled_totals(share_total, lv, cumulative=True)
    for a, b in ((rm, em), (rt, et)):
        assert _bits(a.yhat, b.yhat) and _bits(a.q, b.q) and _bits(a.cum_q, b.cum_q)
    # the members' yhat sums to the totals' within the derived bound; it did not before
    ym, yt = fc.predict(spec, fm.theta, fm.y_scale, fm.grid, fut), fc.predict(spec, ft.theta, ft.y_scale, ft.grid, fut)
    for g in range(4):
        idx = np.flatnonzero(group == g)
        bound = rr.coherence_bound(3, np.abs(ym[idx]).sum(axis=0), np.abs(yt[g]))
        assert (np.abs((rm.yhat[idx[0]] + rm.yhat[idx[1]]) + rm.yhat[idx[2]] - rt.yhat[g]) <= bound).all()
        assert (np.abs(ym[idx].sum(axis=0) - yt[g]) > 1e6 * bound).any()
        # halfway between the two base forecasts of the total ('struct': mu = 1/2), and monotone quantiles
        assert np.allclose(rt.yhat[g], 0.5 * (ym[idx].sum(axis=0) + yt[g]), rtol=1e-12)
    assert (np.diff(rm.q, axis=1) >= 0).all() and (np.diff(rt.cum_q, axis=1) >= 0).all()
    with pytest.raises(ValueError, match='shares a key'):
        fc.predict_reconciled(spec, fm.theta, fm.y_scale, fm.grid, fut, labels, lv, keys, ft.theta, ft.y_scale, ft.grid,
                              keys[:4])
    with pytest.raises(ValueError, match='one total per unique label'):
        fc.predict_reconciled(spec, fm.theta, fm.y_scale, fm.grid, fut, labels, lv, keys, ft.theta[:3], ft.y_scale[:3],
                              ft.grid, tkeys[:3])


# ---- 8. plain C -------------------------------------------------------------------------------------------------------------

def test_abi_reconcile_plain_c(env, case, tmp_path):
    """tests/c/abi_reconcile.c drives shares / create / add twice / set_totals / reconcile / reconciled_totals / free from
    plain C99 on the contract case and writes what they return"""
    fc, _lib = env
    d = case
    m, t = d['m'], d['t']
    p = str(tmp_path)
    v = np.where(HAS_TOP == 1, 2.5, np.nan)
    files = [('spec.bin', np.frombuffer(bytes(m.spec.to_c()), dtype=np.uint8)), ('fut.i64', d['cal']), ('v.f64', v)]
    for prefix, s, group in (('', m, d['group']), ('t_', t, T_GROUP)):
        files += [(prefix + 'theta.f64', s.theta), (prefix + 'ys.f64', s.y_scale), (prefix + 'grid.bin', s.grid),
                  (prefix + 'floor.f64', s.floor), (prefix + 'cap.f64', s.cap), (prefix + 'key.i64', s.keys),
                  (prefix + 'group.i64', group)]
    for name, a in files:
        np.ascontiguousarray(a).tofile(os.path.join(p, name))
    exe = p + '/abi_reconcile'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_reconcile.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, '65', '4', '3', str(G), p])
    got = np.fromfile(p + '/out.f64')
    share, share_total = fc.reconcile_shares(d['group'], G, total_weight=v)
    lv = [0.1, 0.5, 0.9]
    with fc.Rollup(d['cal'], G, uncertainty_samples=50, seed=5) as roll:
        _add(roll, m.take(slice(0, 32)), d['group'][:32])
        _add(roll, m.take(slice(32, 65)), d['group'][32:])
        _totals(roll, t, T_GROUP)
        r = _reconcile(roll, m, d['group'], share, quantiles=lv, cumulative=True, samples=True)
        tq, ts = roll.reconciled_totals(share_total, lv, cumulative=True, samples=True)
    want = np.concatenate([a.ravel() for a in (share, share_total, r.yhat, r.q, r.cum_q, r.samples, tq.yhat, tq.q,
                                               tq.cum_q, ts)])
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0
    assert (share[d['group'] != 3] > 0).all()
