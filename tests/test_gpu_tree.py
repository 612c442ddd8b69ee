"""GPU tests of tree reconciliation (tsf_rollup_set_tree / _set_node_totals / _solve_tree / _reconcile_tree /
_tree_totals: tree_blend_kernel, tree_gather_kernel and tree_push_kernel over the roll-up's accumulators,
tree_member_kernel behind the draw loop of the roll-ups, tree_total_kernel, rollup_cumsum_kernel and quantile_kernel on
what they write).

The reference in every test is numpy on fc.predictive_samples and fc.predict of the same members and totals, keys, seed
and sample count, through the restatement of the contract in tests/tree_ref.py (include/tsf.h "tree reconciliation").
Every comparison is bit for bit on the int64 view, except coherence and the comparison with the two-level
reconciliation, whose bounds are tree_ref.solve_errors' running error analysis.

The case is the tree of tests/test_tree_ref.py on real fits: 9 short series of one linear model in 5 groups (group 3
empty, group 1 without a total), 3 parents (parent 2 with a single child, parent 0 without a total), one root, and the
fitted totals of the aggregated histories; three future rows.  A sample does not depend on the sample count (pinned by
test_gpu_quantiles.test_prefix_property), so the reference draws are taken once at 257 samples and cut."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import helpers, reconcile_ref as rr, tree_ref as tr
from tests.tree_ref import GROUP, N_NODES, PARENT, V

pytestmark = pytest.mark.gpu

SEED = 17
LEVELS = np.array([0, 0.1, 0.5, 0.975, 1])
H = 3
SPLIT = 5
# the fitted totals per level: (nodes, in the order given); the empty group 3 is given one, which is ignored
T_NODE = [np.array([2, 0, 4, 3], dtype=np.int64), np.array([2, 1], dtype=np.int64), np.array([0], dtype=np.int64)]
HAS = [np.array([1, 0, 1, 1, 1]), np.array([0, 1, 1]), np.array([1])]


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU tree reconciliation tests cannot run (product has no CPU fallback)')
    return fc, _lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Fitted(object):
    """n series of one spec out of one fit: spec, theta, y_scale, grid [n], keys"""

    def __init__(self, spec, fit, idx, keys):
        self.spec, self.theta, self.y_scale = spec, fit.theta[idx].copy(), fit.y_scale[idx].copy()
        self.grid = np.array([fit.grid_of(n) for n in idx], dtype=fit.grid.dtype)
        self.keys, self.N = np.ascontiguousarray(keys, dtype=np.int64), len(idx)

    def take(self, sl):
        m = Fitted.__new__(Fitted)
        m.spec, m.theta, m.y_scale, m.grid, m.keys = self.spec, self.theta[sl], self.y_scale[sl], self.grid[sl], self.keys[sl]
        m.N = len(m.theta)
        return m

    def args(self):
        return self.spec, self.theta, self.y_scale, self.grid


def _draws(fc, m, cal, S):
    """(draws [n][H][S], yhat [n][H]) of the series on the calendar: fc.predictive_samples and fc.predict"""
    ps = fc.predictive_samples(*m.args(), cal, series_key=m.keys, uncertainty_samples=S, seed=SEED)
    return ps['yhat'], fc.predict(*m.args(), cal)


def _into(n, node, x):
    """+0.0 + x[j] in cell node[j] of n cells"""
    out = np.zeros((n,) + x.shape[1:])
    for j, i in enumerate(node):
        out[i] = out[i] + x[j]
    return out


@pytest.fixture(scope='module')
def case(env):
    """One fit_aligned call of 16 histories of 128 days: the 9 members, then the totals of groups 2, 0, 4 (the sums of
    their members' histories) and of the empty group 3 (a history of its own: the total is ignored), of parents 2 and 1,
    and of the root.  The reference at 257 samples: every series' draws and point forecast, the weights and the shares."""
    fc, _lib = env
    from time_series_spark_amd import synth
    ds, y = synth.make_panel(9, 128, 'linear', seed=6)
    g1 = fc.aggregate_aligned(y, GROUP, 5)
    g2 = fc.aggregate_aligned(g1, PARENT[0], 3)
    g3 = fc.aggregate_aligned(g2, PARENT[1], 1)
    g1[3] = 0.5 * y[0] + 3.0
    hist = np.concatenate([y, g1[T_NODE[0]], g2[T_NODE[1]], g3[T_NODE[2]]])
    spec = fc.ModelSpec(growth='linear', n_changepoints=5,
                        seasonalities=[{'name': 'weekly', 'period': 7, 'fourier_order': 3, 'mode': 'additive'}])
    fit = fc.fit_aligned(spec, ds, hist)
    cal = np.ascontiguousarray(ds[-1] + synth.DAY_NS * np.arange(1, H + 1))
    m = Fitted(spec, fit, np.arange(9), np.arange(9) * 7919 + 10 ** 7)
    t, at = [], 9
    for k, node in enumerate(T_NODE):
        t.append(Fitted(spec, fit, np.arange(at, at + len(node)), (np.int64(k + 1) << 40) + np.arange(len(node))))
        at += len(node)
    x, y_hat = _draws(fc, m, cal, 257)
    tx = [_draws(fc, tk, cal, 257) for tk in t]
    tree = fc.RollupTree(GROUP, N_NODES, PARENT)
    w = np.random.default_rng(77).uniform(0.2, 5.0, 9)
    shares = fc.reconcile_tree_shares(tree, weight=w, node_weight=V)
    assert shares.mu[0][3] == 0 and shares.mu[0][1] == 0 and shares.mu[1][0] == 0 and shares.kappa[0][4] == 1
    d = dict(m=m, t=t, cal=cal, x=x, y=y_hat, tx=[a for a, _ in tx], ty=[b for _, b in tx], tree=tree, w=w, shares=shares)
    for a in [x, y_hat, w] + d['tx'] + d['ty']:
        a.setflags(write=False)
    return d


def _reference(d, S, shares=None, has=HAS):
    """the contract at S samples -> dict: the members' and per level the nodes' yhat, samples, q, cum_q (numpy)"""
    sh = d['shares'] if shares is None else shares
    x = d['x'][:, :, :S]
    acc, ysum = _into(5, GROUP[:SPLIT], x[:SPLIT]), _into(5, GROUP[:SPLIT], d['y'][:SPLIT])
    for n in range(SPLIT, 9):                                       # the second add call goes on where the first stopped
        acc[GROUP[n]] = acc[GROUP[n]] + x[n]
        ysum[GROUP[n]] = ysum[GROUP[n]] + d['y'][n]
    tot = [_into(N_NODES[k], T_NODE[k], d['tx'][k][:, :, :S]) for k in range(3)]
    ytot = [_into(N_NODES[k], T_NODE[k], d['ty'][k]) for k in range(3)]
    delta, c, _ = tr.solve(acc, tot, has, N_NODES, PARENT, sh.mu, sh.kappa)
    ydelta, yc, _ = tr.solve(ysum, ytot, has, N_NODES, PARENT, sh.mu, sh.kappa)
    r = dict(acc=acc, ysum=ysum, tot=tot, x=x)
    r['samples'], r['yhat'] = tr.members(x, GROUP, sh.share, delta), tr.members(d['y'], GROUP, sh.share, ydelta)
    r['q'], r['cum_q'] = rr.q_and_cum_q(r['samples'], LEVELS)
    r['t_samples'] = [tr.group_totals(acc, delta)] + c[1:]
    r['t_yhat'] = [tr.group_totals(ysum, ydelta)] + yc[1:]
    r['t_q'] = [rr.q_and_cum_q(s, LEVELS) for s in r['t_samples']]
    return r


def _add(roll, m, group):
    roll.add(*m.args(), group, m.keys)


def _filled(fc, d, S, totals=True, tree=True, seed=SEED):
    """a roll-up with the case's members (two add calls), its totals at every level and its tree"""
    roll = fc.Rollup(d['cal'], 5, uncertainty_samples=S, seed=seed)
    _add(roll, d['m'].take(slice(0, SPLIT)), GROUP[:SPLIT])
    _add(roll, d['m'].take(slice(SPLIT, 9)), GROUP[SPLIT:])
    if tree:
        roll.set_tree(d['tree'])
    if totals:
        roll.set_totals(*d['t'][0].args(), T_NODE[0], d['t'][0].keys)
        for level in (2, 3):
            roll.set_node_totals(level, *d['t'][level - 1].args(), T_NODE[level - 1], d['t'][level - 1].keys)
    return roll


def _reconcile(roll, d, share=None, **kw):
    return roll.reconcile_tree(*d['m'].args(), GROUP, d['m'].keys, d['shares'].share if share is None else share, **kw)


# ---- 1. the contract --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [257, 2])
def test_members_and_every_level_are_the_contract(env, case, S):
    """S = 257: one sample in a tail block behind a full one; S = 2: the smallest"""
    fc, _lib = env
    d = case
    want = _reference(d, S)
    with _filled(fc, d, S) as roll:
        roll.solve_tree(d['shares'])
        r = _reconcile(roll, d, quantiles=LEVELS, cumulative=True, samples=True)
        tq = [roll.tree_totals(level, LEVELS, cumulative=True, samples=True) for level in (1, 2, 3)]
    assert r.samples.shape == (9, H, S) and r.q.shape == (9, len(LEVELS), H)
    assert _bits(r.samples, want['samples']) and _bits(r.yhat, want['yhat'])
    assert _bits(r.q, want['q']) and _bits(r.cum_q, want['cum_q']) and _bits(r.cum_q[:, :, 0], r.q[:, :, 0])
    for k, (q, s) in enumerate(tq):
        assert s.shape == (N_NODES[k], H, S), k
        assert _bits(s, want['t_samples'][k]) and _bits(q.yhat, want['t_yhat'][k]), k
        assert _bits(q.q, want['t_q'][k][0]) and _bits(q.cum_q, want['t_q'][k][1]), k
    assert [list(q.count) for q, _ in tq] == [[1, 2, 4, 0, 2], [3, 4, 2], [9]]
    # the empty group, whose total is ignored: +0.0; everything else moved, the group without a total through its parent
    assert _bits(tq[0][1][3], np.zeros((H, S))) and _bits(tq[0][0].q[3], np.zeros((len(LEVELS), H)))
    assert (r.samples != d['x'][:, :, :S]).mean() > 0.99 and (tq[0][1][1] != want['acc'][1]).mean() > 0.99
    # a range of nodes is the same nodes
    with _filled(fc, d, S) as roll:
        roll.solve_tree(d['shares'])
        for level, (n0, n) in ((1, (1, 3)), (2, (2, 1))):
            q, s = roll.tree_totals(level, LEVELS, cumulative=True, samples=True, nodes=(n0, n))
            full = tq[level - 1]
            assert _bits(s, full[1][n0:n0 + n]) and _bits(q.q, full[0].q[n0:n0 + n]) and _bits(q.cum_q, full[0].cum_q[n0:n0 + n])
            assert _bits(q.yhat, full[0].yhat[n0:n0 + n]) and list(q.count) == list(full[0].count[n0:n0 + n])
    f = r.frame(1, d['cal'])
    assert list(f.columns) == ['ds', 'yhat'] + fc.quantile_columns(LEVELS) + fc.quantile_columns(LEVELS, 'yhat_cum_q')


# ---- 2. the neutral element ---------------------------------------------------------------------------------------------

def test_no_total_is_neutral_and_accumulators_untouched(env, case):
    fc, _lib = env
    d = case
    m, S = d['m'], 257
    none = fc.reconcile_tree_shares(d['tree'], weight=d['w'], node_weight=[np.full(n, np.nan) for n in N_NODES])
    with _filled(fc, d, S, totals=False) as roll:
        before = (roll.quantiles(LEVELS, cumulative=True), roll.samples())
        roll.solve_tree(none)
        r0 = _reconcile(roll, d, share=none.share, quantiles=LEVELS, cumulative=True, samples=True)
        t0, ts0 = roll.tree_totals(1, LEVELS, cumulative=True, samples=True)
        after = (roll.quantiles(LEVELS, cumulative=True), roll.samples())
    p = fc.predict_quantiles(*m.args(), d['cal'], LEVELS, series_key=m.keys, uncertainty_samples=S, seed=SEED, cumulative=True)
    assert _bits(r0.yhat, p.yhat) and _bits(r0.q, p.q) and _bits(r0.cum_q, p.cum_q) and _bits(r0.samples, d['x'])
    for a in (t0, after[0]):
        assert _bits(a.yhat, before[0].yhat) and _bits(a.q, before[0].q) and _bits(a.cum_q, before[0].cum_q)
        assert np.array_equal(a.count, before[0].count)
    assert _bits(ts0, before[1]) and _bits(after[1], before[1])
    # with totals: acc and top as they were after the solve and both reads (top through the two-level read at share 1)
    ones = np.ones(5)
    with _filled(fc, d, S) as roll:
        before = (roll.samples(), roll.reconciled_totals(ones, LEVELS, cumulative=True, samples=True))
        roll.solve_tree(d['shares'])
        _reconcile(roll, d, quantiles=LEVELS, cumulative=True)
        roll.tree_totals(1, LEVELS, cumulative=True)
        after = (roll.samples(), roll.reconciled_totals(ones, LEVELS, cumulative=True, samples=True))
    assert _bits(before[0], after[0]) and _bits(before[1][1], after[1][1]) and _bits(before[1][0].yhat, after[1][0].yhat)
    assert _bits(before[1][0].q, after[1][0].q) and _bits(before[1][0].cum_q, after[1][0].cum_q)


# ---- 3. one upper level without totals is the two-level reconciliation --------------------------------------------------

def test_one_upper_level_without_totals_is_reconcile(env, case):
    """in exact arithmetic; on the device within the sum of the two running error analyses (tree_ref.solve_errors,
    tree_ref.two_level_error): each side is that close to the projection.  Measured on the MI355X: the members differ by
    at most 0.28 of the bound (2.9e-11 on values near 8e4), the group totals by a rounding or two."""
    fc, _lib = env
    d = case
    S = 257
    flat = fc.RollupTree(GROUP, [5, 1], [np.zeros(5, dtype=np.int64)])
    v1 = np.where(HAS[0] == 1, V[0], np.nan)
    has1 = (~np.isnan(v1)).astype(np.int32)
    t_sel = np.flatnonzero(has1[T_NODE[0]])
    sh = fc.reconcile_tree_shares(flat, weight=d['w'], node_weight=[v1, [np.nan]])
    lam, mu = fc.reconcile_shares(GROUP, 5, weight=d['w'], total_weight=v1)
    t1 = d['t'][0].take(t_sel)
    with _filled(fc, d, S, totals=False, tree=False) as roll:
        roll.set_totals(*t1.args(), T_NODE[0][t_sel], t1.keys)
        two = roll.reconcile(*d['m'].args(), GROUP, d['m'].keys, lam, samples=True)
        two_t, two_ts = roll.reconciled_totals(mu, [0.5], samples=True)
        roll.set_tree(flat)
        roll.solve_tree(sh)
        got = _reconcile(roll, d, share=sh.share, samples=True)
        got_t, got_ts = roll.tree_totals(1, [0.5], samples=True)
    x = d['x']
    top = _into(5, T_NODE[0][t_sel], d['tx'][0][t_sel])
    e_tree, e_lvl = tr.solve_errors(x, GROUP, sh.share, [top, None], [has1, None], [5, 1], flat.parent, sh.mu, sh.kappa,
                                    [v1, np.array([np.nan])])
    e_two = tr.two_level_error(x, GROUP, lam, top, has1)
    bound = e_tree + e_two
    diff = np.abs(got.samples - two.samples)
    print('tree against reconcile, members: max share of the bound %.3f (max difference %.3g on values near %.3g)'
          % ((diff / bound).max(), diff.max(), np.abs(x).mean()))
    assert (diff <= bound).all() and not _bits(got.samples, two.samples)
    # a group without a total: untouched by both, bit for bit
    assert _bits(got.samples[GROUP == 1], x[GROUP == 1]) and _bits(two.samples[GROUP == 1], x[GROUP == 1])
    # the totals: acc + delta against acc + mu (top - acc)
    tbound = e_lvl[0] + tr.two_level_total_error(x, GROUP, mu, top, has1)
    tdiff = np.abs(got_ts - two_ts)
    live = np.bincount(GROUP, minlength=5) > 0
    print('tree against reconcile, totals: max share of the bound %.2e' % (tdiff[live] / tbound[live]).max())
    assert (tdiff <= tbound).all() and _bits(got_t.yhat[3], np.zeros(H))
    assert np.abs(got.samples - x).mean() > 1e9 * bound.max()


# ---- 4. coherence on the device -----------------------------------------------------------------------------------------

def test_every_level_sums_to_its_parent(env, case):
    """the members to their group, every level to the level above: the exact projection is coherent, so the bound is
    what tree_ref.solve_errors allows each summand and the parent to be off by, plus the test's own sum"""
    fc, _lib = env
    d = case
    S = 257
    with _filled(fc, d, S) as roll:
        roll.solve_tree(d['shares'])
        r = _reconcile(roll, d, samples=True)
        lv = [roll.tree_totals(level, [0.5], samples=True)[1] for level in (1, 2, 3)]
    tot = [_into(N_NODES[k], T_NODE[k], d['tx'][k]) for k in range(3)]
    sh = d['shares']
    e_b, e_c = tr.solve_errors(d['x'], GROUP, sh.share, tot, HAS, N_NODES, PARENT, sh.mu, sh.kappa, V)
    below, e_below, index = r.samples, e_b, GROUP
    for k in range(3):
        n = N_NODES[k]
        s, e_s, a_s = tr.gather(below, index, n), tr.gather(e_below, index, n), tr.gather(np.abs(below), index, n)
        n_ch = np.bincount(index, minlength=n)
        worst = 0.0
        for i in range(n):
            bound = e_s[i] + e_c[k][i] + tr.sum_bound(n_ch[i], a_s[i])
            err = np.abs(s[i] - lv[k][i])
            assert (err <= bound).all(), (k, i)
            if n_ch[i]:
                worst = max(worst, float((err / bound).max()))
        print('level %d: max |sum of children - node| / bound = %.3f' % (k + 1, worst))
        if k < 2:
            below, e_below, index = lv[k], e_c[k], PARENT[k]
    # (what it started from is incoherent by far more)
    assert np.abs(tr.gather(d['x'], GROUP, 5)[2] - tot[0][2]).mean() > 1e9 * e_c[0][2].max()


# ---- 5. chunk and output independence -----------------------------------------------------------------------------------

def test_chunk_independence(env):
    """20 members x 960 rows x 4096 samples with cum_q: 8 * 960 * (3 + 2 * 4096) bytes of scratch per series, 8 series per
    chunk, so one call runs 3 chunks (8 + 8 + 4); the same members reconciled in calls of 7, 6 and 7 (one chunk each)"""
    fc, _lib = env
    from tests.test_gpu_reconcile import _tiled
    m, c = _tiled('h960', 20, seed=9, key0=5)
    t, _ = _tiled('h960', 1, seed=10, key0=10 ** 12)
    assert c.H == 960 and (512 << 20) // (8 * 960 * (3 + 2 * 4096)) == 8
    group = np.arange(20, dtype=np.int64) % 3
    tree = fc.RollupTree(group, [3, 1], [np.zeros(3, dtype=np.int64)])
    sh = fc.reconcile_tree_shares(tree, node_weight=[[np.nan] * 3, [4.0]])
    lv = [0.1, 0.5, 0.9]

    def rec(roll, mm, sl):
        return roll.reconcile_tree(*mm.args(), group[sl], mm.keys, sh.share[sl], quantiles=lv, cumulative=True, **mm.kw())

    with fc.Rollup(c.fut, 3, uncertainty_samples=4096, seed=SEED) as roll:
        roll.add(*m.args(), group, m.keys, **m.kw())
        roll.set_tree(tree)
        roll.set_node_totals(2, *t.args(), np.zeros(1, dtype=np.int64), t.keys, **t.kw())
        roll.solve_tree(sh)
        one = rec(roll, m, slice(None))
        parts = [rec(roll, m.take(sl), sl) for sl in (slice(0, 7), slice(7, 13), slice(13, 20))]
    for k in ('yhat', 'q', 'cum_q'):
        assert _bits(getattr(one, k), np.concatenate([getattr(p, k) for p in parts])), k
    assert _bits(one.cum_q[:, :, 0], one.q[:, :, 0]) and (one.q[:, 1] != one.q[:, 0]).all()


def test_output_independence(env, case):
    """q alone (one sample buffer), q with cum_q (two: another scratch layout), q with samples, samples alone"""
    fc, _lib = env
    d = case
    with _filled(fc, d, 257) as roll:
        roll.solve_tree(d['shares'])
        full = _reconcile(roll, d, quantiles=LEVELS, cumulative=True, samples=True)
        q = _reconcile(roll, d, quantiles=LEVELS)
        qc = _reconcile(roll, d, quantiles=LEVELS, cumulative=True)
        qs = _reconcile(roll, d, quantiles=LEVELS, samples=True)
        s = _reconcile(roll, d, samples=True)
        for level in (1, 2, 3):
            tf = roll.tree_totals(level, LEVELS, cumulative=True, samples=True)
            tq = roll.tree_totals(level, LEVELS)
            tqc = roll.tree_totals(level, LEVELS, cumulative=True)
            tqs = roll.tree_totals(level, LEVELS, samples=True)
            assert tq.cum_q is None and _bits(tq.q, tf[0].q) and _bits(tqc.q, tf[0].q) and _bits(tqs[0].q, tf[0].q)
            assert _bits(tqc.cum_q, tf[0].cum_q) and _bits(tqs[1], tf[1]) and _bits(tq.yhat, tf[0].yhat)
    assert q.cum_q is None and q.samples is None and qc.samples is None and qs.cum_q is None and s.q is None
    for r in (q, qc, qs):
        assert _bits(r.q, full.q) and _bits(r.yhat, full.yhat)
    assert _bits(qc.cum_q, full.cum_q) and _bits(qs.samples, full.samples) and _bits(s.samples, full.samples)
    assert _bits(s.yhat, full.yhat)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals(env, case):
    """each < 0 with a message (or a ValueError before the library is touched); the handle stays usable, and a later
    valid sequence is bit-identical to the same on a fresh handle"""
    fc, _lib = env
    L = _lib.load()
    ctx = fc.get_context()
    d = case
    m, S = d['m'], 10
    sh = d['shares']
    mu, kappa = np.concatenate(sh.mu), np.concatenate(sh.kappa)
    cs = m.spec.to_c()
    p = lambda a: None if a is None else a.ctypes.data             # noqa: E731

    def message():
        return L.tsf_last_error(ctx.handle).decode()

    def series(s, group):
        group = np.ascontiguousarray(group, dtype=np.int64)
        keep = (np.ascontiguousarray(s.theta), np.ascontiguousarray(s.y_scale), np.ascontiguousarray(s.grid), s.keys, group)
        return keep, (ctypes.byref(cs), len(group), p(keep[0]), p(keep[1]), p(keep[2]), len(group), None, None, None, 1,
                      p(keep[3]), p(keep[4]))

    bufs = dict(yhat=np.zeros((9, H)), q=np.zeros((9, 5, H)))
    lv = np.ascontiguousarray(LEVELS)

    def read_members(roll):
        keep, a = series(m, GROUP)
        out = _lib.TsfReconcileOut(**{k: v.ctypes.data for k, v in bufs.items()})
        return L.tsf_rollup_reconcile_tree(roll._h, *a, p(sh.share), 5, p(lv), ctypes.byref(out))

    def read_level(roll, level, n0=0, n=1):
        out = _lib.TsfRollupOut(**{k: v.ctypes.data for k, v in bufs.items()})
        return L.tsf_rollup_tree_totals(roll._h, level, n0, n, 5, p(lv), ctypes.byref(out))

    def node_totals(roll, level, s, node):
        keep, a = series(s, node)
        return L.tsf_rollup_set_node_totals(roll._h, level, *a)

    roll = _filled(fc, d, S, totals=False, tree=False)
    # everything of the tree before set_tree
    assert L.tsf_rollup_solve_tree(roll._h, p(mu), p(kappa)) < 0 and 'before tsf_rollup_set_tree' in message()
    assert read_members(roll) < 0 and 'before tsf_rollup_set_tree' in message()
    assert read_level(roll, 1) < 0 and 'before tsf_rollup_set_tree' in message()
    assert node_totals(roll, 2, d['t'][1], T_NODE[1]) < 0 and 'before tsf_rollup_set_tree' in message()
    for call in (lambda: roll.solve_tree(sh), lambda: roll.tree_totals(1, [0.5]),
                 lambda: roll.set_node_totals(2, *d['t'][1].args(), T_NODE[1], d['t'][1].keys)):
        with pytest.raises(ValueError, match='no tree'):
            call()
    # a parent out of range, too many levels; then the tree, and a second one
    nn, par = np.array([3, 1], dtype=np.int64), np.concatenate(PARENT)
    bad_par = par.copy()
    bad_par[4] = 3
    assert L.tsf_rollup_set_tree(roll._h, 2, p(nn), p(bad_par)) < 0 and 'parent[4] = 3' in message()
    assert L.tsf_rollup_set_tree(roll._h, 5, p(nn), p(par)) < 0 and 'n_upper' in message()
    assert L.tsf_rollup_set_tree(roll._h, 0, p(nn), p(par)) < 0 and 'n_upper' in message()
    with pytest.raises(ValueError, match='groups'):
        roll.set_tree(fc.RollupTree(GROUP % 4, [4, 1], [np.zeros(4, dtype=np.int64)]))
    roll.set_tree(d['tree'])
    assert L.tsf_rollup_set_tree(roll._h, 2, p(nn), p(par)) < 0 and 'a tree already' in message()
    with pytest.raises(ValueError, match='a tree already'):
        roll.set_tree(d['tree'])
    # the reads before solve_tree
    assert read_members(roll) < 0 and 'not solved' in message()
    assert read_level(roll, 2) < 0 and 'not solved' in message()
    # levels out of range; a node out of range; a node given a total twice, in one call and over two
    for level in (1, 4, 0):
        assert node_totals(roll, level, d['t'][1], T_NODE[1]) < 0 and 'level = %d' % level in message()
        with pytest.raises(ValueError, match='level'):
            roll.set_node_totals(level, *d['t'][1].args(), T_NODE[1], d['t'][1].keys)
    assert node_totals(roll, 2, d['t'][1], [2, 3]) < 0 and 'group[1] = 3' in message()
    assert node_totals(roll, 2, d['t'][1], [1, 1]) < 0 and 'already' in message()
    with pytest.raises(ValueError, match='twice'):
        roll.set_node_totals(2, *d['t'][1].args(), [1, 1], d['t'][1].keys)
    roll.set_totals(*d['t'][0].args(), T_NODE[0], d['t'][0].keys)
    roll.set_node_totals(2, *d['t'][1].take(slice(0, 1)).args(), T_NODE[1][:1], d['t'][1].keys[:1])
    assert node_totals(roll, 2, d['t'][1], T_NODE[1]) < 0 and 'node[0] = 2' in message() and 'already' in message()
    roll.set_node_totals(2, *d['t'][1].take(slice(1, 2)).args(), T_NODE[1][1:], d['t'][1].keys[1:])
    roll.set_node_totals(3, *d['t'][2].args(), T_NODE[2], d['t'][2].keys)
    # shares outside [0, 1]
    for which, i, x in (('mu', 0, 1.5), ('kappa', 8, np.nan), ('kappa', 2, -1e-9)):
        a = dict(mu=mu.copy(), kappa=kappa.copy())
        a[which][i] = x
        assert L.tsf_rollup_solve_tree(roll._h, p(a['mu']), p(a['kappa'])) < 0 and '%s[%d]' % (which, i) in message()
    assert L.tsf_rollup_solve_tree(roll._h, None, p(kappa)) < 0
    with pytest.raises(ValueError, match='not of this tree'):
        roll.solve_tree(fc.reconcile_tree_shares(fc.RollupTree(GROUP, [5, 1], [np.zeros(5, dtype=np.int64)])))
    with pytest.raises(ValueError):
        roll.solve_tree((mu, kappa))
    roll.solve_tree(sh)
    assert read_members(roll) == 0 and read_level(roll, 3) == 0
    # levels and nodes out of range in the read
    for level in (0, 4):
        assert read_level(roll, level) < 0 and 'level = %d' % level in message()
        with pytest.raises(ValueError, match='level'):
            roll.tree_totals(level, [0.5])
    assert read_level(roll, 2, 2, 2) < 0 and 'nodes' in message()
    assert read_level(roll, 2, -1, 1) < 0 and 'nodes' in message()
    assert read_level(roll, 2, 3, 0) == 0                          # a legal no-op
    for nodes in ((0, 0), (3, 1), (-1, 2)):
        with pytest.raises(ValueError, match='nodes'):
            roll.tree_totals(2, [0.5], nodes=nodes)
    with pytest.raises(ValueError):
        roll.tree_totals(2, [])
    with pytest.raises(ValueError):
        _reconcile(roll, d, share=sh.share[:-1], samples=True)
    # a later add invalidates the solve; so do set_totals and set_node_totals (here refused ones do not)
    assert node_totals(roll, 2, d['t'][1], T_NODE[1]) < 0 and read_level(roll, 3) == 0
    roll.add(*m.take(slice(0, 1)).args(), GROUP[:1], np.array([4242], dtype=np.int64))
    assert read_members(roll) < 0 and 'not solved' in message()
    assert read_level(roll, 1) < 0 and 'not solved' in message()
    with pytest.raises(_lib.TsfError, match='not solved'):
        roll.tree_totals(2, [0.5])
    roll.solve_tree(sh)
    assert read_level(roll, 1) == 0
    roll.close()
    with pytest.raises(ValueError, match='closed'):
        roll.solve_tree(sh)
    # set_totals after a solve invalidates it as well; the sequence on this handle is what a fresh one gives
    with _filled(fc, d, S, totals=False) as roll:
        roll.solve_tree(sh)
        assert read_level(roll, 1) == 0
        roll.set_totals(*d['t'][0].args(), T_NODE[0], d['t'][0].keys)
        assert read_level(roll, 1) < 0 and 'not solved' in message()
        roll.solve_tree(sh)
        roll.set_node_totals(2, *d['t'][1].args(), T_NODE[1], d['t'][1].keys)
        assert read_members(roll) < 0 and 'not solved' in message()
        roll.set_node_totals(3, *d['t'][2].args(), T_NODE[2], d['t'][2].keys)
        roll.solve_tree(sh)
        got = _reconcile(roll, d, quantiles=LEVELS, cumulative=True, samples=True)
        got_t = [roll.tree_totals(level, LEVELS, cumulative=True, samples=True) for level in (1, 2, 3)]
    with _filled(fc, d, S) as fresh:
        fresh.solve_tree(sh)
        want = _reconcile(fresh, d, quantiles=LEVELS, cumulative=True, samples=True)
        want_t = [fresh.tree_totals(level, LEVELS, cumulative=True, samples=True) for level in (1, 2, 3)]
    for k in ('yhat', 'q', 'cum_q', 'samples'):
        assert _bits(getattr(got, k), getattr(want, k)), k
    for a, b in zip(got_t, want_t):
        assert _bits(a[1], b[1]) and _bits(a[0].q, b[0].q) and _bits(a[0].cum_q, b[0].cum_q) and _bits(a[0].yhat, b[0].yhat)
    # a tree on a roll-up with a noise correlation, either way round
    with fc.Rollup(d['cal'], 5, uncertainty_samples=S, seed=SEED, noise_corr=np.full(5, 0.3)) as corr:
        assert L.tsf_rollup_set_tree(corr._h, 2, p(nn), p(par)) < 0 and 'noise correlation' in message()
        with pytest.raises(ValueError, match='noise_corr'):
            corr.set_tree(d['tree'])


# ---- 7. plain C -------------------------------------------------------------------------------------------------------------

def test_abi_tree_plain_c(env, case, tmp_path):
    """tests/c/abi_tree.c drives shares / create / add twice / set_totals / set_tree / set_node_totals / solve_tree /
    reconcile_tree / tree_totals / free from plain C99 on the contract case and writes what they return"""
    fc, _lib = env
    d = case
    m, sh = d['m'], d['shares']
    p = str(tmp_path)
    files = [('spec.bin', np.frombuffer(bytes(m.spec.to_c()), dtype=np.uint8)), ('fut.i64', d['cal']), ('w.f64', d['w']),
             ('parent.i64', np.concatenate(PARENT)), ('v.f64', np.concatenate(V))]
    for prefix, s, group in [('', m, GROUP)] + [('t%d_' % (k + 1), d['t'][k], T_NODE[k]) for k in range(3)]:
        files += [(prefix + 'theta.f64', s.theta), (prefix + 'ys.f64', s.y_scale), (prefix + 'grid.bin', s.grid),
                  (prefix + 'key.i64', s.keys), (prefix + 'group.i64', group)]
    for name, a in files:
        np.ascontiguousarray(a).tofile(os.path.join(p, name))
    exe = p + '/abi_tree'
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    root = helpers.ROOT
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(root, 'include'),
                           os.path.join(root, 'tests', 'c', 'abi_tree.c'), '-o', exe, '-L', lib_dir, '-ltsf_amd',
                           '-Wl,-rpath,' + lib_dir])
    subprocess.check_call([exe, '9', str(H), p, '3'] + [str(n) for n in N_NODES] + [str(len(t)) for t in T_NODE])
    got = np.fromfile(p + '/out.f64')
    lv = [0.1, 0.5, 0.9]
    with fc.Rollup(d['cal'], 5, uncertainty_samples=50, seed=5) as roll:
        _add(roll, m.take(slice(0, 4)), GROUP[:4])
        _add(roll, m.take(slice(4, 9)), GROUP[4:])
        roll.set_totals(*d['t'][0].args(), T_NODE[0], d['t'][0].keys)
        roll.set_tree(d['tree'])
        for level in (2, 3):
            roll.set_node_totals(level, *d['t'][level - 1].args(), T_NODE[level - 1], d['t'][level - 1].keys)
        roll.solve_tree(sh)
        r = _reconcile(roll, d, quantiles=lv, cumulative=True, samples=True)
        tq = [roll.tree_totals(level, lv, cumulative=True, samples=True) for level in (1, 2, 3)]
    want = [sh.share, np.concatenate(sh.mu), np.concatenate(sh.kappa), r.yhat, r.q, r.cum_q, r.samples]
    for q, s in tq:
        want += [q.yhat, q.q, q.cum_q, s]
    want = np.concatenate([a.ravel() for a in want])
    assert got.shape == want.shape and helpers.n_bit_diff(got, want) == 0
