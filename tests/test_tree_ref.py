"""CPU tests of tree reconciliation's host side (include/tsf.h "tree reconciliation"): tsf_reconcile_tree_shares against
the numpy restatement of tests/tree_ref.py bit for bit, its refusals, fc.rollup_tree and fc.reconcile_tree_shares, and
the restatement itself against the dense weighted least squares projection in np.longdouble and against coherence, both
within bounds derived from the operations themselves (tree_ref.solve_errors: a running error analysis)."""
import numpy as np
import pytest

from tests import tree_ref as tr
from tests.tree_ref import GROUP, N_NODES, PARENT, V

# a chain of single children: 3 members in one group, four levels of one node above it
CHAIN = (np.zeros(3, dtype=np.int64), [1, 1, 1, 1, 1], [np.zeros(1, dtype=np.int64)] * 4,
         [np.array([0.8]), np.array([np.nan]), np.array([1.7]), np.array([0.4]), np.array([3.0])])
S = 257


@pytest.fixture(scope='module')
def lib(built):
    from time_series_spark_amd import _lib, forecaster as fc
    return _lib.load(), fc, _lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _call(L, group, w, n_nodes, parent, v):
    group = np.ascontiguousarray(group, dtype=np.int64)
    nn = np.ascontiguousarray(n_nodes[1:], dtype=np.int64)
    par = np.ascontiguousarray(np.concatenate(list(parent) + [np.zeros(0, dtype=np.int64)]), dtype=np.int64)
    v = np.ascontiguousarray(np.concatenate(v), dtype=np.float64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    M = int(np.sum(n_nodes))
    share, mu, e, kappa = np.full(len(group), -7.0), np.full(M, -7.0), np.full(M, -7.0), np.full(M, -7.0)
    rc = L.tsf_reconcile_tree_shares(len(group), group.ctypes.data, None if w is None else w.ctypes.data, n_nodes[0],
                                     len(nn), nn.ctypes.data, par.ctypes.data, v.ctypes.data, share.ctypes.data,
                                     mu.ctypes.data, e.ctypes.data, kappa.ctypes.data)
    return rc, share, mu, e, kappa


def test_exports(lib):
    L, fc, _lib = lib
    for sym in ('tsf_reconcile_tree_shares', 'tsf_rollup_set_tree', 'tsf_rollup_set_node_totals', 'tsf_rollup_solve_tree',
                'tsf_rollup_reconcile_tree', 'tsf_rollup_tree_totals'):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert _lib.TREE_MAX_LEVELS == 4


@pytest.mark.parametrize('weights', ['given', 'null'])
def test_shares_are_the_restatement(lib, weights):
    L, fc, _lib = lib
    w = None if weights == 'null' else np.random.default_rng(3).uniform(1e-3, 30.0, len(GROUP))
    rc, share, mu, e, kappa = _call(L, GROUP, w, N_NODES, PARENT, V)
    assert rc == 0
    want = tr.shares(GROUP, w, N_NODES, PARENT, V)
    assert _bits(share, want[0])
    for got, ref in zip((mu, e, kappa), want[1:]):
        assert _bits(got, np.concatenate(ref))
    mu, e, kappa = (np.split(a, [5, 8]) for a in (mu, e, kappa))
    # the empty group: +0.0 everywhere; no total: mu = +0.0 and e = E; the root: kappa = +0.0
    assert _bits([mu[0][3], e[0][3], kappa[0][3]], np.zeros(3)) and _bits([mu[0][1], mu[1][0]], np.zeros(2))
    assert _bits(kappa[2], np.zeros(1)) and e[0][1] == (2.0 if w is None else w[1] + w[2])
    # the single child takes all of what its parent moves by; siblings' kappa sum to 1; shares sum to 1 per group
    assert kappa[0][4] == 1.0 and abs(kappa[0][0] + kappa[0][1] - 1) < 1e-15 and abs(kappa[1].sum() - 1) < 1e-15
    assert all(abs(share[GROUP == g].sum() - 1) < 1e-15 for g in (0, 1, 2, 4))
    assert (mu[0][[0, 2, 4]] > 0).all() and (np.concatenate(mu) < 1).all() and (np.concatenate(kappa) <= 1).all()


def test_shares_refusals(lib):
    L, fc, _lib = lib
    w = np.ones(len(GROUP))

    def bad(a, i, x):
        a = a.copy()
        a[i] = x
        return a

    assert _call(L, GROUP, w, N_NODES, PARENT, V)[0] == 0
    for g in (-1, 5):
        assert _call(L, bad(GROUP, 6, g), w, N_NODES, PARENT, V)[0] == -1
    for p in (-1, 3):
        assert _call(L, GROUP, w, N_NODES, [bad(PARENT[0], 2, p), PARENT[1]], V)[0] == -1
    assert _call(L, GROUP, w, N_NODES, [PARENT[0], bad(PARENT[1], 1, 1)], V)[0] == -1
    for x in (0.0, -1.0, np.inf, np.nan):
        assert _call(L, GROUP, bad(w, 2, x), N_NODES, PARENT, V)[0] == -1, x
    for x in (0.0, -2.0, np.inf, -np.inf):
        assert _call(L, GROUP, w, N_NODES, PARENT, [V[0], bad(V[1], 1, x), V[2]])[0] == -1, x
    assert _call(L, GROUP, w, N_NODES, PARENT, [V[0], bad(V[1], 1, np.nan), V[2]])[0] == 0
    # TSF_TREE_MAX_LEVELS levels above the groups are taken, one more is refused
    chain = lambda k: (np.zeros(3, dtype=np.int64), None, [1] * (k + 1), [np.zeros(1, dtype=np.int64)] * k,   # noqa: E731
                       [np.ones(1)] * (k + 1))
    assert _call(L, *chain(4))[0] == 0 and _call(L, *chain(5))[0] == -1
    assert _call(L, *chain(0))[0] == 0


def test_rollup_tree(lib):
    L, fc, _lib = lib
    series = np.array([11, 11, 12, 12, 12, 13, 14, 14, 14])
    region = np.array([7, 7, 7, 7, 7, 9, 9, 9, 9])
    world = np.zeros(9, dtype=np.int64)
    t = fc.rollup_tree([series, region, world])
    assert isinstance(t, fc.RollupTree) and t.n_nodes == [4, 2, 1] and t.n_levels == 3
    assert list(t.group) == [0, 0, 1, 1, 1, 2, 3, 3, 3] and list(t.parent[0]) == [0, 0, 1, 1] and list(t.parent[1]) == [0, 0]
    assert [list(u) for u in t.labels] == [[11, 12, 13, 14], [7, 9], [0]]
    assert [list(c) for c in t.member_counts()] == [[2, 3, 1, 3], [5, 4], [9]]
    assert fc.rollup_tree([series]).n_levels == 1
    with pytest.raises(ValueError, match='differ in length'):
        fc.rollup_tree([series, region[:-1]])
    with pytest.raises(ValueError, match='two different parents'):
        fc.rollup_tree([series, np.array([7, 9, 7, 7, 7, 9, 9, 9, 9])])
    with pytest.raises(ValueError):
        fc.rollup_tree([])
    with pytest.raises(ValueError):
        fc.rollup_tree([series.astype(np.float64), region])
    # built by hand: an empty group is legal, a parent out of range is not
    assert fc.RollupTree(GROUP, N_NODES, PARENT).member_counts()[1].tolist() == [3, 4, 2]
    for args in ((GROUP, N_NODES, [PARENT[0]]), (GROUP, N_NODES, [PARENT[0], np.array([0, 1, 0])]),
                 (GROUP + 1, N_NODES, PARENT), (GROUP, [5, 3, 0], PARENT), (GROUP, [5] + [1] * 5, PARENT)):
        with pytest.raises(ValueError):
            fc.RollupTree(*args)


def test_python_policies(lib):
    L, fc, _lib = lib
    t = fc.RollupTree(GROUP, N_NODES, PARENT)
    w = np.linspace(0.5, 2.0, len(GROUP))
    s = fc.reconcile_tree_shares(t, weight=w, node_weight=V)
    want = tr.shares(GROUP, w, N_NODES, PARENT, V)
    assert _bits(s.share, want[0])
    for got, ref in zip((s.mu, s.e, s.kappa), want[1:]):
        assert len(got) == 3 and all(_bits(a, b) for a, b in zip(got, ref))
    s = fc.reconcile_tree_shares(t)                                 # 'struct': the member count, none for the empty group
    want = tr.shares(GROUP, None, N_NODES, PARENT, [np.array([1, 2, 4, np.nan, 2.0]), np.array([3.0, 4, 2]), np.array([9.0])])
    assert all(_bits(a, b) for a, b in zip(s.mu + s.kappa, want[1] + want[3])) and _bits(s.mu[0][:3], [0.5] * 3)
    s = fc.reconcile_tree_shares(t, node_weight='ols')
    assert _bits(s.mu[0], [0.5, 2 / 3.0, 0.8, 0.0, 2 / 3.0])
    for kw in (dict(weight=w[:-1]), dict(weight=-w), dict(node_weight='mint'), dict(node_weight=V[:2]),
               dict(node_weight=[V[0], V[1], -V[2]]), dict(node_weight=[V[0][:4], V[1], V[2]])):
        with pytest.raises(ValueError):
            fc.reconcile_tree_shares(t, **kw)
    with pytest.raises(ValueError):
        fc.reconcile_tree_shares((GROUP, N_NODES, PARENT))


# ---- the restatement alone: the projection and coherence ---------------------------------------------------------------

def _synthetic(group, n_nodes, parent, v, seed):
    """draws x ~ N(10, 2^2) of the members and t of every node around the node's member count times 10, one row, S
    samples; a total for every node whose v is a number -> dict with the restatement's solution and its error analysis"""
    rng = np.random.default_rng(seed)
    N = len(group)
    w = rng.uniform(0.5, 2.0, N)
    x = rng.normal(10, 2, (N, S))
    cnt = [np.bincount(group, minlength=n_nodes[0])]
    for k in range(1, len(n_nodes)):
        cnt.append(np.bincount(parent[k - 1], weights=cnt[-1], minlength=n_nodes[k]))
    tot = [rng.normal(10.0 * c[:, None] + 1.0, 3, (len(c), S)) for c in cnt]
    has = [(~np.isnan(vk)).astype(np.int32) for vk in v]
    share, mu, e, kappa = tr.shares(group, w, n_nodes, parent, v)
    acc = tr.gather(x, group, n_nodes[0])
    delta, c, A = tr.solve(acc, tot, has, n_nodes, parent, mu, kappa)
    e_b, e_c = tr.solve_errors(x, group, share, tot, has, n_nodes, parent, mu, kappa, v)
    return dict(group=group, n_nodes=n_nodes, parent=parent, v=v, w=w, x=x, tot=tot, acc=acc, c=c, e_b=e_b, e_c=e_c,
                b=tr.members(x, group, share, delta), c1=tr.group_totals(acc, delta))


@pytest.fixture(scope='module', params=['tree', 'chain'])
def solved(request):
    if request.param == 'tree':
        return _synthetic(GROUP, N_NODES, PARENT, V, 0)
    return _synthetic(*CHAIN, seed=1)


def test_restatement_is_the_dense_projection(solved):
    """within tree_ref.solve_errors: the running error analysis of the operations, plus the reference's own error"""
    s = solved
    want, ref_err = tr.dense(s['x'], s['w'], s['group'], s['n_nodes'], s['parent'], s['tot'], s['v'])
    err = np.abs(s['b'].astype(np.longdouble) - want).astype(np.float64)
    bound = s['e_b'] + ref_err
    print('%d levels: max |recursion - dense| = %.3g (relative %.3g), max share of the bound %.3f; the reference\'s own '
          'allowance is %.2g of the bound' % (len(s['n_nodes']), err.max(), (err / np.abs(want).astype(np.float64)).max(),
                                             (err / bound).max(), (ref_err / bound).max()))
    assert (err <= bound).all() and (ref_err < 0.05 * bound).all()
    # the projection moved the members by far more than the bound: it is not vacuous
    assert np.abs(s['b'] - s['x']).mean() > 1e10 * bound.max()


def test_every_level_sums_to_its_parent(solved):
    """the members to c_1 = acc + delta, every level's c to the level above: the exact projection is coherent, so the
    bound is what solve_errors allows each summand and the parent to be off by, plus the test's own sum (sum_bound)"""
    s = solved
    below, e_below, index, above = s['b'], s['e_b'], s['group'], [s['c1']] + s['c'][1:]
    worst = 0.0
    for k in range(len(s['n_nodes'])):
        n = s['n_nodes'][k]
        tot, e_tot, absum = tr.gather(below, index, n), tr.gather(e_below, index, n), tr.gather(np.abs(below), index, n)
        n_ch = np.bincount(index, minlength=n)
        for i in range(n):
            bound = e_tot[i] + s['e_c'][k][i] + tr.sum_bound(n_ch[i], absum[i])
            err = np.abs(tot[i] - above[k][i])
            if n_ch[i]:
                worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (k, i)
        if k + 1 < len(s['n_nodes']):
            below, e_below, index = above[k], s['e_c'][k], s['parent'][k]
    print('%d levels: max |sum of children - parent| / bound = %.3f' % (len(s['n_nodes']), worst))
    # an empty node stays +0.0
    if len(s['n_nodes']) == 3:
        assert _bits(s['c1'][3], np.zeros(S))


def test_no_total_is_neutral():
    s = _synthetic(GROUP, N_NODES, PARENT, [np.full(5, np.nan), np.full(3, np.nan), np.full(1, np.nan)], 2)
    assert _bits(s['b'], s['x']) and _bits(s['c1'], s['acc'])


def test_one_upper_level_without_totals_is_the_two_level_solution():
    """in exact arithmetic; here within the sum of the two error analyses (each side is that close to the projection)"""
    from tests import reconcile_ref as rr
    v1, par = V[0], [np.zeros(5, dtype=np.int64)]
    s = _synthetic(GROUP, [5, 1], par, [v1, np.array([np.nan])], 4)
    has = ~np.isnan(v1)
    lam, mu = rr.shares(GROUP, s['w'], 5, v1)
    two = rr.members(s['x'], GROUP, lam, rr.incoherence(s['tot'][0], s['acc'], has))
    bound = s['e_b'] + tr.two_level_error(s['x'], GROUP, lam, s['tot'][0], has)
    diff = np.abs(two - s['b'])
    print('tree against two levels: max share of the bound %.3f' % (diff[bound > 0] / bound[bound > 0]).max())
    assert (diff <= bound).all() and not _bits(two, s['b'])
