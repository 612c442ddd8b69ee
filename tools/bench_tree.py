"""Times tree reconciliation (forecaster.Rollup.set_tree / set_node_totals / solve_tree / reconcile_tree / tree_totals ->
tsf_rollup_set_tree / ... / tsf_rollup_tree_totals) beside the two-level reconciliation of the same roll-up and against
the same answer by hand: fc.predictive_samples of every member and every fitted total to the host, then the recursion in
numpy (sum the members' draws per group, the sweep up, the sweep down, the reconciled draws, their sort and the three
levels).

Panel: tools/bench_reconcile.py's (10 000 series, linear / additive, 90 daily steps on one shared future grid, groups
of --members consecutive series, the groups' fitted totals) with --regions regions of consecutive groups and one root
above them; every node's history is fc.aggregate_aligned of the level below, fitted like the members; 'struct' weights.
Everything is fitted once outside the timed region.  All routes run in one process: every repetition builds a roll-up
(add, set_totals, set_tree, set_node_totals: timed on their own), then times solve_tree, reconcile (two levels),
reconcile_tree and tree_totals per level; the first repetition is the warm-up and is dropped.  The host entry points
copy back and synchronise the device before they return.  reconcile's own spread over the repetitions is printed as the
run-to-run noise reconcile_tree is to be read against.  The by-hand side runs on the first --hand-series series only
(N * H * S * 8 bytes of draws on the host: 7 GB at the full size) and says so in its line; it is checked against the
device there (bit for bit, the contract).  Prints one JSON line per route; kernel_bytes is what the route's tree kernels
move per call (tree_member_kernel: two 8-byte reads and one write per (series, row, sample)), to be divided by the kernel
times of a separate profiler run over this tool (rocprofv3 --kernel-trace --stats).  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import timed  # noqa: E402

LEVELS = [0.1, 0.5, 0.9]


def _sum_into(n, index, x):
    out = np.zeros((n,) + x.shape[1:])
    for c in range(len(index)):
        out[index[c]] = out[index[c]] + x[c]
    return out


def _q(v, S):
    v = np.sort(v, axis=-1)
    out = []
    for p in LEVELS:
        pos = p * (S - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, S - 1)
        out.append(v[..., lo] + (v[..., hi] - v[..., lo]) * (pos - lo))
    return np.moveaxis(np.stack(out, axis=-1), -1, 1)


def by_hand(spec, fits, fut, tree, keys, shares, S):
    """the same answer through the host: fits = [members, level 1 totals, level 2, ...] (every node has a total) ->
    (member q [N][3][H], [per level q [n][3][H]])"""
    draws = [fc.predictive_samples(spec, f.theta, f.y_scale, f.grid, fut, series_key=k, uncertainty_samples=S, seed=0,
                                   floor=np.zeros(len(k)))['yhat'] for f, k in zip(fits, keys)]
    x, tot = draws[0], [0.0 + t for t in draws[1:]]
    L = tree.n_levels
    A, m = [_sum_into(tree.n_nodes[0], tree.group, x)], []
    for k in range(L):
        if k:
            A.append(_sum_into(tree.n_nodes[k], tree.parent[k - 1], m[k - 1]))
        m.append(A[k] + shares.mu[k][:, None, None] * (tot[k] - A[k]))
    c = [None] * L
    c[L - 1] = m[L - 1]
    for k in range(L - 2, -1, -1):
        p = tree.parent[k]
        c[k] = m[k] + shares.kappa[k][:, None, None] * (c[k + 1][p] - A[k + 1][p])
    delta = c[0] - A[0]
    x = x + shares.share[:, None, None] * delta[tree.group]
    return _q(x, S), [_q(A[0] + delta, S)] + [_q(ck, S) for ck in c[1:]]


class Cut(object):
    def __init__(self, r, k):
        self.theta, self.y_scale, self.grid = r.theta[:k], r.y_scale[:k], r.grid if len(r.grid) == 1 else r.grid[:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--members', type=int, default=20, help='series per group')
    ap.add_argument('--regions', type=int, default=50, help='regions above the groups (one root above them)')
    ap.add_argument('--hand-series', type=int, default=400, help='series of the by-hand side (whole regions)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    a = ap.parse_args()
    N, S = a.series, a.samples
    G = -(-N // a.members)
    per_region = -(-G // a.regions)
    R = -(-G // per_region)
    ds, y = synth.make_panel(N, 730, 'linear', seed=751)
    seas = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
    spec = fc.ModelSpec(growth='linear', seasonalities=seas)
    group = np.arange(N, dtype=np.int64) // a.members
    region = np.arange(G, dtype=np.int64) // per_region
    tree = fc.RollupTree(group, [G, R, 1], [region, np.zeros(R, dtype=np.int64)])
    hist = [y, fc.aggregate_aligned(y, group, G)]
    hist.append(fc.aggregate_aligned(hist[1], region, R))
    hist.append(fc.aggregate_aligned(hist[2], np.zeros(R, dtype=np.int64), 1))
    fits = [fc.fit_aligned(spec, ds, h) for h in hist]
    keys = [(np.int64(k) << 40) + np.arange(len(h), dtype=np.int64) for k, h in enumerate(hist)]
    fut = ds[-1] + synth.DAY_NS * np.arange(1, 91)
    H = len(fut)
    shares = fc.reconcile_tree_shares(tree, node_weight='struct')
    share2, _ = fc.reconcile_shares(group, G, total_weight='struct')
    base = dict(panel='cfg2', series=N, groups=G, regions=R, H=H, samples=S)
    args = [(spec, f.theta, f.y_scale, f.grid) for f in fits]
    kw = [dict(floor=np.zeros(len(k))) for k in keys]

    def build(roll, tr_, ar, ky, kws):
        """add, set_totals, set_tree, set_node_totals of levels 2 and 3 -> the four times"""
        t = [time.perf_counter()]
        roll.add(*ar[0], tr_.group, ky[0], **kws[0])
        t.append(time.perf_counter())
        roll.set_totals(*ar[1], np.arange(tr_.n_nodes[0]), ky[1], **kws[1])
        t.append(time.perf_counter())
        roll.set_tree(tr_)
        t.append(time.perf_counter())
        for level in (2, 3):
            roll.set_node_totals(level, *ar[level], np.arange(tr_.n_nodes[level - 1]), ky[level], **kws[level])
        t.append(time.perf_counter())
        return list(np.diff(t))

    names = ['add', 'set_totals', 'set_tree', 'set_node_totals (levels 2 and 3)', 'solve_tree',
             'reconcile 3 levels (two-level)', 'reconcile_tree 3 levels', 'reconcile 3 levels + cumulative (two-level)',
             'reconcile_tree 3 levels + cumulative', 'tree_totals level 1, 3 levels', 'tree_totals level 2, 3 levels',
             'tree_totals level 3, 3 levels']
    times = {k: [] for k in names}
    for rep in range(a.reps + 1):                        # (the first repetition is the warm-up)
        with fc.Rollup(fut, G, uncertainty_samples=S, seed=0) as roll:
            dt = build(roll, tree, args, keys, kw)
            t = [time.perf_counter()]
            roll.solve_tree(shares)
            t.append(time.perf_counter())
            for cumulative in (False, True):
                roll.reconcile(*args[0], group, keys[0], share2, quantiles=LEVELS, cumulative=cumulative, **kw[0])
                t.append(time.perf_counter())
                roll.reconcile_tree(*args[0], group, keys[0], shares.share, quantiles=LEVELS, cumulative=cumulative, **kw[0])
                t.append(time.perf_counter())
            for level in (1, 2, 3):
                roll.tree_totals(level, LEVELS)
                t.append(time.perf_counter())
        if rep:
            for k, d in zip(names, dt + list(np.diff(t))):
                times[k].append(float(d))
    M = G + R + 1
    # solve_tree: the blends read two cells and write one, the gathers read the children and write the parents, the
    # push-downs read three (at the groups four, with acc) and write one
    kernel_bytes = {'solve_tree': H * S * (24 * (G + R + 1) + 8 * (G + 2 * R + 1) + 32 * R + 40 * G),
                    'reconcile_tree 3 levels': 24 * N * H * S, 'reconcile_tree 3 levels + cumulative': 24 * N * H * S,
                    'reconcile 3 levels (two-level)': 32 * N * H * S,
                    'reconcile 3 levels + cumulative (two-level)': 32 * N * H * S,
                    'tree_totals level 1, 3 levels': 24 * G * H * S}
    for route, wall in times.items():
        extra = {'kernel_bytes': kernel_bytes[route]} if route in kernel_bytes else {}
        print(json.dumps(dict(base, nodes=M, route='rollup: ' + route, call_s=wall, best_ms=1e3 * min(wall),
                              spread_ms=1e3 * (max(wall) - min(wall)), **extra)), flush=True)
    for tag in ('3 levels', '3 levels + cumulative'):
        two, three = times['reconcile %s (two-level)' % tag], times['reconcile_tree ' + tag]
        noise = max(two) - min(two)
        print(json.dumps(dict(base, route='reconcile_tree against reconcile, ' + tag, reconcile_best_ms=1e3 * min(two),
                              reconcile_tree_best_ms=1e3 * min(three), reconcile_spread_ms=1e3 * noise,
                              slower_beyond_noise=bool(min(three) > min(two) + noise))), flush=True)

    # by hand, at a reduced size: the first whole regions and one root above them; and the device on the same
    per = a.members * per_region
    n = min(N, max(per, a.hand_series // per * per))
    g, r = n // a.members, n // per
    small_tree = fc.RollupTree(group[:n], [g, r, 1], [region[:g], np.zeros(r, dtype=np.int64)])
    sizes = [n, g, r, 1]
    cf = [Cut(f, k) for f, k in zip(fits, sizes)]
    ck = [k[:s] for k, s in zip(keys, sizes)]
    csh = fc.reconcile_tree_shares(small_tree, node_weight='struct')
    cargs = [(spec, f.theta, f.y_scale, f.grid) for f in cf]
    ckw = [dict(floor=np.zeros(s)) for s in sizes]
    hand = lambda: by_hand(spec, cf, fut, small_tree, ck, csh, S)  # noqa: E731

    def device():
        with fc.Rollup(fut, g, uncertainty_samples=S, seed=0) as roll:
            build(roll, small_tree, cargs, ck, ckw)
            roll.solve_tree(csh)
            q = roll.reconcile_tree(*cargs[0], group[:n], ck[0], csh.share, quantiles=LEVELS, **ckw[0]).q
            return q, [roll.tree_totals(level, LEVELS).q for level in (1, 2, 3)]
    hq, dq = hand(), device()
    same = all(np.array_equal(h.view(np.int64), d.view(np.int64)) for h, d in zip([hq[0]] + hq[1], [dq[0]] + dq[1]))
    small = dict(base, series=n, groups=g, regions=r,
                 note='reduced size: %d of %d series, so that the draws fit in host memory' % (n, N))
    for route, fn in (('by hand: predictive_samples to the host + numpy', hand),
                      ('device at the same reduced size: add .. solve_tree + reconcile_tree + tree_totals of 3 levels', device)):
        wall = timed(fn, a.reps)
        print(json.dumps(dict(small, route=route, call_s=wall, best_ms=1e3 * min(wall), bit_identical=bool(same),
                              host_bytes=8 * (n + g + r + 1) * H * S * 2)), flush=True)


if __name__ == '__main__':
    main()
