"""Times reconciliation in group roll-ups (forecaster.Rollup.set_totals / reconcile / reconciled_totals ->
tsf_rollup_set_totals / tsf_rollup_reconcile / tsf_rollup_reconciled_totals) against the same answer by hand:
fc.predictive_samples of every member and every total to the host, then numpy (sum the members' draws per group, the
incoherence, the reconciled draws, their sort and the three levels).

Panel: tools/bench_components.py's cfg2 (10 000 series, linear / additive, 90 daily steps on one shared future grid) in
groups of --members consecutive series; the totals' histories are fc.aggregate_aligned of the members', fitted like
them; 'struct' weights.  Everything is fitted once outside the timed region.  Every route is warmed up once, then timed
--reps times (the host entry points copy back and synchronise the device before they return); the roll-up's create, add
and free are outside the timed calls of reconciliation and are timed on their own.  The by-hand side runs on the first
--hand-series series only (N * H * S * 8 bytes of draws on the host: 7 GB at the full size) and says so in its line;
it is checked against the device there (bit for bit, the contract).  Prints one JSON line per route; the lines of the
two kernels' routes carry kernel_bytes, the bytes the kernel moves per call (reconcile_member_kernel: three 8-byte
reads and one write per (series, row, sample); reconcile_total_kernel: two reads and one write per (group, row,
sample)), to be divided by the kernel times of a separate profiler run over this tool (rocprofv3 --kernel-trace
--stats).  Not part of bench.py."""
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


def by_hand(spec, rm, rt, fut, group, keys, tkeys, share, share_total, S, kw):
    """the same answer through the host: -> (member q [N][3][H], total q [G][3][H])"""
    G = len(tkeys)
    x = fc.predictive_samples(spec, rm.theta, rm.y_scale, rm.grid, fut, series_key=keys, uncertainty_samples=S, seed=0,
                              **kw)['yhat']
    t = fc.predictive_samples(spec, rt.theta, rt.y_scale, rt.grid, fut, series_key=tkeys, uncertainty_samples=S, seed=0,
                              floor=np.zeros(G))['yhat']
    acc = np.zeros_like(t)
    for n in range(len(group)):
        acc[group[n]] = acc[group[n]] + x[n]
    d = (0.0 + t) - acc
    x = x + share[:, None, None] * d[group]
    tot = acc + share_total[:, None, None] * d

    def q(v):
        v = np.sort(v, axis=-1)
        out = []
        for p in LEVELS:
            pos = p * (S - 1)
            lo = int(np.floor(pos))
            hi = min(lo + 1, S - 1)
            out.append(v[..., lo] + (v[..., hi] - v[..., lo]) * (pos - lo))
        return np.moveaxis(np.stack(out, axis=-1), -1, 1)
    return q(x), q(tot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--members', type=int, default=20, help='series per group')
    ap.add_argument('--hand-series', type=int, default=400, help='series of the by-hand side (a multiple of --members)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    a = ap.parse_args()
    N, S = a.series, a.samples
    G = -(-N // a.members)
    ds, y = synth.make_panel(N, 730, 'linear', seed=751)
    seas = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
    spec = fc.ModelSpec(growth='linear', seasonalities=seas)
    keys = np.arange(N, dtype=np.int64)
    group = keys // a.members
    tkeys = (np.int64(1) << 40) + np.arange(G, dtype=np.int64)
    rm = fc.fit_aligned(spec, ds, y)
    rt = fc.fit_aligned(spec, ds, fc.aggregate_aligned(y, group, G))
    fut = ds[-1] + synth.DAY_NS * np.arange(1, 91)
    H = len(fut)
    kw = dict(floor=np.zeros(N))
    share, share_total = fc.reconcile_shares(group, G, total_weight='struct')
    base = dict(panel='cfg2', series=N, groups=G, H=H, samples=S)
    margs, targs = (spec, rm.theta, rm.y_scale, rm.grid), (spec, rt.theta, rt.y_scale, rt.grid)

    wall = timed(lambda: fc.predict_quantiles(*margs, fut, LEVELS, series_key=keys, uncertainty_samples=S, seed=0, **kw), a.reps)
    print(json.dumps(dict(base, route='predict_quantiles 3 levels (the unreconciled yardstick)', call_s=wall,
                          best_ms=1e3 * min(wall))), flush=True)
    times = {k: [] for k in ('add', 'set_totals', 'reconcile 3 levels', 'reconcile 3 levels + cumulative',
                             'reconciled_totals 3 levels', 'reconciled_totals 3 levels + cumulative')}
    for rep in range(a.reps + 1):                        # (the first repetition is the warm-up)
        with fc.Rollup(fut, G, uncertainty_samples=S, seed=0) as roll:
            t = [time.perf_counter()]
            roll.add(*margs, group, keys, **kw)
            t.append(time.perf_counter())
            roll.set_totals(*targs, np.arange(G), tkeys, floor=np.zeros(G))
            t.append(time.perf_counter())
            roll.reconcile(*margs, group, keys, share, quantiles=LEVELS, **kw)
            t.append(time.perf_counter())
            roll.reconcile(*margs, group, keys, share, quantiles=LEVELS, cumulative=True, **kw)
            t.append(time.perf_counter())
            roll.reconciled_totals(share_total, LEVELS)
            t.append(time.perf_counter())
            roll.reconciled_totals(share_total, LEVELS, cumulative=True)
            t.append(time.perf_counter())
        if rep:
            for k, dt in zip(times, np.diff(t)):
                times[k].append(float(dt))
    kernel_bytes = {'reconcile 3 levels': 32 * N * H * S, 'reconcile 3 levels + cumulative': 32 * N * H * S,
                    'reconciled_totals 3 levels': 24 * G * H * S, 'reconciled_totals 3 levels + cumulative': 24 * G * H * S}
    for route, wall in times.items():
        extra = {'kernel_bytes': kernel_bytes[route]} if route in kernel_bytes else {}
        print(json.dumps(dict(base, route='rollup: ' + route, call_s=wall, best_ms=1e3 * min(wall), **extra)), flush=True)

    # by hand, at a reduced size: the first n series (whole groups) and their totals; and the device on the same
    n = min(N, max(a.members, a.hand_series // a.members * a.members))
    g = n // a.members

    class Cut(object):
        def __init__(self, r, k):
            self.theta, self.y_scale, self.grid = r.theta[:k], r.y_scale[:k], r.grid if len(r.grid) == 1 else r.grid[:k]
    cm, ct, ckw = Cut(rm, n), Cut(rt, g), dict(floor=np.zeros(n))
    hand = lambda: by_hand(spec, cm, ct, fut, group[:n], keys[:n], tkeys[:g], share[:n], share_total[:g], S, ckw)  # noqa: E731

    def device():
        with fc.Rollup(fut, g, uncertainty_samples=S, seed=0) as roll:
            roll.add(spec, cm.theta, cm.y_scale, cm.grid, group[:n], keys[:n], **ckw)
            roll.set_totals(spec, ct.theta, ct.y_scale, ct.grid, np.arange(g), tkeys[:g], floor=np.zeros(g))
            r = roll.reconcile(spec, cm.theta, cm.y_scale, cm.grid, group[:n], keys[:n], share[:n], quantiles=LEVELS, **ckw)
            return r.q, roll.reconciled_totals(share_total[:g], LEVELS).q
    hq, dq = hand(), device()
    same = all(np.array_equal(h.view(np.int64), d.view(np.int64)) for h, d in zip(hq, dq))
    small = dict(base, series=n, groups=g, note='reduced size: %d of %d series, so that the draws fit in host memory' % (n, N))
    for route, fn in (('by hand: predictive_samples to the host + numpy', hand),
                      ('device at the same reduced size: add + set_totals + reconcile + reconciled_totals', device)):
        wall = timed(fn, a.reps)
        print(json.dumps(dict(small, route=route, call_s=wall, best_ms=1e3 * min(wall), bit_identical=bool(same),
                              host_bytes=8 * (n + g) * H * S * 2)), flush=True)


if __name__ == '__main__':
    main()
