"""Times temporal reconciliation (forecaster.predict_temporal -> tsf_predict_temporal) against the unreconciled pair it
replaces (predict_quantiles on the days plus predict_windows on the weeks) and against the same answer by hand:
fc.predictive_samples of both models to the host, then numpy (the window sums, the incoherence, the reconciled draws,
their sort and the three levels).

Panel: tools/bench_components.py's cfg2 (10 000 series, linear / additive, 90 daily steps on one shared future grid) and a
second model per series fitted on the weekly totals of the history (period_history(ds, y, 'W'): the full weeks; linear,
yearly seasonality only).  The windows are the calendar weeks of the 90 future days, the full ones reconciled ('struct'
weights), the partial ones at either end left as they are.  Everything is fitted once outside the timed region.  Every
route is warmed up once, then timed --reps times (the host entry points copy back and synchronise the device before they
return).  The by-hand side runs on the first --hand-series series only (N * H * S * 8 bytes of draws on the host: 7 GB
at the full size) and says so in its line; it is checked against the device there (bit for bit, the contract).  Prints
one JSON line per route; the predict_temporal lines carry kernel_bytes, the bytes temporal_reconcile_kernel moves per
call (two 8-byte reads and one write per (series, row of a window, sample), one read and one write per (series, window,
sample)), to be divided by the kernel time of a separate profiler run.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import timed  # noqa: E402

LEVELS = [0.1, 0.5, 0.9]


def by_hand(day, week, fut, w, shares, keys, pkeys, S):
    """the same answer through the host: -> (q [N][3][H], win_q [N][3][K])"""
    x = fc.predictive_samples(*day, fut, series_key=keys, uncertainty_samples=S, seed=0)['yhat']
    t = fc.predictive_samples(*week, w.label_ns, series_key=pkeys, uncertainty_samples=S, seed=0)['yhat']
    win = np.empty_like(t)
    for k, (a, b) in enumerate(zip(w.start, w.end)):
        c = x[:, a].copy()
        for h in range(a + 1, b):
            c = c + x[:, h]
        mu = shares.share_total[:, k]
        active = ~np.isnan(mu)
        d = np.where(active[:, None], t[:, k] - c, 0.0)
        win[:, k] = c + np.where(active, mu, 0.0)[:, None] * d
        for h in range(a, b):
            x[:, h] = x[:, h] + shares.share[:, h, None] * d

    def q(v):
        v = np.sort(v, axis=-1)
        out = []
        for p in LEVELS:
            pos = p * (S - 1)
            lo = int(np.floor(pos))
            hi = min(lo + 1, S - 1)
            out.append(v[..., lo] + (v[..., hi] - v[..., lo]) * (pos - lo))
        return np.moveaxis(np.stack(out, axis=-1), -1, 1)
    return q(x), q(win)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--hand-series', type=int, default=400, help='series of the by-hand side')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    a = ap.parse_args()
    N, S = a.series, a.samples
    ds, y = synth.make_panel(N, 730, 'linear', seed=751)
    seas = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
    spec = fc.ModelSpec(growth='linear', seasonalities=seas)
    pspec = fc.ModelSpec(growth='linear', n_changepoints=10,
                         seasonalities=[{'name': 'yearly', 'period': 365.25, 'fourier_order': 5}])
    ds_p, y_p, hist = fc.period_history(ds, y, 'W')
    rd, rw = fc.fit_aligned(spec, ds, y), fc.fit_aligned(pspec, ds_p, y_p)
    fut = ds[-1] + synth.DAY_NS * np.arange(1, 91)
    H = len(fut)
    w = fc.period_windows(fut, 'W')
    K = len(w)
    shares = fc.temporal_shares(w, N, H, period_weight='struct')
    n_active = int((~np.isnan(shares.share_total[0])).sum())
    keys = np.arange(N, dtype=np.int64)
    pkeys = (np.int64(1) << 40) + keys
    day, week = (spec, rd.theta, rd.y_scale, rd.grid), (pspec, rw.theta, rw.y_scale, rw.grid)
    base = dict(panel='cfg2', series=N, H=H, windows=K, reconciled_windows=n_active, history_weeks=len(hist), samples=S)
    kw = dict(uncertainty_samples=S, seed=0)
    rows_in_windows = int(w.n_rows.sum())
    kernel_bytes = 8 * N * S * (3 * rows_in_windows + 2 * K)

    def temporal(cumulative):
        return fc.predict_temporal(*day, fut, w, *week, w.label_ns, shares, LEVELS, keys, pkeys, cumulative=cumulative, **kw)

    def unreconciled():
        return (fc.predict_quantiles(*day, fut, LEVELS, series_key=keys, **kw),
                fc.predict_windows(*day, fut, w, LEVELS, series_key=keys, **kw))

    for route, fn, extra in (('predict_temporal 3 levels', lambda: temporal(False), dict(kernel_bytes=kernel_bytes)),
                             ('predict_temporal 3 levels + cumulative', lambda: temporal(True), dict(kernel_bytes=kernel_bytes)),
                             ('predict_quantiles + predict_windows 3 levels (the unreconciled pair)', unreconciled, {})):
        wall = timed(fn, a.reps)
        print(json.dumps(dict(base, route=route, call_s=wall, best_ms=1e3 * min(wall), **extra)), flush=True)

    # by hand, at a reduced size: the first n series; and the device on the same
    n = min(N, a.hand_series)

    def cut(m):
        return m[0], m[1][:n], m[2][:n], m[3] if len(m[3]) == 1 else m[3][:n]
    cd, cw = cut(day), cut(week)
    cs = fc.TemporalShares(w, shares.share[:n], shares.share_total[:n])
    hand = lambda: by_hand(cd, cw, fut, w, cs, keys[:n], pkeys[:n], S)  # noqa: E731

    def device():
        r = fc.predict_temporal(*cd, fut, w, *cw, w.label_ns, cs, LEVELS, keys[:n], pkeys[:n], **kw)
        return r.q, r.win_q
    same = all(np.array_equal(h.view(np.int64), d.view(np.int64)) for h, d in zip(hand(), device()))
    small = dict(base, series=n, note='reduced size: %d of %d series, so that the draws fit in host memory' % (n, N))
    for route, fn in (('by hand: predictive_samples of both models to the host + numpy', hand),
                      ('predict_temporal 3 levels at the same reduced size', device)):
        wall = timed(fn, a.reps)
        print(json.dumps(dict(small, route=route, call_s=wall, best_ms=1e3 * min(wall), bit_identical=bool(same),
                              host_bytes=8 * n * (H + K) * S * 2)), flush=True)


if __name__ == '__main__':
    main()
