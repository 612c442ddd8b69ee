"""Times the totals over row windows (forecaster.predict_windows -> tsf_predict_windows) against the per-row quantiles
they extend and against the by-hand route they replace.

Panel: tools/bench_components.py's cfg2 (10 000 series, linear / additive, 90 daily steps on one shared future grid),
models fitted once outside the timed region.  Routes, every one warmed up once, then timed --reps times (the host entry
points copy back and synchronise the device before they return):
  predict_quantiles at 3 levels, and the same with cumulative=True (a second sample buffer: half the chunk);
  predict_windows over the calendar weeks and months of the 90 rows (disjoint windows: one draw, one pass over the
  sample buffer, one sort per window instead of one per row);
  predict_windows over the 84 rolling 7-row windows (they overlap: the buffer is read 6.5 times);
  by hand: predictive_samples to the host, the window sums and np.quantile in numpy, on the first --sample-series series
  only (the raw draws are [N][H][samples] float64 per array on the host).
Prints one JSON line per route.  No time is asserted anywhere.  Kernel times come from a separate profiler run over this
tool (rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc  # noqa: E402
from tools.bench_components import panels, timed  # noqa: E402

LEVELS = [0.1, 0.5, 0.9]


def by_hand(args, kw, dr, w):
    draws = fc.predictive_samples(*args, **kw, **dr)['yhat']
    sums = np.stack([draws[:, a:b].sum(axis=1) for a, b in zip(w.start, w.end)], axis=1)
    return np.quantile(sums, LEVELS, axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--sample-series', type=int, default=400)
    ap.add_argument('--routes', help='comma-separated substrings of the route names to run (default: all)')
    a = ap.parse_args()
    for name, spec, r, fut, kw in panels(a.series, 'cfg2'):
        H = fut.shape[-1]
        args = (spec, r.theta, r.y_scale, r.grid, fut)
        dr = dict(uncertainty_samples=a.samples, seed=0)
        weeks, months = fc.period_windows(fut, 'W'), fc.period_windows(fut, 'M')
        periods = fc.Windows(np.concatenate([weeks.start, months.start]), np.concatenate([weeks.end, months.end]),
                             np.concatenate([weeks.label_ns, months.label_ns]))
        rolling = fc.row_windows(H, 7, step=1)
        m = min(a.sample_series, a.series)
        sub = (spec, r.theta[:m], r.y_scale[:m], r.grid if len(r.grid) == 1 else r.grid[:m], fut)
        skw = {k: v[:m] for k, v in kw.items()}
        routes = [('predict_quantiles 3 levels', a.series, H, lambda: fc.predict_quantiles(*args, LEVELS, **kw, **dr)),
                  ('predict_quantiles 3 levels + cumulative', a.series, H,
                   lambda: fc.predict_quantiles(*args, LEVELS, cumulative=True, **kw, **dr)),
                  ('predict_windows %d weeks + %d months' % (len(weeks), len(months)), a.series, len(periods),
                   lambda: fc.predict_windows(*args, periods, LEVELS, **kw, **dr)),
                  ('predict_windows %d rolling 7-row windows' % len(rolling), a.series, len(rolling),
                   lambda: fc.predict_windows(*args, rolling, LEVELS, **kw, **dr)),
                  ('by hand: predictive_samples + numpy, weeks + months', m, len(periods),
                   lambda: by_hand(sub, skw, dr, periods))]
        for route, n, sorts, fn in routes:
            if a.routes and not any(s in route for s in a.routes.split(',')):
                continue
            wall = timed(fn, a.reps)
            print(json.dumps({'panel': name, 'route': route, 'series': n, 'H': H, 'sorts_per_series': sorts,
                              'samples': a.samples, 'call_s': wall, 'best_ms': 1e3 * min(wall)}), flush=True)


if __name__ == '__main__':
    main()
