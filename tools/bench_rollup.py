"""Times the group roll-ups (forecaster.Rollup -> tsf_rollup_add / tsf_rollup_quantiles) against the per-series
quantiles whose draw loop they share: fc.predict_quantiles with 3 levels is the yardstick (one draw and one sort per
(series, row)), then a Rollup of the same panel -- add (the same draws, one streaming pass over each chunk's samples
instead of the per-series sorts) and quantiles (one sort per (group, row)) -- for G = 1, 100 and 10 000 groups
(group = series index mod G; G = the series count makes every group one series), all in the same run.

Panel: tools/bench_components.py's cfg2 (10 000 series, linear / additive, 90 daily steps on one shared future grid),
models fitted once outside the timed region.  Every route is warmed up once, then timed --reps times (the host entry
points copy back and synchronise the device before they return); the roll-up's create and free are outside its two timed
calls.  Prints one JSON line per route.  Kernel times come from a separate profiler run over this tool
(rocprofv3 --kernel-trace --stats).  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc  # noqa: E402
from tools.bench_components import panels, timed  # noqa: E402

LEVELS = [0.1, 0.5, 0.9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--groups', default='1,100,10000', help='comma-separated group counts (each at most --series)')
    a = ap.parse_args()
    (name, spec, r, fut, kw), = panels(a.series, 'cfg2')
    H, N = fut.shape[-1], a.series
    keys = np.arange(N, dtype=np.int64)
    base = dict(panel=name, series=N, H=H, samples=a.samples)
    wall = timed(lambda: fc.predict_quantiles(spec, r.theta, r.y_scale, r.grid, fut, LEVELS, series_key=keys,
                                              uncertainty_samples=a.samples, seed=0, **kw), a.reps)
    print(json.dumps(dict(base, route='predict_quantiles 3 levels', call_s=wall, best_ms=1e3 * min(wall))), flush=True)
    for G in [min(int(g), N) for g in a.groups.split(',')]:
        group = keys % G
        t_add, t_q, t_cq = [], [], []
        for rep in range(a.reps + 1):                    # (the first repetition is the warm-up)
            with fc.Rollup(fut, G, uncertainty_samples=a.samples, seed=0) as roll:
                t0 = time.perf_counter()
                roll.add(spec, r.theta, r.y_scale, r.grid, group, keys, **kw)
                t1 = time.perf_counter()
                roll.quantiles(LEVELS)
                t2 = time.perf_counter()
                roll.quantiles(LEVELS, cumulative=True)
                t3 = time.perf_counter()
            if rep:
                t_add.append(t1 - t0)
                t_q.append(t2 - t1)
                t_cq.append(t3 - t2)
        for route, wall in (('add', t_add), ('quantiles 3 levels', t_q), ('quantiles 3 levels + cumulative', t_cq)):
            print(json.dumps(dict(base, route='rollup G=%d: %s' % (G, route), groups=G, call_s=wall,
                                  best_ms=1e3 * min(wall))), flush=True)


if __name__ == '__main__':
    main()
