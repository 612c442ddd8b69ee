"""Times the correlated group roll-ups (include/tsf.h "correlated group roll-ups") beside the independent ones, in the
same run: forecaster.Rollup.add without and with a noise correlation (rho = 0.3 in every group: no group takes the
rho = 0 shortcut) for G = 1, 100 and 10 000 groups (group = series index mod G), then the estimator,
forecaster.residual_correlation, on the panel's own history (10 000 x 730) for the same group counts.

Panel: tools/bench_rollup.py's (tools/bench_components.py's cfg2: 10 000 series, linear / additive, 90 daily steps on
one shared future grid), models fitted once and the fitted history formed once outside the timed region.  Every route is
warmed up once, then timed --reps times; the host entry points copy their inputs over, copy back and synchronise the
device before they return, and a roll-up's create, set_noise_corr and free are outside its timed call.  The expectation
to check: the correlated add repeats the noise part of interval_sample_kernel once per element plus once per cell, so
its extra time per add should stay below that kernel's own (10.3 ms in DESIGN.md 5f's table).  Prints one JSON line per
route.  Kernel times come from a separate profiler run over this tool.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import panels, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--groups', default='1,100,10000', help='comma-separated group counts (each at most --series)')
    ap.add_argument('--rho', type=float, default=0.3)
    a = ap.parse_args()
    (name, spec, r, fut, kw), = panels(a.series, 'cfg2')
    H, N = fut.shape[-1], a.series
    keys = np.arange(N, dtype=np.int64)
    base = dict(panel=name, series=N, H=H, samples=a.samples)
    groups = [min(int(g), N) for g in a.groups.split(',')]
    for G in groups:
        group = keys % G
        best = {}
        for route, corr in (('add', None), ('add with noise_corr', np.full(G, a.rho))):
            wall = []
            for rep in range(a.reps + 1):                    # (the first repetition is the warm-up)
                with fc.Rollup(fut, G, uncertainty_samples=a.samples, seed=0, noise_corr=corr) as roll:
                    t0 = time.perf_counter()
                    roll.add(spec, r.theta, r.y_scale, r.grid, group, keys, **kw)
                    t1 = time.perf_counter()
                if rep:
                    wall.append(t1 - t0)
            best[route] = 1e3 * min(wall)
            print(json.dumps(dict(base, route='rollup G=%d: %s' % (G, route), groups=G, call_s=wall, best_ms=best[route])),
                  flush=True)
        print(json.dumps(dict(base, route='rollup G=%d: extra per add' % G, groups=G,
                              extra_ms=best['add with noise_corr'] - best['add'])), flush=True)
    ds, y = synth.make_panel(N, 730, 'linear', seed=751)                # the panel `panels` fitted
    fitted = fc.fitted_history(spec, r, ds, floor=kw.get('floor'))
    for G in groups:
        group = keys % G
        wall = timed(lambda: fc.residual_correlation(y, fitted, group, G), a.reps)
        print(json.dumps(dict(panel=name, series=N, T=y.shape[1], route='residual_correlation G=%d' % G, groups=G,
                              call_s=wall, best_ms=1e3 * min(wall))), flush=True)


if __name__ == '__main__':
    main()
