"""Times scoring observed values (forecaster.score_actuals -> tsf_score_actuals) against the per-series quantiles whose
draw and sort it shares: fc.predict_quantiles with 3 levels is the yardstick (one draw and one sort per (series, row);
this change leaves its code path as it was), then score_actuals with the same 3 levels and every output wanted (the
same draw and sort, plus per row two binary searches, the CRPS terms and their tree reduction in LDS, and four more
[N][H]-sized stores), then score_actuals with the per-series aggregates alone, all in the same run.

Panel: tools/bench_components.py's cfg2 (10 000 series, linear / additive, 90 daily steps on one shared future grid),
models fitted once outside the timed region; y_obs is the point forecast plus noise of the model's own scale, one row in
twenty not observed.  Every route is warmed up once, then timed --reps times (the host entry points copy back and
synchronise the device before they return).  Prints one JSON line per route and one with the ratio.  Kernel times come
from a separate profiler run over this tool (rocprofv3 --kernel-trace --stats).  Not part of bench.py."""
import argparse
import json
import os
import sys

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
    a = ap.parse_args()
    (name, spec, r, fut, kw), = panels(a.series, 'cfg2')
    H, N = fut.shape[-1], a.series
    keys = np.arange(N, dtype=np.int64)
    args = (spec, r.theta, r.y_scale, r.grid, fut)
    rng = np.random.default_rng(0)
    yhat = fc.predict(*args, **kw)
    y_obs = yhat + rng.normal(size=yhat.shape) * (np.exp(r.theta[:, 2]) * r.y_scale)[:, None]
    y_obs[rng.uniform(size=y_obs.shape) < 0.05] = np.nan
    base = dict(panel=name, series=N, H=H, samples=a.samples)
    draw = dict(series_key=keys, uncertainty_samples=a.samples, seed=0, **kw)
    agg = ('n_obs', 'mean_crps', 'mean_pinball', 'coverage')
    routes = [('predict_quantiles 3 levels', lambda: fc.predict_quantiles(*args, LEVELS, **draw)),
              ('score_actuals 3 levels, all outputs', lambda: fc.score_actuals(*args, y_obs, LEVELS, **draw)),
              ('score_actuals 3 levels, aggregates only',
               lambda: fc._score_actuals_call(*args, y_obs, kw.get('floor'), kw.get('cap'), None, keys, a.samples, 0, LEVELS,
                                              agg, None))]
    best = {}
    for route, fn in routes:
        wall = timed(fn, a.reps)
        best[route] = min(wall)
        print(json.dumps(dict(base, route=route, call_s=wall, best_ms=1e3 * min(wall))), flush=True)
    print(json.dumps(dict(base, route='ratio score_actuals (all outputs) / predict_quantiles',
                          ratio=best[routes[1][0]] / best[routes[0][0]])), flush=True)


if __name__ == '__main__':
    main()
