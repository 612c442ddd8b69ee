"""Times the forecast quantiles (forecaster.predict_quantiles / predictive_samples -> tsf_predict_quantiles) against the
forecasts they extend: fc.predict (the point forecast) and fc.predict_intervals (one symmetric pair from the same draws;
untouched by the quantile entry, so it is the yardstick: 3 levels draw once and sort once per row, as it does).

Panels: tools/bench_components.py's two (cfg2: 10 000 series, linear / additive, 90 daily steps on one shared future
grid; ref: the reference's model on the fixture's calendars, 96 steps of 15 min per series), models fitted once outside
the timed region.  Every route is warmed up once, then timed --reps times (the host entry points copy back and
synchronise the device before they return).  The raw draws are [N][H][samples] float64 per array on the host (7.2 GB for
cfg2 at 10 000 series), so that route runs on the first --sample-series series only.  Prints one JSON line per (panel,
route).  Kernel times come from a separate profiler run over this tool (rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc  # noqa: E402
from tools.bench_components import panels, timed  # noqa: E402

LEVELS = [0.1, 0.5, 0.9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--sample-series', type=int, default=1000)
    ap.add_argument('--only', choices=['cfg2', 'ref'])
    ap.add_argument('--routes', help='comma-separated substrings of the route names to run (default: all)')
    a = ap.parse_args()
    for name, spec, r, fut, kw in panels(a.series, a.only):
        H = fut.shape[-1]
        args = (spec, r.theta, r.y_scale, r.grid, fut)
        dr = dict(uncertainty_samples=a.samples, seed=0)
        m = min(a.sample_series, a.series)
        sub = (spec, r.theta[:m], r.y_scale[:m], r.grid if len(r.grid) == 1 else r.grid[:m],
               fut if fut.ndim == 1 else fut[:m])
        skw = {k: v[:m] for k, v in kw.items()}
        routes = [('predict', a.series, lambda: fc.predict(*args, **kw)),
                  ('predict_intervals', a.series, lambda: fc.predict_intervals(*args, **kw, interval_width=0.8, **dr)),
                  ('predict_quantiles 3 levels', a.series, lambda: fc.predict_quantiles(*args, LEVELS, **kw, **dr)),
                  ('predict_quantiles 3 levels + cumulative', a.series,
                   lambda: fc.predict_quantiles(*args, LEVELS, cumulative=True, **kw, **dr)),
                  ('predict_quantiles 3 levels + cumulative + trend', a.series,
                   lambda: fc.predict_quantiles(*args, LEVELS, cumulative=True, trend=True, **kw, **dr)),
                  ('predict_quantiles 9 levels', a.series,
                   lambda: fc.predict_quantiles(*args, [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99], **kw, **dr)),
                  ('predictive_samples', m, lambda: fc.predictive_samples(*sub, **skw, **dr))]
        for route, n, fn in routes:
            if a.routes and not any(s in route for s in a.routes.split(',')):
                continue
            wall = timed(fn, a.reps)
            print(json.dumps({'panel': name, 'route': route, 'series': n, 'H': H, 'samples': 0 if route == 'predict' else a.samples,
                              'call_s': wall, 'best_ms': 1e3 * min(wall)}), flush=True)


if __name__ == '__main__':
    main()
