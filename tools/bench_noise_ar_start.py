"""Times the conditioned start of the AR(1) noise chain (include/tsf.h "the conditioned start") beside the stationary
chain, in the same run: forecaster.predict_quantiles (3 levels, cumulative) and forecaster.predict_windows (the
calendar weeks of the horizon, 14 on cfg2's 90 days) with noise_ar = phi (the stationary chain) and with a conditioned
object (phi = --phi for every series, the last residual at one residual deviation, steps = 1: no series takes the
phi = 0 select), then forecaster.residual_last beside forecaster.residual_autocorrelation on the panel's own history
(10 000 x 730; residual_autocorrelation includes one residual_last since it fills last_resid and last_gap).

Panel: tools/bench_components.py's cfg2 (10 000 series, linear / additive, 90 daily steps on one shared future grid),
models fitted once and the fitted history formed once outside the timed region.  Every route is warmed up once, then
timed --reps times; the host entry points copy their inputs over, copy back and synchronise the device before they
return.  The expectation to check: the conditioned start adds one small launch per chunk (one thread per series, two
adds per row) and one product per thread at row 0 of the sample kernel, so the difference should lie within the
stationary route's own best-to-worst spread.  Prints one JSON line per route.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import panels, timed  # noqa: E402

LEVELS = [0.1, 0.5, 0.9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--phi', type=float, default=0.6)
    a = ap.parse_args()
    (name, spec, r, fut, kw), = panels(a.series, 'cfg2')
    H, N = fut.shape[-1], a.series
    args = (spec, r.theta, r.y_scale, r.grid, fut)
    dr = dict(uncertainty_samples=a.samples, seed=0)
    ds, y = synth.make_panel(N, 730, 'linear', seed=751)                # the panel `panels` fitted
    fitted = fc.fitted_history(spec, r, ds, floor=kw.get('floor'))
    est = fc.residual_autocorrelation(y, fitted)
    phi = np.full(N, a.phi)
    cond = fc.NoiseARStart(phi, np.where(np.isfinite(est.scale), est.scale, 0.0), est.last_gap.astype(np.int64) + 1)
    weeks = fc.period_windows(fut, 'W')
    base = dict(panel=name, series=N, H=H, samples=a.samples)
    for what, fn in (('predict_quantiles 3 levels + cumulative',
                      lambda ar: fc.predict_quantiles(*args, LEVELS, cumulative=True, noise_ar=ar, **kw, **dr)),
                     ('predict_windows %d weeks, 3 levels' % len(weeks),
                      lambda ar: fc.predict_windows(*args, weeks, LEVELS, noise_ar=ar, **kw, **dr))):
        best = {}
        for route, ar in ((what + ' with the stationary chain', phi), (what + ' with the conditioned start', cond)):
            wall = timed(lambda: fn(ar), a.reps)
            best[route] = 1e3 * min(wall)
            print(json.dumps(dict(base, route=route, call_s=wall, best_ms=best[route], worst_ms=1e3 * max(wall))), flush=True)
        print(json.dumps(dict(base, route=what + ': extra with the conditioned start',
                              extra_ms=best[what + ' with the conditioned start'] - best[what + ' with the stationary chain'])),
              flush=True)
    for route, fn in (('residual_last', lambda: fc.residual_last(y, fitted)),
                      ('residual_autocorrelation', lambda: fc.residual_autocorrelation(y, fitted))):
        wall = timed(fn, a.reps)
        print(json.dumps(dict(panel=name, series=N, T=y.shape[1], route=route, call_s=wall, best_ms=1e3 * min(wall),
                              worst_ms=1e3 * max(wall))), flush=True)


if __name__ == '__main__':
    main()
