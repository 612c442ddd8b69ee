"""Times forecaster.fit_noise_state (include/tsf.h tsf_noise_state: the AR(1) noise state of a fitted panel in one
launch) beside the route it replaces and beside the fit it follows, in the same run:

  aligned   BASELINE cfg2's panel (10 000 series x 730 daily rows, linear growth, additive yearly + weekly), fitted once
            outside the timed region: fit_noise_state, fit_residual_autocorrelation (fitted_history to the host, then
            both estimator kernels on a second copy of the panel), fit_aligned alone
  ragged    the same series, each keeping a random 90 % of its rows: the same three with offsets (fit_ragged)
  modeler   jobs.prophet_modeler.model_arrays on the cfg2 panel's columns with and without model.noise

Every route is warmed up once, then timed --reps times; the host entries copy their inputs over, copy back and
synchronise the device before they return; the best call counts.  The one condition: fit_noise_state is not slower than
fit_residual_autocorrelation in the same run (that is why the kernel exists); the last line says whether it held.
Prints one JSON line per route.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from time_series_spark_amd.jobs import prophet_modeler as pm  # noqa: E402
from tools.bench_components import timed  # noqa: E402

SEAS = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--rows', type=int, default=730)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    N, T = a.series, a.rows
    ds, y = synth.make_panel(N, T, 'linear', seed=751)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    rng = np.random.default_rng(751)
    keep = rng.random((N, T)) < 0.9
    keep[:, [0, -1]] = True
    lens = keep.sum(axis=1)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ds_r, y_r = np.broadcast_to(ds, (N, T))[keep], y[keep]
    best = {}

    def report(panel, route, fn, **more):
        wall = timed(fn, a.reps)
        best[(panel, route)] = 1e3 * min(wall)
        print(json.dumps(dict(panel=panel, series=N, rows=int(T if panel != 'ragged' else off[-1]), route=route,
                              call_s=wall, best_ms=1e3 * min(wall), worst_ms=1e3 * max(wall), **more)), flush=True)

    r = fc.fit_aligned(spec, ds, y)
    one, hand = fc.fit_noise_state(spec, r, ds, y), fc.fit_residual_autocorrelation(spec, r, ds, y)
    same = all(np.array_equal(getattr(one, f).view(np.int64 if getattr(one, f).itemsize == 8 else np.int32),
                              getattr(hand, f).view(np.int64 if getattr(hand, f).itemsize == 8 else np.int32))
               for f in ('phi', 'phi_raw', 'n_pairs', 'scale', 'status', 'last_resid', 'last_gap', 'last_ds_ns'))
    report('aligned', 'fit_noise_state', lambda: fc.fit_noise_state(spec, r, ds, y), same_bits_as_by_hand=bool(same))
    report('aligned', 'fit_residual_autocorrelation', lambda: fc.fit_residual_autocorrelation(spec, r, ds, y))
    report('aligned', 'fit_aligned', lambda: fc.fit_aligned(spec, ds, y))
    rr = fc.fit_ragged(spec, off, ds_r, y_r)
    report('ragged', 'fit_noise_state', lambda: fc.fit_noise_state(spec, rr, ds_r, y_r, offsets=off))
    report('ragged', 'fit_residual_autocorrelation', lambda: fc.fit_residual_autocorrelation(spec, rr, ds_r, y_r, offsets=off))
    report('ragged', 'fit_ragged', lambda: fc.fit_ragged(spec, off, ds_r, y_r))
    # the modeler on the same panel as columns (series_id, dim_id, ds, y), with and without model.noise
    sid, did = np.repeat(np.arange(N, dtype=np.int64), T), np.zeros(N * T, np.int64)
    cols = (sid, did, np.tile(ds, N), np.ascontiguousarray(y, dtype=np.float64).reshape(-1))
    model = {'floor': 0, 'cap_multiplier': 1.1,
             'prophet': {'growth': 'linear', 'seasonality_mode': 'additive', 'daily_seasonality': False}}
    report('modeler', 'model_arrays', lambda: pm.model_arrays({'io': {}, 'model': model}, batch=True)(*cols))
    report('modeler', 'model_arrays with model.noise',
           lambda: pm.model_arrays({'io': {}, 'model': dict(model, noise={})}, batch=True)(*cols))
    held = all(best[(p, 'fit_noise_state')] <= best[(p, 'fit_residual_autocorrelation')] for p in ('aligned', 'ragged'))
    print(json.dumps(dict(condition='fit_noise_state is not slower than fit_residual_autocorrelation', held=bool(held),
                          aligned_speedup=best[('aligned', 'fit_residual_autocorrelation')] / best[('aligned', 'fit_noise_state')],
                          ragged_speedup=best[('ragged', 'fit_residual_autocorrelation')] / best[('ragged', 'fit_noise_state')],
                          modeler_extra_ms=best[('modeler', 'model_arrays with model.noise')] - best[('modeler', 'model_arrays')])),
          flush=True)


if __name__ == '__main__':
    main()
