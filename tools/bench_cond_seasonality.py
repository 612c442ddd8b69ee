"""Times what a conditional seasonality costs (ModelSpec seasonalities with condition_name; include/tsf.h "conditional
seasonalities") on BASELINE cfg2's panel -- 10 000 series x 730 daily rows, linear growth, additive yearly (order 10) +
weekly (order 3):

  * fit_aligned with the weekly seasonality split into an in-season and an off-season conditional pair (June-August
    against the rest, a date rule of the spec), `extra` from conditional_extra, against the plain spec in the same run.
    The pair's 12 columns are dense explicit columns: the fit leaves the lattice tables and the in-register harmonic
    expansion, as a model with holidays does -- this is the figure that says what that costs;
  * conditional_extra alone on the same series as one ragged call: 7.3 M rows, 12 columns, host arrays in and out
    (upload of ds and the masks, one launch, download of 700 MB of columns).

Prints one JSON line per leg, wall seconds of every repetition after a warm-up; report the best of --reps (default 5)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402

YEARLY = {'name': 'yearly', 'period': 365.25, 'fourier_order': 10}
WEEKLY = {'name': 'weekly', 'period': 7, 'fourier_order': 3}
RULES = {'in_season': {'months': [6, 7, 8]}, 'off_season': {'months': [6, 7, 8], 'negate': True}}
PAIR = [dict(WEEKLY, name='weekly_in', condition_name='in_season'), dict(WEEKLY, name='weekly_off', condition_name='off_season')]


def timed(fn, reps):
    fn()                                    # warm-up (workspace, pool)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
    return wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--rows', type=int, default=730)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    N, T = a.series, a.rows
    ds, y = synth.make_panel(N, T, 'linear', seed=751)
    plain = fc.ModelSpec(growth='linear', seasonalities=[dict(YEARLY), dict(WEEKLY)])
    pair = fc.ModelSpec(growth='linear', seasonalities=[dict(YEARLY)] + PAIR, conditions=RULES)
    wall, ex = timed(lambda: fc.conditional_extra(pair, ds), a.reps)
    print(json.dumps({'leg': 'conditional_extra, one calendar', 'rows': T, 'columns': int(ex.shape[0]), 'call_s': wall,
                      'best_s': min(wall)}), flush=True)
    wall, rp = timed(lambda: fc.fit_aligned(plain, ds, y), a.reps)
    print(json.dumps({'leg': 'fit_aligned, plain weekly', 'series': N, 'rows': T, 'K': plain.K, 'call_s': wall,
                      'best_s': min(wall), 'fits_per_s': N / min(wall), 'mean_iter': float(rp.n_iter.mean())}), flush=True)
    wall, rc = timed(lambda: fc.fit_aligned(pair, ds, y, extra=ex), a.reps)
    print(json.dumps({'leg': 'fit_aligned, in / off-season weekly pair', 'series': N, 'rows': T, 'K': pair.K, 'call_s': wall,
                      'best_s': min(wall), 'fits_per_s': N / min(wall), 'mean_iter': float(rc.n_iter.mean()),
                      'ok': bool((rc.status > 0).all())}), flush=True)
    ds_r = np.tile(ds, N)
    off = np.arange(N + 1, dtype=np.int64) * T
    wall, exr = timed(lambda: fc.conditional_extra(pair, ds_r, offsets=off), a.reps)
    print(json.dumps({'leg': 'conditional_extra, ragged', 'series': N, 'rows': int(ds_r.size), 'columns': int(exr.shape[0]),
                      'call_s': wall, 'best_s': min(wall), 'rows_per_s': ds_r.size / min(wall),
                      'same_as_one_calendar': bool(np.array_equal(exr[:, :T], ex) and np.array_equal(exr[:, -T:], ex))}),
          flush=True)


if __name__ == '__main__':
    main()
