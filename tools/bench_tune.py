"""Times prior-scale tuning (forecaster.tune -> tsf_tune) against the same work done by hand: one
cross_validate(rolling_window=1) per candidate, a host argmin, and one fit_aligned per distinct choice.

Panel: BASELINE cfg2's model and shape -- 10 000 series x 730 daily rows, linear growth, additive yearly + weekly,
horizon 90 d, fbprophet's default period / initial (9 cutoffs) -- and a 4 x 4 grid over changepoint_prior_scale x
seasonality_prior_scale: 16 x 90 000 = 1.44 M fold fits plus the refit.  Prints one JSON line per route (best of
--reps calls after a warm-up); the by-hand route's choice and scores are checked against tune's.

--leg tune | cv | cv2x runs once for a profiler (rocprofv3 --kernel-trace --stats -- python tools/bench_tune.py
--leg ...): the tune call; one cross_validate per candidate, in candidate order; the same on the panel stacked twice
(twice the folds in each launch, the same fits).  --summarize <kernel_trace.csv> [...] sums such a trace per kernel
and lists the fit kernel's launches in order.  The straggler tail of candidate c's fit launch is what one launch over
twice its folds saves against two launches: 2 t_c(cv) - t_c(cv2x) of the fit kernel."""
import argparse
import csv
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402

DAY = fc.DAY_NS
SEAS = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
GRID = {'changepoint_prior_scale': [0.001, 0.01, 0.1, 0.5], 'seasonality_prior_scale': [0.01, 0.1, 1.0, 10.0]}


def by_hand(spec, ds, y, cands):
    """C cross_validate calls, the host argmin (first minimum of the finite scores), a fit_aligned per choice."""
    N, C = len(y), len(cands)
    score = np.full((N, C), np.nan)
    status = None
    for c, sp in enumerate(cands):
        cv = fc.cross_validate(sp, ds, y, 90 * DAY, rolling_window=1.0)
        mo = cv.metric_offsets
        has = np.diff(mo) == 1
        score[has, c] = cv.rmse[mo[:-1][has]]
        status = cv.status
    fin = np.isfinite(score)
    best = np.where(fin.any(axis=1) & (status == 0), np.argmin(np.where(fin, score, np.inf), axis=1), -1)
    fits = {}
    for b in np.unique(best):
        sel = np.flatnonzero(best == b)
        fits[int(b)] = fc.fit_aligned(cands[b] if b >= 0 else spec, ds, y[sel])
    return score, best, fits


def summarize(paths):
    tot = defaultdict(lambda: [0, 0.0])
    fits = []
    for p in paths:
        with open(p) as fh:
            for row in csv.DictReader(fh):
                name = row['Kernel_Name'].split('(')[0].split('<')[0].replace('void ', '').strip()
                t = tot[name]
                t[0] += 1
                ms = (int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-6
                t[1] += ms
                if name.startswith('tsf::fit_'):
                    fits.append((int(row['Start_Timestamp']), name, ms))
    all_ms = sum(v[1] for v in tot.values())
    for name, (n, ms) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        print(json.dumps({'kernel': name, 'launches': n, 'ms': round(ms, 3), 'share': round(ms / all_ms, 4)}))
    print(json.dumps({'kernel': 'ALL', 'ms': round(all_ms, 3)}))
    print(json.dumps({'fit_launches_ms': [round(ms, 1) for _, _, ms in sorted(fits)]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--leg', choices=['tune', 'cv', 'cv2x'])
    ap.add_argument('--no-by-hand', action='store_true')
    ap.add_argument('--summarize', nargs='+')
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    ds, y = synth.make_panel(a.series, 730, 'linear', seed=751)
    spec = fc.ModelSpec(growth='linear', seasonalities=SEAS)
    cands, _ = fc.tune_candidates(spec, GRID)
    if a.leg:
        t0 = time.perf_counter()
        if a.leg == 'tune':
            fc.tune(spec, ds, y, 90 * DAY, grid=GRID)
        else:
            yy = y if a.leg == 'cv' else np.concatenate([y, y])
            for sp in cands:
                fc.cross_validate(sp, ds, yy, 90 * DAY, rolling_window=1.0)
        print(json.dumps({'leg': a.leg, 'series': a.series, 'call_s': time.perf_counter() - t0}), flush=True)
        return
    fc.tune(spec, ds, y, 90 * DAY, grid=GRID)            # warm-up (workspace, pool)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = fc.tune(spec, ds, y, 90 * DAY, grid=GRID)
        wall.append(time.perf_counter() - t0)
    F = int(fc.cv_plan(ds, 90 * DAY, N=a.series)['n_folds'].sum())
    C = len(cands)
    print(json.dumps({'route': 'tune', 'series': a.series, 'candidates': C, 'folds': F, 'call_s': wall,
                      'fold_fits_per_s': F * C / min(wall), 'counts': fc.last_tune_counts(),
                      'choices': int(len(np.unique(r.best)))}), flush=True)
    if a.no_by_hand:
        return
    by_hand(spec, ds, y, cands)
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        score, best, fits = by_hand(spec, ds, y, cands)
        wall.append(time.perf_counter() - t0)
    same = bool(np.array_equal(best, r.best) and np.array_equal(score.view(np.int64), r.score.view(np.int64)) and
                all(np.array_equal(f.theta, r.fit.theta[best == b]) for b, f in fits.items()))
    print(json.dumps({'route': 'by hand (cross_validate per candidate + argmin + fit_aligned per choice)',
                      'series': a.series, 'candidates': C, 'folds': F, 'call_s': wall,
                      'fold_fits_per_s': F * C / min(wall), 'same_as_tune': same}), flush=True)


if __name__ == '__main__':
    main()
