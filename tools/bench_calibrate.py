"""Times conformal calibration in one call (forecaster.calibrate -> tsf_calibrate) against cross-validation alone and
against the same work by hand, all in the same run, and reports what calibration does to interval coverage.

Panel: the cfg2 cross-validation panel (10 000 series x 730 daily rows, linear / additive, yearly order 10 + weekly
order 3; horizon 90 d, fbprophet's default period / initial: 9 cutoffs), B = 10 horizon buckets, levels 0.8 and 0.95,
|y - yhat| scores.  Routes:
  cross_validate                  the folds, their forecasts and metrics: what a validator run pays already
  by hand                         cross_validate, then the rule in numpy on its holdout rows (vectorised over the
                                  aligned panel: one sort per series for the pooled row, one per bucket) -- the fold
                                  fits and the forecasts come back to the host first
  calibrate                       one call: only the table comes back
Every route is warmed up once, then timed --reps times.  The by-hand table is checked against the library's before
anything is timed.

Coverage: the first 640 rows of every series are fitted, the next 90 days forecast with the model's own 0.8 interval
(1000 samples), and the share of the 90 x N held-back rows inside the model's interval and inside the calibrated 0.8
interval (the table of those 640 rows' cross-validation; --coverage-initial-days sets its `initial`) is printed, pooled
over the panel.
Prints one JSON line per route, one with the ratios, one with the coverages.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import timed  # noqa: E402

DAY = synth.DAY_NS
CV = dict(period=None, initial=None)       # fbprophet's defaults: horizon / 2, 3 * horizon
LEVELS, B, MIN_SCORES = [0.8, 0.95], 10, 20


def rule_numpy(cv, N, horizon):
    """include/tsf.h's ABS rule on an aligned panel's CVResult (every series has the same holdout horizons), vectorised
    over the series -> q [N][B+1][L]"""
    R = len(cv.y) // N
    h = (cv.ds - cv.cutoff[cv.row_fold])[:R]
    s = np.abs(cv.y - cv.yhat).reshape(N, R)
    w = (horizon + B - 1) // B
    bucket = np.minimum(B - 1, (h - 1) // w)
    q = np.full((N, B + 1, len(LEVELS)), np.nan)
    for b in range(B + 1):
        a = np.sort(s[:, bucket == b] if b < B else s, axis=1)
        m = a.shape[1]
        if m < MIN_SCORES:
            continue
        for l, p in enumerate(LEVELS):
            k = int(np.ceil(np.float64(m + 1) * np.float64(p)))
            q[:, b, l] = a[:, min(k, m) - 1]
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--coverage-initial-days', type=int, default=None,
                    help="the coverage leg's cross-validation `initial` in days (default: fbprophet's 3 * horizon)")
    a = ap.parse_args()
    N, T, horizon = a.series, 730, 90 * DAY
    ds, y = synth.make_panel(N, T, 'linear', seed=751)
    seas = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
    spec = fc.ModelSpec(growth='linear', seasonalities=seas)
    kw = dict(n_buckets=B, min_scores=MIN_SCORES)

    def by_hand():
        cv = fc.cross_validate(spec, ds, y, horizon, **CV)
        return cv, rule_numpy(cv, N, horizon)
    cal = fc.calibrate(spec, ds, y, horizon, LEVELS, **kw, **CV)
    cv, q = by_hand()
    # (a series with a failed fold has no table in the library; the vectorised rule does not model that)
    ok = (np.asarray(cv.status) == 0) & np.isfinite(cv.yhat.reshape(N, -1)).all(axis=1)
    assert np.array_equal(cal.q[ok], q[ok]), 'the by-hand rule disagrees with the library'
    base = dict(panel='cfg2 cv', series=N, T=T, folds=int(len(cv.cutoff) // N), holdout_rows=int(len(cv.y)), buckets=B,
                levels=LEVELS, series_checked_against_numpy=int(ok.sum()))
    routes = [('cross_validate', lambda: fc.cross_validate(spec, ds, y, horizon, **CV)),
              ('by hand: cross_validate, numpy rule', by_hand),
              ('calibrate', lambda: fc.calibrate(spec, ds, y, horizon, LEVELS, **kw, **CV))]
    best = {}
    for route, fn in routes:
        wall = timed(fn, a.reps)
        best[route] = min(wall)
        print(json.dumps(dict(base, route=route, call_s=wall, best_ms=1e3 * min(wall))), flush=True)
    print(json.dumps(dict(base, route='ratios', calibrate_over_by_hand=best[routes[2][0]] / best[routes[1][0]],
                          calibrate_over_cross_validate=best[routes[2][0]] / best[routes[0][0]],
                          calibrate_minus_cross_validate_ms=1e3 * (best[routes[2][0]] - best[routes[0][0]]))), flush=True)
    # coverage on rows no fit has seen
    Tf = 640
    fit = fc.fit_aligned(spec, ds[:Tf], y[:, :Tf])
    fut, held = ds[Tf:Tf + 90], y[:, Tf:Tf + 90]
    _, lo, hi = fc.predict_intervals(spec, fit.theta, fit.y_scale, fit.grid, fut, uncertainty_samples=1000, interval_width=0.8)
    cv_kw = dict(CV, initial=None if a.coverage_initial_days is None else a.coverage_initial_days * DAY)
    cal = fc.calibrate(spec, ds[:Tf], y[:, :Tf], horizon, [0.8], **kw, **cv_kw)
    _, clo, chi = fc.predict_calibrated(spec, fit.theta, fit.y_scale, fit.grid, fut, cal)
    good = (fit.status >= 0) & (cal.status == 0)
    inside = lambda a_, b_: float(np.mean((held[good] >= a_[good]) & (held[good] <= b_[good])))     # noqa: E731
    print(json.dumps(dict(route='coverage', target=0.8, series=int(good.sum()), fitted_rows=Tf, held_back_rows=90,
                          initial_days=a.coverage_initial_days, scores_per_series=int(cal.n[good, B, 0].min()),
                          model_interval=inside(lo, hi), calibrated=inside(clo[:, 0], chi[:, 0]),
                          mean_width_model=float(np.mean((hi - lo)[good])),
                          mean_width_calibrated=float(np.mean((chi[:, 0] - clo[:, 0])[good])))), flush=True)


if __name__ == '__main__':
    main()
