"""Times model-structure selection in one call (forecaster.select_model -> tsf_select) against the same work done by
hand in the same run: one cross_validate(rolling_window=1) per candidate (each copying every fold's fit and forecast
back to the host), the choice rule in numpy, the panel cut by choice on the host, and one fit_aligned per group.

Panel: the cfg2 cross-validation panel -- 10 000 series x 730 daily rows, horizon 90 d, fbprophet's default period /
initial (9 cutoffs).  Candidates, simple to complex and back: linear / additive (yearly order 10 + weekly order 3);
linear / multiplicative; logistic / multiplicative with cap = 1.2 max y; linear / additive with yearly only and 5
changepoints.  Every route is warmed up once, then timed --reps times (best of the calls is reported); the by-hand
route's scores, choice and refit are checked against select_model's before anything is timed.  The per-candidate split:
a one-candidate select_model (no refit) per candidate, with its tsf_last_tune_counts.
Prints one JSON line per route, one per candidate, one with the ratio.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import timed  # noqa: E402

DAY = synth.DAY_NS
YEARLY = {'name': 'yearly', 'period': 365.25, 'fourier_order': 10}
WEEKLY = {'name': 'weekly', 'period': 7, 'fourier_order': 3}
NAMES = ['linear/additive', 'linear/multiplicative', 'logistic/multiplicative', 'linear/additive yearly, 5 changepoints']


def candidates():
    return [fc.ModelSpec(growth='linear', seasonalities=[YEARLY, WEEKLY]),
            fc.ModelSpec(growth='linear', seasonality_mode='multiplicative', seasonalities=[YEARLY, WEEKLY]),
            fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=[YEARLY, WEEKLY]),
            fc.ModelSpec(growth='linear', seasonalities=[YEARLY], n_changepoints=5)]


def rule_numpy(score, status, tolerance):
    """include/tsf.h's choice: the lowest candidate with a finite score <= m * (1 + tolerance), m the least finite one;
    -1 without a fold or a finite score"""
    fin = np.isfinite(score)
    m = np.where(fin, score, np.inf).min(axis=1)
    under = fin & (score <= (m * (1.0 + tolerance))[:, None])
    return np.where(under.any(axis=1) & (status == 0), under.argmax(axis=1), -1).astype(np.int32)


def by_hand(cands, ds, y, cap, horizon, tolerance, fallback):
    N, C = len(y), len(cands)
    score = np.full((N, C), np.nan)
    plan_ok = None
    for c, sp in enumerate(cands):
        cv = fc.cross_validate(sp, ds, y, horizon, cap=cap, rolling_window=1.0)
        mo = cv.metric_offsets
        has = np.diff(mo) == 1
        score[has, c] = cv.rmse[mo[:-1][has]]
        plan_ok = np.where(np.asarray(cv.n_folds) > 0, 0, -1)
    best = rule_numpy(score, plan_ok, tolerance)
    chosen = np.where(best >= 0, best, fallback)
    fits = {}
    for c in np.unique(chosen):
        sel = np.flatnonzero(chosen == c)
        fits[int(c)] = (sel, fc.fit_aligned(cands[c], ds, y[sel], cap=cap[sel]))
    return score, best, fits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--tolerance', type=float, default=0.02)
    a = ap.parse_args()
    N, T, horizon = a.series, 730, 90 * DAY
    ds, y = synth.make_panel(N, T, 'linear', seed=751)
    cap = 1.2 * y.max(axis=1)
    cands = candidates()
    kw = dict(cap=cap, tolerance=a.tolerance, fallback=0)

    r = fc.select_model(cands, ds, y, horizon, **kw)
    counts = fc.last_tune_counts()
    score, best, fits = by_hand(cands, ds, y, cap, horizon, a.tolerance, 0)
    same = bool(np.array_equal(score.view(np.int64), r.score.view(np.int64)) and np.array_equal(best, r.best) and
                all(np.array_equal(f.theta, r.fit.theta[sel, :cands[c].theta_stride]) for c, (sel, f) in fits.items()))
    assert same, 'the by-hand route disagrees with select_model'
    F = int(fc.cv_plan(ds, horizon, N=N)['n_folds'].sum())
    base = dict(panel='cfg2 cv', series=N, T=T, folds=F, candidates=len(cands), tolerance=a.tolerance)
    chosen = np.bincount(r.chosen, minlength=len(cands)).tolist()
    routes = [('select_model', lambda: fc.select_model(cands, ds, y, horizon, **kw)),
              ('by hand: cross_validate per candidate, numpy rule, host cut, fit_aligned per group',
               lambda: by_hand(cands, ds, y, cap, horizon, a.tolerance, 0))]
    best_s = {}
    for route, fn in routes:
        wall = timed(fn, a.reps)
        best_s[route] = min(wall)
        print(json.dumps(dict(base, route=route, call_s=wall, best_s=min(wall), fold_fits_per_s=F * len(cands) / min(wall),
                              **(dict(counts=counts, chosen=chosen, same_as_by_hand=same) if route == 'select_model' else {}))),
              flush=True)
    for c, sp in enumerate(cands):
        wall = timed(lambda: fc.select_model([sp], ds, y, horizon, cap=cap, refit=False), a.reps)
        print(json.dumps(dict(base, route='one candidate, no refit', candidate=c, name=NAMES[c], stride=sp.theta_stride,
                              call_s=wall, best_s=min(wall), counts=fc.last_tune_counts(), chosen_by=chosen[c])), flush=True)
    print(json.dumps(dict(base, route='ratio', select_over_by_hand=best_s[routes[0][0]] / best_s[routes[1][0]],
                          by_hand_minus_select_s=best_s[routes[1][0]] - best_s[routes[0][0]])), flush=True)


if __name__ == '__main__':
    main()
