"""Times outlier screening in one call (forecaster.fit_screened -> tsf_fit_screened) against the same work by hand and
against the plain fit, all in the same run.

Panel: the cfg2 panel (10 000 series x 730 daily rows, linear / additive, yearly order 10 + weekly order 3) with three
spikes of 20 x the series' range in 5 % of the series (every 20th).  Routes:
  fit_aligned                     the plain fit: what a job without screening pays
  by hand                         fit_aligned, predict on the history, the rule and the cut in numpy (vectorised over
                                  the panel: a partition for the medians, one more for the budget's order statistic),
                                  fit_ragged on the flagged series -- the panel crosses to the device twice, the
                                  fitted values come back once
  fit_screened                    one call, passes = 1
Every route is warmed up once, then timed --reps times (the host entry points copy back and synchronise the device
before they return).  The by-hand route is checked against fit_screened (same flags, same refits) before anything is
timed.  Prints one JSON line per route and one with the ratios.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import forecaster as fc, synth  # noqa: E402
from tools.bench_components import timed  # noqa: E402

SCREEN = dict(threshold=5.0, max_share=0.05, min_rows=10)


def rule_numpy(y, fitted, y_scale, threshold, max_share, scale_floor=1e-8):
    """include/tsf.h's rule on an aligned panel without earlier exclusions, vectorised (the values of the median and
    of the order statistics do not depend on how they are found) -> flag [N][T] bool"""
    N, T = y.shape
    r = y - fitted
    lo, hi = (T - 1) // 2, T // 2
    a = np.partition(r, (lo, hi), axis=1)
    center = 0.5 * (a[:, lo] + a[:, hi])
    d = np.abs(r - center[:, None])
    B = int(np.floor(max_share * T))
    b = np.partition(d, (lo, hi, T - 1 - B), axis=1)
    scale = np.fmax(1.4826 * (0.5 * (b[:, lo] + b[:, hi])), scale_floor * y_scale)
    if B <= 0:
        return np.zeros(y.shape, bool)
    cut = np.fmax(threshold * scale, b[:, T - 1 - B])
    return d > cut[:, None]


def by_hand(spec, ds, y):
    first = fc.fit_aligned(spec, ds, y)
    fitted = fc.predict(spec, first.theta, first.y_scale, first.grid, ds)
    flag = rule_numpy(y, fitted, first.y_scale, SCREEN['threshold'], SCREEN['max_share'])
    sel = np.flatnonzero(flag.any(axis=1))
    if len(sel) == 0:
        return first, flag, sel, None
    keep = ~flag[sel]
    off = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    refit = fc.fit_ragged(spec, off, np.broadcast_to(ds, keep.shape)[keep], y[sel][keep])
    return first, flag, sel, refit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    N, T = a.series, 730
    ds, y = synth.make_panel(N, T, 'linear', seed=751)
    rs = np.random.RandomState(5)
    spiked = np.arange(0, N, 20)
    for n in spiked:
        y[n, rs.choice(T, 3, replace=False)] += 20.0 * (y[n].max() - y[n].min())
    seas = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
    spec = fc.ModelSpec(growth='linear', seasonalities=seas)
    # the two routes compute the same thing
    sf = fc.fit_screened(spec, ds, y, **SCREEN)
    first, flag, sel, refit = by_hand(spec, ds, y)
    assert np.array_equal(sf.screen.flag.astype(bool), flag), 'the by-hand rule disagrees with the library'
    assert np.array_equal(sf.fit.theta[sel], refit.theta) and np.array_equal(np.delete(sf.fit.theta, sel, 0), np.delete(first.theta, sel, 0))
    base = dict(panel='cfg2 + spikes', series=N, T=T, spiked=int(len(spiked)), flagged_series=int(len(sel)),
                flagged_rows=int(flag.sum()))
    routes = [('fit_aligned', lambda: fc.fit_aligned(spec, ds, y)),
              ('by hand: fit_aligned, predict, numpy rule and cut, fit_ragged', lambda: by_hand(spec, ds, y)),
              ('fit_screened', lambda: fc.fit_screened(spec, ds, y, **SCREEN))]
    best = {}
    for route, fn in routes:
        wall = timed(fn, a.reps)
        best[route] = min(wall)
        print(json.dumps(dict(base, route=route, call_s=wall, best_ms=1e3 * min(wall))), flush=True)
    print(json.dumps(dict(base, route='ratios', fit_screened_over_by_hand=best[routes[2][0]] / best[routes[1][0]],
                          fit_screened_over_fit_aligned=best[routes[2][0]] / best[routes[0][0]])), flush=True)


if __name__ == '__main__':
    main()
