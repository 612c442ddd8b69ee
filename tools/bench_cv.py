"""Times batched cross-validation (forecaster.cross_validate -> tsf_cross_validate) against the same folds done by
hand (C fit_ragged calls on prefix panels cut on the host, one per cutoff, and one predict per cutoff; metrics not
included in the by-hand time, which therefore flatters it).

Panels:
  cfg2  BASELINE cfg2's model and shape: 10 000 series x 730 daily rows, linear growth, additive yearly + weekly,
        horizon 90 d, fbprophet's default period / initial: 9 cutoffs, 90 000 fits (quadratic-form route)
  ref   the reference's model (logistic growth, multiplicative auto seasonalities, algorithm auto) on the fixture's
        shape: the two irregular timestamp vectors of tests/golden/fixture_751.npz (410 / 406 rows), each series on one
        of them, horizon 40 d, period 20 d, initial 300 d
Prints one JSON line per (panel, route).  --series N scales both panels; --only cfg2|ref.  The kernels' shares of the
call come from a profiler run over this tool (rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import _lib, forecaster as fc, synth  # noqa: E402

DAY = fc.DAY_NS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def panels(N, only):
    if only in (None, 'cfg2'):
        ds, y = synth.make_panel(N, 730, 'linear', seed=751)
        seas = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]
        yield ('cfg2', fc.ModelSpec(growth='linear', seasonalities=seas), dict(ds_ns=ds, y=y, horizon=90 * DAY), None)
    if only in (None, 'ref'):
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'fixture_751.npz'))
        o, d = g['offsets'], g['raw_ds_ns']
        cal = [d[o[0]:o[1]], d[o[1]:o[2]]]
        _, yy = synth.make_panel(N, len(cal[0]), 'logistic', seed=751)
        lens = np.array([len(cal[n % 2]) for n in range(N)])
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ds = np.concatenate([cal[n % 2] for n in range(N)])
        y = np.concatenate([yy[n][:lens[n]] for n in range(N)])
        cap = np.array([yy[n][:lens[n]].max() * 1.1 for n in range(N)])
        seas = fc.ModelSpec.auto_seasonalities(cal[0], seasonality_mode='multiplicative')
        spec = fc.ModelSpec(growth='logistic', seasonality_mode='multiplicative', seasonalities=seas,
                            algorithm=_lib.ALGO_AUTO)
        yield ('ref', spec, dict(ds_ns=ds, y=y, horizon=40 * DAY, period=20 * DAY, initial=300 * DAY, offsets=off,
                                 floor=np.zeros(N), cap=cap), off)


def by_hand(spec, kw, off):
    """C fit_ragged calls on host-cut prefix panels (one per cutoff index) + one predict per cutoff index."""
    ds, y, hz = kw['ds_ns'], kw['y'], kw['horizon']
    N = len(y) if off is None else len(off) - 1
    plan = fc.cv_plan(ds, hz, kw.get('period'), kw.get('initial'), offsets=off, N=N)
    fo = np.concatenate([[0], np.cumsum(plan['n_folds'])])
    C = int(plan['n_folds'].max())
    fits = 0
    for c in range(C):
        have = np.flatnonzero(plan['n_folds'] > c)
        f = fo[have] + c
        hist, hold = plan['hist_rows'][f].astype(np.int64), plan['hold_rows'][f].astype(np.int64)
        start = np.zeros(len(have), np.int64) if off is None else off[have]
        rows = lambda a, h: np.concatenate([a[s:s + k] for s, k in zip(start, h)])    # noqa: E731
        offs = np.concatenate([[0], np.cumsum(hist)]).astype(np.int64)
        if off is None:
            dsp, yp = np.tile(ds[:hist[0]], len(have)), y[have, :hist[0]].ravel()
        else:
            dsp, yp = rows(ds, hist), rows(y, hist)
        cp = None if kw.get('cap') is None else kw['cap'][have]
        fl = None if kw.get('floor') is None else kw['floor'][have]
        sp = spec
        if spec.lbfgs.get('algorithm') == _lib.ALGO_AUTO:
            sp = fc.ModelSpec.from_dict(dict(spec.to_dict(), lbfgs=dict(spec.lbfgs, algorithm=_lib.ALGO_LBFGS)))
        r = fc.fit_ragged(sp, offs, dsp, yp, floor=fl, cap=cp)
        Hm = int(hold.max())
        fut = np.stack([ds[b + h + np.minimum(np.arange(Hm), k - 1)] for b, h, k in zip(start, hist, hold)])
        fc.predict(spec, r.theta, r.y_scale, r.grid, fut, floor=fl, cap=cp)
        fits += len(have)
    return fits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--only', choices=['cfg2', 'ref'])
    ap.add_argument('--no-by-hand', action='store_true')
    a = ap.parse_args()
    for name, spec, kw, off in panels(a.series, a.only):
        fc.cross_validate(spec, **kw)                   # warm-up (workspace, pool)
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            cv = fc.cross_validate(spec, **kw)
            wall.append(time.perf_counter() - t0)
        F = len(cv.cutoff)
        print(json.dumps({'panel': name, 'route': 'cross_validate', 'series': a.series, 'folds': F,
                          'holdout_rows': int(len(cv.yhat)), 'metric_rows': int(len(cv.horizon)),
                          'call_s': wall, 'folds_per_s': F / min(wall),
                          'grids_launches': fc.last_cv_grids(), 'mean_evals': float(cv.fit.n_eval.mean())}), flush=True)
        if a.no_by_hand:
            continue
        by_hand(spec, kw, off)
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fits = by_hand(spec, kw, off)
            wall.append(time.perf_counter() - t0)
        print(json.dumps({'panel': name, 'route': 'by hand (fit_ragged + predict per cutoff, no metrics)',
                          'series': a.series, 'folds': fits, 'call_s': wall, 'folds_per_s': fits / min(wall)}),
              flush=True)


if __name__ == '__main__':
    main()
