"""Times fit_aligned with specified changepoint dates against the automatic rule on the bench panel.

Panel: BASELINE cfg2's model and shape -- 10 000 series x 730 daily rows, linear growth, additive yearly + weekly --
resident on the device (DeviceForecaster, the flagship's path).  The specified dates are the 25 row timestamps the
automatic rule picks, so both variants run the same kernels on the same tables and must return the same bits (checked);
only the grid set-up differs.  A difference in time beyond the spread of the automatic leg means a route fell off its
fast path (the quadratic form not chosen, the caller's y rows not read in place).

The two variants alternate inside one process after --warmup calls of each; every call is timed with device events
around the whole entry point (set-up kernels included).  Prints one JSON line: per variant the median, the minimum and
the quartiles over --reps calls, the median of the per-pair differences, and whether the outputs are identical."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_series_spark_amd import device, forecaster as fc, synth  # noqa: E402

SEAS = [{'name': 'yearly', 'period': 365.25, 'fourier_order': 10}, {'name': 'weekly', 'period': 7, 'fourier_order': 3}]


def automatic_dates(ds, n_changepoints=25, changepoint_range=0.8):
    """The row timestamps the automatic rule picks (setup_grid_kernel; fbprophet set_changepoints)."""
    hist = int(np.floor(len(ds) * changepoint_range))
    S = min(n_changepoints, hist - 1)
    step = (hist - 1) / S
    return ds[[int(np.rint((hist - 1) if j + 1 == S else (j + 1) * step)) for j in range(S)]]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--series', type=int, default=10000)
    ap.add_argument('--rows', type=int, default=730)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    ds_np, y_np = synth.make_panel(a.series, a.rows, 'linear', seed=751)
    specs = {'automatic': fc.ModelSpec(growth='linear', seasonalities=SEAS),
             'specified': fc.ModelSpec(growth='linear', seasonalities=SEAS, changepoints=automatic_dates(ds_np))}
    dev = torch.device('cuda', 0)
    ds, y = torch.from_numpy(ds_np).to(dev), torch.from_numpy(y_np).to(dev)
    legs = {k: device.DeviceForecaster(s, 0) for k, s in specs.items()}
    outs = {k: f.alloc_fit_output(a.series) for k, f in legs.items()}
    ms = {k: [] for k in legs}
    for it in range(a.warmup + a.reps):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f.fit_aligned(ds, y, outs[k])
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    same = all(torch.equal(getattr(outs['automatic'], k), getattr(outs['specified'], k))
               for k in ('theta', 'y_scale', 'fval', 'status', 'n_iter', 'n_eval', 'grid'))
    res = {'series': a.series, 'rows': a.rows, 'warmup': a.warmup, 'reps': a.reps, 'identical_outputs': bool(same)}
    for k, v in ms.items():
        q = np.percentile(v, [25, 50, 75])
        res[k + '_ms'] = {'median': round(float(q[1]), 3), 'min': round(float(min(v)), 3), 'q25': round(float(q[0]), 3),
                          'q75': round(float(q[2]), 3), 'max': round(float(max(v)), 3)}
    res['median_pair_difference_ms'] = round(float(np.median(np.array(ms['specified']) - np.array(ms['automatic']))), 3)
    print(json.dumps(res), flush=True)
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
