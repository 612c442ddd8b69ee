"""Cross-validation job: fbprophet's diagnostics.cross_validation + performance_metrics for every (series_id, dim_id) of
the modeler's input, on the GPU (include/tsf.h tsf_cross_validate).  The reference has no such job; this one reads the
same input directory and `model.*` keys as the modeler (jobs/prophet_modeler.py), chooses every series' model exactly
as fit_packed does (auto seasonalities from the full history, holidays, fbprophet's optimiser rule per fold), and
writes one parquet of metric rows

    series_id, dim_id, horizon, mse, rmse, mae, mape, coverage

(horizon as a duration; coverage null without intervals) and, if io.folds is set, the fold frame

    series_id, dim_id, ds, cutoff, y, yhat[, yhat_lower, yhat_upper]

Settings under `cv` (durations as pandas Timedelta strings): horizon (required), period (default horizon / 2),
initial (default 3 * horizon), rolling_window (0.1), intervals (false), uncertainty_samples (1000), interval_width
(0.8), seed (0).  A series the plan or a fit fails (include/tsf.h TSF_CV_*) has no rows and is reported on stdout."""
import os
import time

import numpy as np
import pandas as pd

from .. import _lib, features, forecaster as fc, panel as pk
from . import prophet_modeler as pm

CV_STATUS_NAMES = {_lib.CV_LESS_THAN_HORIZON: 'Less data than horizon.',
                   _lib.CV_NO_CUTOFF: 'Less data than horizon after initial window.',
                   _lib.CV_TOO_FEW: 'Less than two datapoints before cutoff.',
                   _lib.CV_FIT_FAILED: 'a fold fit failed'}


def _ns(v):
    return None if v is None else int(pd.Timedelta(v).value)


def cv_settings(config):
    c = dict(config.get('cv') or {})
    if 'horizon' not in c:
        raise ValueError('cv.horizon is required')
    return dict(horizon=_ns(c['horizon']), period=_ns(c.get('period')), initial=_ns(c.get('initial')),
                rolling_window=float(c.get('rolling_window', 0.1)), intervals=bool(c.get('intervals', False)),
                uncertainty_samples=int(c.get('uncertainty_samples', 1000)),
                interval_width=float(c.get('interval_width', 0.8)), seed=int(c.get('seed', 0)))


def validate_panel(config, panel):
    """-> (metrics frame, fold frame) for a PackedPanel."""
    cvs = cv_settings(config)
    kw = pm._prophet_kwargs(config)
    floor = float(config['model']['floor'])
    cap = pk.per_series_stats(panel)[2] * config['model']['cap_multiplier']
    algo = str(kw.get('algorithm', 'auto')).lower()
    algos = {'auto': _lib.ALGO_AUTO, 'lbfgs': _lib.ALGO_LBFGS, 'newton': _lib.ALGO_NEWTON}
    if algo not in algos:
        raise ValueError("algorithm must be 'auto', 'lbfgs' or 'newton'")
    opts = pm._spec_opts(kw)
    buckets, _, hol_days, hol_extra = pm.bucket_models(panel, kw)
    sids = panel.keys['series_id'].to_numpy().astype(np.int64)
    dids = panel.keys['dim_id'].to_numpy().astype(np.int64)
    # the interval streams of a series are keyed by (series_id, dim_id): the same intervals whatever else is in the run
    key = (sids << 32) | (dids & 0xffffffff)
    metrics, folds = [], []
    for seas, members, model in buckets:
        spec = fc.ModelSpec(algorithm=algos[algo], **model, **opts)
        lens = panel.lengths[members]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = np.repeat(panel.offsets[members] - off[:-1], lens) + np.arange(off[-1], dtype=np.int64)
        ds_r, y_r = panel.ds_ns[idx], panel.y[idx]
        ex = features.holiday_matrix(ds_r, hol_days) if hol_extra else (np.zeros((1, len(ds_r))) if not seas else None)
        cv = fc.cross_validate(spec, ds_r, y_r, offsets=off, floor=np.full(len(members), floor), cap=cap[members],
                               extra=ex, series_key=key[members], devices=config.get('devices'), **cvs)
        for i in np.flatnonzero(cv.status != 0):
            n = members[i]
            print(f"Cross-validation skipped for series_id: {sids[n]}, dim_id: {dids[n]}: "
                  f"{CV_STATUS_NAMES.get(int(cv.status[i]), cv.status[i])}")
        ok = cv.status[cv.metric_series] == 0
        ms = members[cv.metric_series[ok]]
        metrics.append(pd.DataFrame({
            'series_id': sids[ms].astype('int32'), 'dim_id': dids[ms].astype('int32'),
            'horizon': pd.to_timedelta(cv.horizon[ok], unit='ns'), 'mse': cv.mse[ok], 'rmse': cv.rmse[ok],
            'mae': cv.mae[ok], 'mape': cv.mape[ok],
            'coverage': cv.coverage[ok] if cv.coverage is not None else np.full(int(ok.sum()), np.nan)}))
        rs = members[cv.fold_series[cv.row_fold]]
        keep = cv.status[cv.fold_series[cv.row_fold]] == 0
        fr = {'series_id': sids[rs][keep].astype('int32'), 'dim_id': dids[rs][keep].astype('int32'),
              'ds': cv.ds[keep].astype('datetime64[ns]'), 'cutoff': cv.cutoff[cv.row_fold][keep].astype('datetime64[ns]'),
              'y': cv.y[keep], 'yhat': cv.yhat[keep]}
        if cv.yhat_lower is not None:
            fr['yhat_lower'], fr['yhat_upper'] = cv.yhat_lower[keep], cv.yhat_upper[keep]
        folds.append(pd.DataFrame(fr))
    m = pd.concat(metrics, ignore_index=True).sort_values(['series_id', 'dim_id', 'horizon'], kind='stable')
    f = pd.concat(folds, ignore_index=True).sort_values(['series_id', 'dim_id', 'cutoff', 'ds'], kind='stable')
    return m.reset_index(drop=True), f.reset_index(drop=True)


class ProphetValidator(object):
    """Cross-validate the models the modeler would fit (config: the modeler's keys + `cv` + io.metrics [+ io.folds])."""

    def __init__(self, config):
        self.config = config

    @staticmethod
    def validate(spark_session, config, return_frame=True):
        t0 = time.time()
        mode = str(config['io'].get('input_mode', 'FAILFAST')).upper()
        sid, did, ds_ns, y = pm.read_model_input_dir(config['io']['input'], mode=mode)
        panel = pk.pack_rows(sid, did, ds_ns, y, key_dtypes=(np.int32, np.int32))
        if (panel.lengths < 2).any() or panel.dropped_keys:
            raise ValueError('Dataframe has less than 2 non-NaN rows.')
        metrics, folds = validate_panel(config, panel)
        os.makedirs(config['io']['metrics'], exist_ok=True)
        metrics.to_parquet(os.path.join(config['io']['metrics'], 'part-00000.parquet'), index=False)
        if config['io'].get('folds'):
            os.makedirs(config['io']['folds'], exist_ok=True)
            folds.to_parquet(os.path.join(config['io']['folds'], 'part-00000.parquet'), index=False)
        print(f"Cross-validated {panel.N} series ({len(folds)} holdout rows, {len(metrics)} metric rows) in "
              f"{time.time() - t0}")
        return (metrics, folds) if return_frame else None
