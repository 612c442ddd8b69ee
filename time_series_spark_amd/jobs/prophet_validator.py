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
(0.8), seed (0).  A series the plan or a fit fails (include/tsf.h TSF_CV_*) has no rows and is reported on stdout.

An optional `tune` section chooses every series' prior scales by cross-validation (include/tsf.h tsf_tune, with the
`cv` cutoffs): axes changepoint_prior_scale / seasonality_prior_scale / holidays_prior_scale as lists, metric (rmse).
An axis a model bucket has no columns for (no seasonality, no holidays) is left out of that bucket's grid and reported
as null.  It writes io.tuning, one row per series with a choice:

    series_id, dim_id, changepoint_prior_scale, seasonality_prior_scale, holidays_prior_scale, metric, score

Series without a choice are reported on stdout.  Without `tune` the job does what it did before.

An optional `scores` section scores every holdout row against its fold's predictive distribution (include/tsf.h
tsf_score_actuals, forecaster.score_cv): quantiles (a list of levels in [0, 1], may be empty), uncertainty_samples
(1000), seed (0).  It writes io.scores, one row per series that was cross-validated:

    series_id, dim_id, n_obs, crps, pinball_q<..> per level, coverage_q<..> per level

(crps and pinball_q*: the means over the series' holdout rows; coverage_q*: the share of them at or below the quantile;
names as forecaster.quantile_columns), and the fold frame gains pit and crps.  Without `scores` every output is what it
was before.

An optional `calibrate` section turns the holdout errors into a conformal calibration table (include/tsf.h
tsf_calibrate_rows, forecaster.calibrate_cv): levels (coverage targets strictly inside (0, 1), required), mode ('abs':
|y - yhat|; 'cqr': max(lower - y, y - upper) around the model's own bounds at each level, from the draws cv.seed and
cv.uncertainty_samples name), n_buckets (10 horizon buckets over cv.horizon), min_scores (20).  It writes io.calibration,
Calibration.frame's rows for every series (series_id, dim_id, bucket, horizon_upto, n_c<..> and q_c<..> per level, the
table's settings), which the scorer's forecast.calibration reads.  Without `calibrate` every output is what it was
before."""
import os
import time

import numpy as np
import pandas as pd

from .. import _lib, forecaster as fc, panel as pk
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


def tune_settings(config):
    """The `tune` section -> (grid {axis: [scales]}, metric), or None without one."""
    t = config.get('tune')
    if t is None:
        return None
    t = dict(t)
    metric = str(t.pop('metric', 'rmse')).lower()
    if metric not in _lib.TUNE_METRICS:
        raise ValueError('tune.metric must be one of %s' % sorted(_lib.TUNE_METRICS))
    unknown = sorted(set(t) - set(fc.TUNE_AXES))
    if unknown:
        raise ValueError('unknown tune keys %s (axes: %s, metric)' % (unknown, fc.TUNE_AXES))
    grid = {}
    for k in fc.TUNE_AXES:
        if k in t:
            v = t[k] if isinstance(t[k], (list, tuple)) else [t[k]]
            if not v:
                raise ValueError('tune.%s is empty' % k)
            grid[k] = [float(x) for x in v]
    if not grid:
        raise ValueError('tune needs at least one of %s' % (fc.TUNE_AXES,))
    return grid, metric


def score_settings(config):
    """The `scores` section -> dict(quantiles, uncertainty_samples, seed), or None without one."""
    sc = config.get('scores')
    if sc is None:
        return None
    sc = dict(sc)
    unknown = sorted(set(sc) - {'quantiles', 'uncertainty_samples', 'seed'})
    if unknown:
        raise ValueError('unknown scores keys %s (quantiles, uncertainty_samples, seed)' % unknown)
    q = sc.get('quantiles')
    q = [] if q is None else (list(q) if isinstance(q, (list, tuple)) else [q])
    levels = [float(x) for x in q]
    fc.quantile_columns(levels)         # (ValueError for a bad level)
    n = int(sc.get('uncertainty_samples', 1000))
    if not 2 <= n <= 4096:
        raise ValueError('scores.uncertainty_samples must be in [2, 4096]')
    return dict(quantiles=levels, uncertainty_samples=n, seed=int(sc.get('seed', 0)))


def calibrate_settings(config):
    """The `calibrate` section -> dict(levels, mode, n_buckets, min_scores), or None without one."""
    c = config.get('calibrate')
    if c is None:
        return None
    c = dict(c)
    unknown = sorted(set(c) - {'levels', 'mode', 'n_buckets', 'min_scores'})
    if unknown:
        raise ValueError('unknown calibrate keys %s (levels, mode, n_buckets, min_scores)' % unknown)
    lv = c.get('levels')
    if lv is None:
        raise ValueError('calibrate.levels is required')
    levels = [float(x) for x in (lv if isinstance(lv, (list, tuple)) else [lv])]
    mode = str(c.get('mode', 'abs')).lower()
    out = dict(levels=levels, mode=mode, n_buckets=int(c.get('n_buckets', 10)), min_scores=int(c.get('min_scores', 20)))
    fc._calib_args(levels, mode, 1, out['n_buckets'], out['min_scores'])      # (ValueError for a bad setting)
    return out


def score_columns(levels):
    """Columns of the io.scores frame for the levels of the `scores` section."""
    return (['series_id', 'dim_id', 'n_obs', 'crps'] + fc.quantile_columns(levels, 'pinball_q')
            + fc.quantile_columns(levels, 'coverage_q'))


def _buckets(config, panel):
    """Per model bucket of the modeler: (spec, members, offsets, ds, y, extra, cap of the members) -- the bucket's
    series as one ragged panel."""
    kw = pm._prophet_kwargs(config)
    cap = pk.per_series_stats(panel)[2] * config['model']['cap_multiplier']
    algo = str(kw.get('algorithm', 'auto')).lower()
    algos = {'auto': _lib.ALGO_AUTO, 'lbfgs': _lib.ALGO_LBFGS, 'newton': _lib.ALGO_NEWTON}
    if algo not in algos:
        raise ValueError("algorithm must be 'auto', 'lbfgs' or 'newton'")
    opts = pm._spec_opts(kw)
    buckets, _, hol_days, hol_extra = pm.bucket_models(panel, kw)
    for seas, members, model in buckets:
        spec = fc.ModelSpec(algorithm=algos[algo], **model, **opts)
        lens = panel.lengths[members]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = np.repeat(panel.offsets[members] - off[:-1], lens) + np.arange(off[-1], dtype=np.int64)
        ds_r, y_r = panel.ds_ns[idx], panel.y[idx]
        ex = pm.bucket_extra(spec, seas, ds_r, hol_days, hol_extra)
        yield spec, members, off, ds_r, y_r, ex, cap[members]


def _series_keys(panel):
    sids = panel.keys['series_id'].to_numpy().astype(np.int64)
    dids = panel.keys['dim_id'].to_numpy().astype(np.int64)
    return sids, dids


def validate_panel(config, panel):
    """-> (metrics frame, fold frame) for a PackedPanel."""
    return validate_scored(config, panel)[:2]


def validate_scored(config, panel):
    """-> (metrics frame, fold frame, scores frame or None without a `scores` section) for a PackedPanel."""
    return validate_calibrated(config, panel)[:3]


def validate_calibrated(config, panel):
    """-> (metrics frame, fold frame, scores frame or None, calibration frame or None without a `calibrate` section) for
    a PackedPanel."""
    cvs = cv_settings(config)
    scs = score_settings(config)
    cas = calibrate_settings(config)
    scores, tables = [], []
    floor = float(config['model']['floor'])
    sids, dids = _series_keys(panel)
    # the interval streams of a series are keyed by (series_id, dim_id): the same intervals whatever else is in the run
    key = (sids << 32) | (dids & 0xffffffff)
    metrics, folds = [], []
    for spec, members, off, ds_r, y_r, ex, cap_m in _buckets(config, panel):
        cv = fc.cross_validate(spec, ds_r, y_r, offsets=off, floor=np.full(len(members), floor), cap=cap_m,
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
        if scs is not None:
            sc = fc.score_cv(cv, scs['quantiles'], floor=np.full(len(members), floor), cap=cap_m, extra=ex,
                             series_key=key[members], uncertainty_samples=scs['uncertainty_samples'], seed=scs['seed'])
            fr['pit'], fr['crps'] = sc.pit[keep], sc.crps[keep]
            good = np.flatnonzero(cv.status == 0)
            sf = {'series_id': sids[members[good]].astype('int32'), 'dim_id': dids[members[good]].astype('int32'),
                  'n_obs': sc.n_obs[good], 'crps': sc.mean_crps[good]}
            for arr, prefix in ((sc.mean_pinball, 'pinball_q'), (sc.coverage, 'coverage_q')):
                for i, name in enumerate(fc.quantile_columns(scs['quantiles'], prefix)):
                    sf[name] = arr[good, i]
            scores.append(pd.DataFrame(sf, columns=score_columns(scs['quantiles'])))
        if cas is not None:
            cal = fc.calibrate_cv(cv, cas['levels'], mode=cas['mode'], n_buckets=cas['n_buckets'], min_scores=cas['min_scores'],
                                  horizon=cvs['horizon'], interval_width=cvs['interval_width'] if cvs['intervals'] else None,
                                  floor=np.full(len(members), floor), cap=cap_m, extra=ex, series_key=key[members],
                                  uncertainty_samples=cvs['uncertainty_samples'], seed=cvs['seed'])
            tables.append(cal.frame({'series_id': sids[members].astype('int32'), 'dim_id': dids[members].astype('int32')}))
        folds.append(pd.DataFrame(fr))
    ca_frame = None
    if cas is not None:
        ca_frame = pd.concat(tables, ignore_index=True).sort_values(['series_id', 'dim_id', 'bucket'], kind='stable')
        ca_frame = ca_frame.reset_index(drop=True)
    sc_frame = None
    if scs is not None:
        sc_frame = pd.concat(scores, ignore_index=True).sort_values(['series_id', 'dim_id'], kind='stable')
        sc_frame = sc_frame.reset_index(drop=True)
    m = pd.concat(metrics, ignore_index=True).sort_values(['series_id', 'dim_id', 'horizon'], kind='stable')
    f = pd.concat(folds, ignore_index=True).sort_values(['series_id', 'dim_id', 'cutoff', 'ds'], kind='stable')
    return m.reset_index(drop=True), f.reset_index(drop=True), sc_frame, ca_frame


def tune_panel(config, panel):
    """-> the tuning frame (one row per series with a choice) for a PackedPanel; series without one on stdout."""
    grid, metric = tune_settings(config)
    cvs = cv_settings(config)
    floor = float(config['model']['floor'])
    sids, dids = _series_keys(panel)
    out = []
    for spec, members, off, ds_r, y_r, ex, cap_m in _buckets(config, panel):
        g = dict(grid)
        if not (spec.seasonalities or spec.conditional):
            g.pop('seasonality_prior_scale', None)
        if not spec.holidays:
            g.pop('holidays_prior_scale', None)
        # (no axis left for this bucket: its own spec is the one candidate)
        r = fc.tune(spec, ds_r, y_r, cvs['horizon'], cvs['period'], cvs['initial'], offsets=off,
                    floor=np.full(len(members), floor), cap=cap_m, extra=ex, grid=g or None,
                    candidates=None if g else [spec], metric=metric, refit=False, devices=config.get('devices'))
        for i in np.flatnonzero(r.best < 0):
            n = members[i]
            why = 'no candidate scored' if r.status[i] == _lib.TUNE_NO_SCORE else \
                CV_STATUS_NAMES.get(int(r.status[i]), r.status[i])
            print(f"Tuning skipped for series_id: {sids[n]}, dim_id: {dids[n]}: {why}")
        ok = np.flatnonzero(r.best >= 0)
        b = r.best[ok]
        fr = {'series_id': sids[members[ok]].astype('int32'), 'dim_id': dids[members[ok]].astype('int32')}
        for k in fc.TUNE_AXES:
            fr[k] = r.params[k][b] if k in g else np.full(len(ok), np.nan)
        fr['metric'] = np.full(len(ok), metric, dtype=object)
        fr['score'] = r.score[ok, b]
        out.append(pd.DataFrame(fr))
    t = pd.concat(out, ignore_index=True).sort_values(['series_id', 'dim_id'], kind='stable')
    return t.reset_index(drop=True)


class ProphetValidator(object):
    """Cross-validate the models the modeler would fit (config: the modeler's keys + `cv` + io.metrics [+ io.folds]
    [+ `scores` + io.scores] [+ `calibrate` + io.calibration])."""

    def __init__(self, config):
        self.config = config

    @staticmethod
    def check_outputs(config):
        """The `calibrate` section's settings and its output path, refused before any input is read."""
        if calibrate_settings(config) is not None and not config['io'].get('calibration'):
            raise ValueError('the calibrate section needs io.calibration')

    @staticmethod
    def validate(spark_session, config, return_frame=True):
        t0 = time.time()
        ProphetValidator.check_outputs(config)
        mode = str(config['io'].get('input_mode', 'FAILFAST')).upper()
        sid, did, ds_ns, y = pm.read_model_input_dir(config['io']['input'], mode=mode)
        panel = pk.pack_rows(sid, did, ds_ns, y, key_dtypes=(np.int32, np.int32))
        if (panel.lengths < 2).any() or panel.dropped_keys:
            raise ValueError('Dataframe has less than 2 non-NaN rows.')
        pm.check_changepoints(pm._prophet_kwargs(config), panel)
        if config.get('scores') is not None and not config['io'].get('scores'):
            raise ValueError('the scores section needs io.scores')
        metrics, folds, scores, calibration = validate_calibrated(config, panel)
        tuning = tune_panel(config, panel) if config.get('tune') is not None else None
        os.makedirs(config['io']['metrics'], exist_ok=True)
        metrics.to_parquet(os.path.join(config['io']['metrics'], 'part-00000.parquet'), index=False)
        if config['io'].get('folds'):
            os.makedirs(config['io']['folds'], exist_ok=True)
            folds.to_parquet(os.path.join(config['io']['folds'], 'part-00000.parquet'), index=False)
        if scores is not None:
            os.makedirs(config['io']['scores'], exist_ok=True)
            scores.to_parquet(os.path.join(config['io']['scores'], 'part-00000.parquet'), index=False)
        if calibration is not None:
            os.makedirs(config['io']['calibration'], exist_ok=True)
            calibration.to_parquet(os.path.join(config['io']['calibration'], 'part-00000.parquet'), index=False)
        if tuning is not None:
            os.makedirs(config['io']['tuning'], exist_ok=True)
            tuning.to_parquet(os.path.join(config['io']['tuning'], 'part-00000.parquet'), index=False)
            print(f"Tuned {len(tuning)} of {panel.N} series")
        print(f"Cross-validated {panel.N} series ({len(folds)} holdout rows, {len(metrics)} metric rows) in "
              f"{time.time() - t0}")
        return (metrics, folds) if return_frame else None
