"""Predict side of the drop-in boundary: same names, config keys, column order and error
behaviour as /root/reference/src/jobs/prophet_scorer.py.

    forecast_time_series(config)      prophet_scorer.py:18-104   curried grouped-map function
    extract_date                                        :107-108
    ProphetScorer.read_model_dataframe                  :123-128
    ProphetScorer.convert_forecasts                     :130-145
    ProphetScorer.write_forecasts                       :147-150
    ProphetScorer.score                                 :152-165
"""
import logging
import os
from datetime import datetime, timezone

import numpy as np
import pandas as pd

from .. import _lib, features, forecaster as fc, panel as pk

FORECAST_COLUMNS = ['series_id', 'dim_id', 'ds', 'yhat']          # prophet_scorer.py:27-32
SINK_PART_ROWS = 1 << 17           # rows per forecast CSV part (ProphetScorer.score)
SINK_WRITERS = 4                   # part files written at the same time
CONVERTED_COLUMNS = ['created_timestamp', 'series_id', 'dim_id', 'forecast_date',
                     'forecast_timestamp', 'forecast_quantity']


def _empty_forecasts():
    return pd.DataFrame(columns=FORECAST_COLUMNS)


def _future_extra(spec, fut):
    """The extra columns of a bucket's future rows fut [n][periods] -> [n][n_extra][periods], or None without any."""
    if not spec.extra:
        return None
    # holiday columns for the future dates (fbprophet rebuilds them from the holidays
    # frame it keeps in the model); any other explicit column has no future values in
    # the reference's scorer (its future frame holds ds, floor, cap only): zeros; the columns of a conditional
    # seasonality are rebuilt from the future dates like the holidays'
    ex = np.zeros((fut.shape[0], len(spec.extra), fut.shape[1]))
    if spec.holidays:
        names, _scales, days = features.holiday_columns(features.normalize_holidays(spec.holidays))
        if [e['name'] for e in spec.extra[:len(names)]] != names:
            # (not an assert: it is the only guard between a blob whose `holidays` and
            # `extra` disagree and holiday indicators multiplied into the wrong coefficients)
            raise ValueError('model blob: the holiday columns rebuilt from `holidays` do not match '
                             'the leading entries of `extra`')
        ex[:, :len(names), :] = np.moveaxis(features.holiday_matrix(fut, days), 0, 1)
    # the columns of conditional seasonalities, from the date rules the blob carries (ModelSpec.conditions)
    return fc.conditional_extra(spec, fut, extra=ex[:, :spec.n_user_extra, :])


NOISE_KEYS = ('table', 'point')


def noise_settings(config):
    """forecast.noise of a scorer configuration (optional, not in the reference) -> {'table': path, 'point': bool}, or
    None without the key.  table: the parquet the modeler's io.noise wrote (model.noise: each model's AR(1) noise state
    at the end of its history); point (default true): the point forecast and the draws start conditioned on the last
    residual -- false: the draws take the plain phi, the stationary chain, and yhat is what it was.  ValueError for an
    unknown key, a missing table, and the combinations that cannot be honoured: forecast.calibration (its table was built
    from uncorrected errors), forecast.components (that entry refuses the setting), more than one device."""
    fcfg = config.get('forecast') or {}
    if 'noise' not in fcfg or fcfg['noise'] is None:
        return None
    sec = fcfg['noise']
    if not isinstance(sec, dict):
        raise ValueError('forecast.noise must be a mapping (table, point)')
    unknown = sorted(set(sec) - set(NOISE_KEYS))
    if unknown:
        raise ValueError('forecast.noise: unknown key(s) %s (known: %s)' % (unknown, sorted(NOISE_KEYS)))
    if not sec.get('table'):
        raise ValueError('forecast.noise.table: the path of the modeler\'s io.noise is required')
    point = sec.get('point', True)
    if not isinstance(point, (bool, np.bool_)):
        raise ValueError('forecast.noise.point must be true or false')
    if fcfg.get('calibration'):
        raise ValueError('forecast.noise together with forecast.calibration: the calibration table was built from '
                         'uncorrected errors')
    if fcfg.get('components'):
        raise ValueError('forecast.noise together with forecast.components: the components\' draws refuse the setting')
    if fc.resolve_devices(config.get('devices')) is not None:
        raise ValueError('forecast.noise on more than one device: the noise setting belongs to one context')
    return {'table': str(sec['table']), 'point': bool(point)}


class NoiseTable(object):
    """forecast.noise.table, read once and joined on (series_id, dim_id) as the calibration table is: per frame of
    models the noise_ar= of the library calls.  Models without a row, with status != 0 (no phi was estimated) or whose
    future rows do not continue their history's row grid (fc.noise_lead: a weekly forecast of a daily history) are
    scored exactly as without the key -- phi = 0, which every entry takes as the independent expression bit for bit --
    counted, and reported in one printed line per call."""

    def __init__(self, settings):
        self.point = settings['point']
        df = pd.read_parquet(settings['table'])
        self.est = fc.NoiseAR.from_frame(df)
        if self.est.last_ds_ns is None or 'row_step_ns' not in df.columns:
            raise ValueError('forecast.noise.table: not a table of the modeler\'s io.noise (last_ds_ns, row_step_ns)')
        self.row_step = df['row_step_ns'].to_numpy().astype(np.int64)
        self.where = {k: i for i, k in enumerate(zip(df['series_id'].tolist(), df['dim_id'].tolist()))}
        self.counts = np.zeros(5, np.int64)

    def report(self):
        """the one line of a call: how many of its models were scored as without the key, and why"""
        c, self.counts = self.counts, np.zeros(5, np.int64)
        print('forecast.noise: %d of %d models scored without it (%d without a table row, %d without an estimate, '
              '%d whose forecast rows do not continue the history\'s)' % (c[1], c[0], c[2], c[3], c[4]))

    def noise_ar(self, sids, dids, last_ds_ns, fut):
        """-> what noise_ar= takes for these models (a NoiseARStart with `point`, else phi [n]), or None where no
        model of the frame takes part; the counts go to report()."""
        at = np.array([self.where.get(k, -1) for k in zip(np.asarray(sids).tolist(), np.asarray(dids).tolist())],
                      dtype=np.int64)
        have = at >= 0
        row = np.maximum(at, 0)
        est = self.est
        stale = np.flatnonzero(have & (est.last_ds_ns[row] != np.asarray(last_ds_ns, dtype=np.int64)))
        if len(stale):
            j = int(stale[0])
            raise ValueError('forecast.noise.table is stale: series_id %d, dim_id %d ends at %s in the table and at %s in '
                             'its model' % (int(sids[j]), int(dids[j]),
                                            np.int64(est.last_ds_ns[row[j]]).view('datetime64[ns]'),
                                            np.int64(last_ds_ns[j]).view('datetime64[ns]')))
        estimated = have & (est.status[row] == _lib.AR_OK)
        lead, ok = fc.noise_lead(last_ds_ns, np.where(have, self.row_step[row], -1), fut)
        use = estimated & ok
        self.counts += np.array([len(use), int((~use).sum()), int((~have).sum()), int((have & ~estimated).sum()),
                                 int((estimated & ~ok).sum())])
        if not use.any():
            return None
        phi = np.where(use, est.phi[row], 0.0)
        if not self.point:
            return phi
        steps = np.where(use, est.last_gap[row].astype(np.int64) + lead, 1)
        return fc.NoiseARStart(phi, np.where(use, est.last_resid[row], 0.0), steps)


def _noise_rows(noise_ar, sel):
    """the series `sel` of a noise_ar= value"""
    if noise_ar is None:
        return None
    if isinstance(noise_ar, fc.NoiseARStart):
        return fc.NoiseARStart(noise_ar.phi[sel], noise_ar.resid[sel], noise_ar.steps[sel])
    return noise_ar[sel]


def forecast_arrays(config):
    """The predict UDF on columns that never were a DataFrame: (series_id, dim_id, floor, cap, models) -> dict of the
    forecast frame's columns (series_id, dim_id int32; ds int64 ns; yhat int32; yhat_lower / yhat_upper when
    forecast.intervals; trend, trend_lower / trend_upper and the components' float64 columns when forecast.components;
    yhat_q<..> per level of forecast.quantiles and yhat_cum_q<..> with forecast.cumulative, named by fc.quantile_columns;
    yhat_lower_c<..> / yhat_upper_c<..> per level of the table forecast.calibration names, float64 like the quantile
    columns, named by fc.calibrated_columns: the validator's io.calibration applied to the float64 point forecast,
    joined on (series_id, dim_id), NaN for a model without a table row),
    `periods` rows per series, or None when there is nothing to forecast.  models: a list of blobs
    (None = no model) or the uint8 [n][L] buffer of a model column whose blobs share one length
    (panel.model_column_buffer: a parquet column as it lies in memory, no Python object per series)."""

    table = []          # forecast.calibration, read at the first frame: [Calibration, {(series_id, dim_id): row}]
    noise = noise_settings(config)          # (a refused combination fails here, before any launch)
    noise_table = []    # forecast.noise.table, read at the first frame

    def calibration_of(sid, did):
        """the rows of the calibration table for these models as a Calibration of their own (no row: no cell)"""
        if not table:
            cal, keys = fc.Calibration.from_frame(pd.read_parquet(config['forecast']['calibration']))
            table.extend([cal, {k: i for i, k in enumerate(zip(keys['series_id'].tolist(), keys['dim_id'].tolist()))}])
        cal, where = table
        at = np.array([where.get(k, -1) for k in zip(sid.tolist(), did.tolist())], dtype=np.int64)
        have = at >= 0
        q = np.where(have[:, None, None], cal.q[np.maximum(at, 0)], np.nan)
        n = np.where(have[:, None, None], cal.n[np.maximum(at, 0)], 0).astype(np.int32)
        st = np.where(have, cal.status[np.maximum(at, 0)], _lib.CALIB_NO_SCORES).astype(np.int32)
        return fc.Calibration(q, n, st, cal.levels, cal.mode, cal.horizon, cal.n_buckets, cal.min_scores)

    def forecast_arrays_fn(sids, dids, floors, caps, blobs):
        if len(sids) == 0:
            return None
        frequency = config['forecast']['frequency']
        # 'W' in pandas date_range snaps to Sundays; the reference keeps the weekday (:59-62)
        if frequency == 'W':
            frequency = pd.offsets.Week()
        periods = int(config['forecast']['periods'])
        sids, dids = np.asarray(sids), np.asarray(dids)
        floors = np.asarray(floors, dtype=np.float64)
        caps = np.asarray(caps, dtype=np.float64)
        if not isinstance(blobs, np.ndarray):
            blobs = [None if (b is None or isinstance(b, float)) else b for b in blobs]
            for i, b in enumerate(blobs):
                if b is None:
                    # prophet_scorer.py:51-55
                    print(f"For series_id: {int(sids[i])}, dim_id: {int(dids[i])}, no model found")
        pieces = []
        from ..pipeline import Laps
        lap = Laps('forecast_arrays %d' % len(sids))
        # one launch per distinct model spec (series fitted together share it)
        for spec_dict, idx, rec in pk.load_models(blobs):
            lap('load_models')
            spec = fc.ModelSpec.from_dict(spec_dict)
            theta = np.zeros((len(idx), spec.theta_stride))
            theta[:, :rec['theta'].shape[1]] = rec['theta']
            grid = pk.grid_from_records(rec)
            lap('theta + grid')
            fut = pk.future_dates(rec['last_ds_ns'], periods, frequency)  # :64-66
            lap('future_dates')
            floor, cap = floors[idx], caps[idx]                          # :67-68
            ex = _future_extra(spec, fut)
            nar = None
            if noise is not None:
                if not noise_table:
                    noise_table.append(NoiseTable(noise))
                nar = noise_table[0].noise_ar(sids[idx], dids[idx], rec['last_ds_ns'], fut)
            nkw = {} if nar is None else {'noise_ar': nar}
            if len(fut) and (fut == fut[0]).all():
                fut = np.ascontiguousarray(fut[0])           # one future grid for the batch: one shared design table on the device
            if isinstance(nar, fc.NoiseARStart):
                # the corrected point forecast with its integer column (fc.predict refuses want_int beside noise_ar)
                yhat, yint = fc.predict_conditioned(
                    spec, theta, rec['y_scale'], grid, fut, nar, floor=floor, cap=cap,
                    extra_future=ex if (ex is None or fut.ndim == 2) else np.ascontiguousarray(ex[0]))
            else:
                yhat, yint = fc.predict(spec, theta, rec['y_scale'], grid, fut, floor=floor, cap=cap,
                                        extra_future=ex if (ex is None or fut.ndim == 2) else np.ascontiguousarray(ex[0]),
                                        want_int=True,      # :70-84
                                        devices=config.get('devices'))
            lap('predict')
            iv = comps = quant = calib = None
            fcfg = config.get('forecast') or {}
            if fcfg.get('calibration'):
                # opt-in: the conformal table of the validator (io.calibration) on the float64 point forecast; a CQR
                # table first takes the model's own bounds at each level's tail pair, from the draws of the quantiles
                cal = calibration_of(sids[idx], dids[idx])
                exf = ex if (ex is None or fut.ndim == 2) else np.ascontiguousarray(ex[0])
                lw = up = None
                if cal.mode == _lib.CALIB_CQR:
                    pq = fc.predict_quantiles(
                        spec, theta, rec['y_scale'], grid, fut, fc.cv_interval_levels(cal.levels), floor=floor, cap=cap,
                        extra_future=exf,
                        series_key=(sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff),
                        uncertainty_samples=int(fcfg.get('uncertainty_samples', 1000)), seed=int(fcfg.get('seed', 0)))
                    nl = len(cal.levels)
                    lw, up = np.ascontiguousarray(pq.q[:, :nl]), np.ascontiguousarray(pq.q[:, nl:])
                calib = (cal.levels,) + cal.apply(yhat, fut, fc.model_origin_ns(grid, len(idx)), lower=lw, upper=up)
            if fcfg.get('quantiles'):
                # opt-in like the intervals below, from the same draws (same key, samples and seed: a level (1 -+ w) / 2
                # is the interval bound at width w, include/tsf.h); forecast.cumulative adds the levels of the running
                # total over the forecast rows
                fc.quantile_columns(fcfg['quantiles'])              # (a bad level list fails before any launch)
                quant = fc.predict_quantiles(
                    spec, theta, rec['y_scale'], grid, fut, fcfg['quantiles'], floor=floor, cap=cap,
                    extra_future=ex if (ex is None or fut.ndim == 2) else np.ascontiguousarray(ex[0]),
                    series_key=(sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff),
                    uncertainty_samples=int(fcfg.get('uncertainty_samples', 1000)), seed=int(fcfg.get('seed', 0)),
                    cumulative=bool(fcfg.get('cumulative')), **nkw)
            if fcfg.get('intervals') or fcfg.get('components'):
                # not in the reference's output (it drops yhat_lower / yhat_upper and the components, :86): opt-in
                # extra columns; the random streams are keyed by (series_id, dim_id), so a series gets the
                # same interval whatever frame it arrives in
                key = (sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff)
                kw = dict(floor=floor, cap=cap,
                          extra_future=ex if (ex is None or fut.ndim == 2) else np.ascontiguousarray(ex[0]),
                          series_key=key, uncertainty_samples=int(fcfg.get('uncertainty_samples', 1000)),
                          interval_width=float(fcfg.get('interval_width', 0.8)), seed=int(fcfg.get('seed', 0)))
                if fcfg.get('components'):
                    # (its yhat_lower / yhat_upper are predict_intervals' bit for bit: include/tsf.h)
                    comps = fc.predict_components(spec, theta, rec['y_scale'], grid, fut,
                                                  intervals=bool(fcfg.get('intervals')),
                                                  devices=config.get('devices'), **kw)
                    if fcfg.get('intervals'):
                        iv = (comps.yhat_lower, comps.yhat_upper)
                else:
                    _, lo, hi = fc.predict_intervals(spec, theta, rec['y_scale'], grid, fut, **kw, **nkw)
                    iv = (lo, hi)
            for j in np.flatnonzero((np.trunc(yhat) < floor[:, None]).any(axis=1)):
                print(f"Negative forecast values found for series_id: {int(sids[idx[j]])}, "
                      f"dim_id: {int(dids[idx[j]])}")                    # :77-79
            if fut.ndim == 1:
                fut = np.broadcast_to(fut, (len(idx), periods))
            pieces.append((idx, fut, yint, iv, comps, quant, calib))
            lap('negative check')
        if noise_table:
            noise_table[0].report()
        if not pieces:
            return None

        def cat(parts):                     # one launch (the usual case): its array, not a copy of it
            return parts[0] if len(parts) == 1 else np.concatenate(parts)
        res = {
            'series_id': cat([np.repeat(sids[p[0]].astype('int32'), periods) for p in pieces]),
            'dim_id': cat([np.repeat(dids[p[0]].astype('int32'), periods) for p in pieces]),
            'ds': cat([np.ascontiguousarray(p[1]).reshape(-1) for p in pieces]),
            'yhat': cat([p[2].reshape(-1) for p in pieces]).astype('int32', copy=False),
        }
        if pieces[0][3] is not None:
            res['yhat_lower'] = np.concatenate([p[3][0].reshape(-1) for p in pieces])
            res['yhat_upper'] = np.concatenate([p[3][1].reshape(-1) for p in pieces])
        if pieces[0][4] is not None:
            # forecast.components: trend (+ trend_lower / trend_upper with intervals) and one column per component name of
            # any bucket, 0.0 where a bucket's model has no such component (what an absent term contributes)
            res['trend'] = np.concatenate([p[4].trend.reshape(-1) for p in pieces])
            if pieces[0][4].intervals:
                res['trend_lower'] = np.concatenate([p[4].trend_lower.reshape(-1) for p in pieces])
                res['trend_upper'] = np.concatenate([p[4].trend_upper.reshape(-1) for p in pieces])
            for name in sorted(set().union(*[p[4].names for p in pieces])):
                res[name] = np.concatenate([p[4].terms[name].reshape(-1) if name in p[4].terms
                                            else np.zeros(len(p[0]) * periods) for p in pieces])
        if pieces[0][5] is not None:
            # forecast.quantiles (+ forecast.cumulative): one column per level, the same levels in every bucket
            for prefix, attr in (('yhat_q', 'q'), ('yhat_cum_q', 'cum_q')):
                if getattr(pieces[0][5], attr) is not None:
                    for i, name in enumerate(fc.quantile_columns(pieces[0][5].quantiles, prefix)):
                        res[name] = np.concatenate([getattr(p[5], attr)[:, i, :].reshape(-1) for p in pieces])
        if pieces[0][6] is not None:
            # forecast.calibration: one pair of columns per level of the table, the same table in every bucket
            for k, prefix in ((1, 'yhat_lower_c'), (2, 'yhat_upper_c')):
                for i, name in enumerate(fc.calibrated_columns(pieces[0][6][0], prefix)):
                    res[name] = np.concatenate([p[6][k][:, i, :].reshape(-1) for p in pieces])
        lap('columns')
        lap.__exit__()
        return res

    return forecast_arrays_fn


def forecast_panel(config):
    """Batched form of forecast_time_series: the model frame may hold any number of rows
    (one per fitted series); returns periods rows per series."""
    arrays = forecast_arrays(config)

    def forecast_panel_fn(pdf):
        if len(pdf.index) == 0:
            return _empty_forecasts()
        cols = arrays(pdf['series_id'].to_numpy(), pdf['dim_id'].to_numpy(), pdf['floor'].to_numpy(dtype=np.float64),
                      pdf['cap'].to_numpy(dtype=np.float64), pdf['model'].tolist())
        if cols is None:
            return _empty_forecasts()
        cols['ds'] = cols['ds'].view('datetime64[ns]')
        # (copy=True stacks the three int32 columns into one block: a copy of 900 000 x 3)
        return pd.DataFrame(cols, columns=FORECAST_COLUMNS + [c for c in cols if c not in FORECAST_COLUMNS], copy=False)

    return forecast_panel_fn


def rollup_panel(config):
    """forecast.rollup: {by: series_id, quantiles: [...], cumulative: bool} -- the predictive distribution of the TOTAL of
    every series_id over its dim_ids (fc.Rollup, include/tsf.h "group roll-ups"): the model frame -> one frame of
    `periods` rows per distinct series_id with columns series_id int32, ds, yhat float64 (the sum of the members' yhat, not
    truncated), count int64 (models summed), then yhat_q<..> per level and, with cumulative, yhat_cum_q<..> (the levels
    of the running total over the forecast rows).  Same uncertainty_samples, seed and series key (series_id << 32) ^ dim_id
    as forecast.quantiles, so a group of one model has that model's quantile columns.  One Rollup for the frame, one add
    per spec bucket of pk.load_models in its order.  The members are taken as independent given their fits.  All models
    must share one forecast calendar: a total over different dates is a decision the job does not take silently."""

    def rollup_panel_fn(pdf):
        fcfg = config['forecast']
        ro = fcfg['rollup']
        if ro.get('by', 'series_id') != 'series_id':
            raise ValueError('forecast.rollup.by: only series_id is supported')
        levels = list(ro['quantiles'])
        names = fc.quantile_columns(levels)                      # (a bad level list fails before any launch)
        if not names:
            raise ValueError('forecast.rollup.quantiles: at least one level')
        cumulative = bool(ro.get('cumulative'))
        cum_names = fc.quantile_columns(levels, 'yhat_cum_q') if cumulative else []
        frequency = fcfg['frequency']
        if frequency == 'W':
            frequency = pd.offsets.Week()
        periods = int(fcfg['periods'])
        sids, dids = pdf['series_id'].to_numpy(), pdf['dim_id'].to_numpy()
        floors, caps = pdf['floor'].to_numpy(dtype=np.float64), pdf['cap'].to_numpy(dtype=np.float64)
        blobs = [None if (b is None or isinstance(b, float)) else b for b in pdf['model'].tolist()]
        uniq, group = fc.rollup_groups(sids.astype(np.int64))
        roll = cal = None
        noise = noise_settings(config)
        noise_table = NoiseTable(noise) if noise is not None else None
        try:
            for spec_dict, idx, rec in pk.load_models(blobs):
                spec = fc.ModelSpec.from_dict(spec_dict)
                theta = np.zeros((len(idx), spec.theta_stride))
                theta[:, :rec['theta'].shape[1]] = rec['theta']
                fut = pk.future_dates(rec['last_ds_ns'], periods, frequency)
                if cal is None:
                    cal = np.ascontiguousarray(fut[0])
                other = np.flatnonzero((fut != cal).any(axis=1))
                if len(other):
                    d = fut[other[0]]
                    raise ValueError('forecast.rollup needs one forecast calendar for all models: %s and %s differ '
                                     '(series_id %d, dim_id %d)'
                                     % (cal[cal != d][0].view('datetime64[ns]'), d[cal != d][0].view('datetime64[ns]'),
                                        int(sids[idx[other[0]]]), int(dids[idx[other[0]]])))
                if roll is None:
                    roll = fc.Rollup(cal, len(uniq), uncertainty_samples=int(fcfg.get('uncertainty_samples', 1000)),
                                     seed=int(fcfg.get('seed', 0)))
                ex = _future_extra(spec, fut[:1])                # (one calendar: one set of columns for the bucket)
                nar = None if noise_table is None else noise_table.noise_ar(sids[idx], dids[idx], rec['last_ds_ns'], fut)
                roll.add(spec, theta, rec['y_scale'], pk.grid_from_records(rec), group[idx],
                         (sids[idx].astype(np.int64) << 32) ^ (dids[idx].astype(np.int64) & 0xffffffff),
                         floor=floors[idx], cap=caps[idx], extra_future=None if ex is None else ex[0],
                         **({} if nar is None else {'noise_ar': nar}))
            if noise_table is not None:
                noise_table.report()
            if roll is None:
                return pd.DataFrame(columns=['series_id', 'ds', 'yhat', 'count'] + names + cum_names)
            r = roll.quantiles(levels, cumulative=cumulative)
        finally:
            if roll is not None:
                roll.close()
        cols = {'series_id': np.repeat(uniq.astype('int32'), periods),
                'ds': np.tile(cal, len(uniq)).view('datetime64[ns]'),
                'yhat': r.yhat.reshape(-1), 'count': np.repeat(r.count, periods)}
        for i, name in enumerate(names):
            cols[name] = r.q[:, i, :].reshape(-1)
        for i, name in enumerate(cum_names):
            cols[name] = r.cum_q[:, i, :].reshape(-1)
        return pd.DataFrame(cols, columns=list(cols))

    return rollup_panel_fn


PERIOD_KEYS = ('freq', 'rows', 'quantiles')


def period_settings(config):
    """forecast.period_totals of a scorer configuration -> {'freq', 'rows', 'quantiles'} (one of freq / rows is None),
    or None without the key.  ValueError for an unknown key, for both or neither of freq and rows, for a freq outside
    fc.PERIOD_FREQS, rows < 1 and a bad or empty level list.  (`forecast.periods` is the number of rows to forecast.)"""
    pt = (config.get('forecast') or {}).get('period_totals')
    if not pt:
        return None
    unknown = set(pt) - set(PERIOD_KEYS)
    if unknown:
        raise ValueError('forecast.period_totals: unknown keys %s' % sorted(unknown))
    freq, rows = pt.get('freq'), pt.get('rows')
    if (freq is None) == (rows is None):
        raise ValueError('forecast.period_totals: give freq (one of %s) or rows, not both' % (fc.PERIOD_FREQS,))
    if freq is not None and freq not in fc.PERIOD_FREQS:
        raise ValueError('forecast.period_totals.freq must be one of %s' % (fc.PERIOD_FREQS,))
    if rows is not None and int(rows) < 1:
        raise ValueError('forecast.period_totals.rows must be >= 1')
    levels = list(pt.get('quantiles') or [])
    if not fc.quantile_columns(levels):
        raise ValueError('forecast.period_totals.quantiles: at least one level')
    return {'freq': freq, 'rows': None if rows is None else int(rows), 'quantiles': levels}


def period_columns(levels):
    """the columns of the period frame behind the model's key columns"""
    return ['period_start', 'period_end', 'n_rows', 'yhat'] + fc.quantile_columns(levels)


def period_panel(config):
    """forecast.period_totals: {freq: D | W | M | Q | Y, quantiles: [...]} (or rows: n in place of freq: blocks of n
    forecast rows) -- the predictive distribution of every model's TOTAL over each calendar period of its forecast rows
    (fc.predict_windows, include/tsf.h "totals over row windows"): the model frame -> one frame of one row per model
    and period, in the order of the model frame, with columns series_id, dim_id int32, period_start, period_end (the
    dates of the period's first and last forecast row), n_rows (the first and the last period may be incomplete),
    yhat float64 (the sum of the period's point forecasts, not truncated), then yhat_q<..> per level.  Same
    uncertainty_samples, seed and series key (series_id << 32) ^ dim_id as forecast.quantiles.  Models whose forecast
    calendars differ get the periods of their own calendar: one call per distinct calendar of a spec bucket."""

    def period_panel_fn(pdf):
        fcfg = config['forecast']
        st = period_settings(config)
        levels = st['quantiles']
        names = fc.quantile_columns(levels)
        frequency = fcfg['frequency']
        if frequency == 'W':
            frequency = pd.offsets.Week()
        periods = int(fcfg['periods'])
        sids, dids = pdf['series_id'].to_numpy(), pdf['dim_id'].to_numpy()
        floors, caps = pdf['floor'].to_numpy(dtype=np.float64), pdf['cap'].to_numpy(dtype=np.float64)
        blobs = [None if (b is None or isinstance(b, float)) else b for b in pdf['model'].tolist()]
        parts = []              # (row of the model frame, its K rows as a dict of columns)
        noise = noise_settings(config)
        noise_table = NoiseTable(noise) if noise is not None else None
        for spec_dict, idx, rec in pk.load_models(blobs):
            spec = fc.ModelSpec.from_dict(spec_dict)
            theta = np.zeros((len(idx), spec.theta_stride))
            theta[:, :rec['theta'].shape[1]] = rec['theta']
            grid = pk.grid_from_records(rec)
            fut = pk.future_dates(rec['last_ds_ns'], periods, frequency)
            ex = _future_extra(spec, fut)
            nar = None if noise_table is None else noise_table.noise_ar(sids[idx], dids[idx], rec['last_ds_ns'], fut)
            cals, which = np.unique(fut, axis=0, return_inverse=True)
            which = which.reshape(-1)
            for c, cal in enumerate(cals):
                sel = np.flatnonzero(which == c)
                cal = np.ascontiguousarray(cal)
                w = fc.period_windows(cal, st['freq']) if st['freq'] else fc.row_windows(periods, st['rows'])
                r = fc.predict_windows(
                    spec, theta[sel], rec['y_scale'][sel], grid if len(grid) == 1 else grid[sel], cal, w, levels,
                    floor=floors[idx][sel], cap=caps[idx][sel],
                    extra_future=None if ex is None else np.ascontiguousarray(ex[sel[0]]),
                    series_key=(sids[idx][sel].astype(np.int64) << 32) ^ (dids[idx][sel].astype(np.int64) & 0xffffffff),
                    uncertainty_samples=int(fcfg.get('uncertainty_samples', 1000)), seed=int(fcfg.get('seed', 0)),
                    **({} if nar is None else {'noise_ar': _noise_rows(nar, sel)}))
                for j, n in enumerate(sel):
                    parts.append((int(idx[n]), r.frame(j)))
        if noise_table is not None:
            noise_table.report()
        if not parts:
            return pd.DataFrame(columns=['series_id', 'dim_id'] + period_columns(levels))
        parts.sort(key=lambda p: p[0])
        out = pd.concat([f for _, f in parts], ignore_index=True)
        rows = np.repeat([i for i, _ in parts], [len(f) for _, f in parts])
        out.insert(0, 'dim_id', dids[rows].astype('int32'))
        out.insert(0, 'series_id', sids[rows].astype('int32'))
        assert list(out.columns) == ['series_id', 'dim_id'] + period_columns(levels) and names
        return out

    return period_panel_fn


def forecast_time_series(config):
    """Forecast using trained time series model (series_id, dim_id) -- prophet_scorer.py:18."""
    batched = forecast_panel(config)

    def forecast_time_series_udf(pdf):
        return batched(pdf)

    return forecast_time_series_udf


def extract_date(datetimestamp):
    return datetimestamp.date().strftime("%Y-%m-%d")                      # :107-108


class ProphetScorer:
    """Forecast quantities using trained models (prophet_scorer.py:114-165), Spark-free."""

    def __init__(self, config, logger=None):
        self.logger = logger or logging.getLogger(self.__class__.__name__)
        self.config = config

    def read_model_dataframe(self, spark=None):
        return pd.read_parquet(self.config['io']['models'])               # :124-126

    @staticmethod
    def convert_forecasts(forecast_df):
        created_timestamp = datetime.now(timezone.utc).replace(microsecond=0).isoformat()
        ds = forecast_df['ds'].values.astype('datetime64[ns]')
        # extract_date per distinct day (the column repeats a few hundred dates)
        inv, days = pd.factorize(ds.astype('datetime64[D]').astype(np.int64))
        names = np.array([extract_date(pd.Timestamp(int(d), unit='D').to_pydatetime()) for d in days],
                         dtype=object)
        out = pd.DataFrame({
            'created_timestamp': created_timestamp,
            'series_id': forecast_df['series_id'].values,
            'dim_id': forecast_df['dim_id'].values,
            'forecast_date': names[inv.reshape(-1)] if len(ds) else names,
            'forecast_timestamp': ds,
            'forecast_quantity': forecast_df['yhat'].values,
        }, columns=CONVERTED_COLUMNS)
        return out

    def write_forecasts(self, output_df):
        """CSV with header, mode='overwrite' (:148-150).  Timestamps are written the way
        Spark 2.4's CSV writer does by default (timestampFormat yyyy-MM-dd'T'HH:mm:ss.SSSXXX)
        with the wall times taken as UTC: 2002-12-28T22:00:00.000Z."""
        import shutil
        import pyarrow as pa
        import pyarrow.csv as pacsv
        path = self.config['io']['forecasts']
        if os.path.isdir(path):
            shutil.rmtree(path)
        os.makedirs(path, exist_ok=True)
        def text_column(codes, values):
            # few distinct strings, many rows: decode a dictionary inside arrow
            d = pa.DictionaryArray.from_arrays(pa.array(codes.astype(np.int32)), pa.array(values, type=pa.string()))
            return d.cast(pa.string())

        cols = {}
        for c in output_df.columns:
            v = output_df[c].values
            if np.issubdtype(v.dtype, np.datetime64):
                u, inv = np.unique(v.astype('datetime64[ns]'), return_inverse=True)
                cols[c] = text_column(inv.reshape(-1), [t + 'Z' for t in np.datetime_as_string(u, unit='ms')])
            elif v.dtype == object:
                codes, uniq = pd.factorize(v)
                cols[c] = text_column(codes, [str(x) for x in uniq])
            else:
                cols[c] = pa.array(v)
        with open(os.path.join(path, 'part-00000.csv'), 'wb') as f:
            f.write((','.join(output_df.columns) + '\n').encode())
            pacsv.write_csv(pa.table(cols), f,
                            write_options=pacsv.WriteOptions(include_header=False, quoting_style='none'))

    def _write_frame(self, path, df, time_columns):
        """A frame as one CSV with a header under `path` (timestamps as write_forecasts writes them; the float64 columns
        with repr's digits, so they read back bit for bit)."""
        import shutil
        if os.path.isdir(path):
            shutil.rmtree(path)
        os.makedirs(path, exist_ok=True)
        out = df.copy()
        for c in time_columns:
            out[c] = [t + 'Z' for t in np.datetime_as_string(out[c].values.astype('datetime64[ns]'), unit='ms')]
        out.to_csv(os.path.join(path, 'part-00000.csv'), index=False)

    def write_rollup(self, rollup_df):
        """The roll-up frame as one CSV with a header under io.rollup_forecasts (_write_frame)."""
        self._write_frame(self.config['io']['rollup_forecasts'], rollup_df, ['ds'])

    def write_periods(self, period_df):
        """The period frame (period_panel) as one CSV with a header under io.period_forecasts, written as write_rollup
        writes."""
        self._write_frame(self.config['io']['period_forecasts'], period_df, ['period_start', 'period_end'])

    def _clear_forecasts(self):
        """-> function that waits until the previous run's files are gone (pipeline.clear_directory)"""
        from ..pipeline import clear_directory
        return clear_directory(self.config['io']['forecasts'])

    def _write_converted_part(self, k, cols, created_timestamp, lo=0, hi=None):
        """part-<k>.csv (with its own header, as each of Spark's part files has: :148-150) from rows [lo, hi) of forecast
        columns: series_id, dim_id, yhat int32 (or int64) and ds int64 ns / datetime64[ns]."""
        from .. import _lib
        if lo or hi is not None:
            cols = {c: np.asarray(cols[c])[lo:hi] for c in FORECAST_COLUMNS}
        ids = [np.asarray(cols[c]) for c in ('series_id', 'dim_id', 'yhat')]
        narrow = all(v.dtype == np.int32 for v in ids)          # forecast_panel's frame: the columns go as they are
        ids = [np.ascontiguousarray(v, dtype=np.int32 if narrow else np.int64) for v in ids]
        ds = np.asarray(cols['ds'])
        if ds.dtype != np.int64:
            ds = ds.view(np.int64) if ds.dtype == np.dtype('datetime64[ns]') else ds.astype('datetime64[ns]').astype(np.int64)
        ds = np.ascontiguousarray(ds)
        L = _lib.load()
        path = os.path.join(self.config['io']['forecasts'], 'part-%05d.csv' % k)
        rc = (L.tsf_csv_write_forecasts_i32 if narrow else L.tsf_csv_write_forecasts)(
            os.fsencode(path), created_timestamp.encode(), len(ds), ids[0].ctypes.data, ids[1].ctypes.data,
            ds.ctypes.data, ids[2].ctypes.data, 0)
        if rc != 0:
            raise OSError('tsf_csv_write_forecasts failed (%d) for %s' % (rc, path))

    def write_converted(self, forecast_df, created_timestamp=None):
        """convert_forecasts + write_forecasts in one native pass (tsf_csv_write_forecasts):
        the same file write_forecasts(convert_forecasts(forecast_df)) produces, formatted by
        threads straight from the forecast columns."""
        if created_timestamp is None:
            created_timestamp = datetime.now(timezone.utc).replace(microsecond=0).isoformat()
        wait = self._clear_forecasts()
        self._write_converted_part(0, {c: forecast_df[c].values for c in FORECAST_COLUMNS}, created_timestamp)
        wait()
        return created_timestamp

    def _model_chunks(self):
        """The model directory (:124-126) one parquet row group at a time: (series_id, dim_id, floor, cap, models)
        column tuples, models as panel.model_column_buffer gives them (the column's own bytes) or a list of blobs."""
        import pyarrow.parquet as pq
        path = self.config['io']['models']
        if os.path.isdir(path):
            parts = sorted(os.path.join(path, f) for f in os.listdir(path)
                           if not f.startswith(('_', '.')) and f.endswith('.parquet'))
        else:
            parts = [path]
        for part in parts:
            pf = pq.ParquetFile(part)
            for g in range(pf.num_row_groups):
                t = pf.read_row_group(g, columns=['series_id', 'dim_id', 'floor', 'cap', 'model'])
                if t.num_rows == 0:
                    continue
                models = pk.model_column_buffer(t.column('model'))
                if models is None:
                    models = t.column('model').to_pylist()
                yield (t.column('series_id').to_numpy(), t.column('dim_id').to_numpy(),
                       t.column('floor').to_numpy().astype(np.float64), t.column('cap').to_numpy().astype(np.float64),
                       models, t)           # (t keeps the buffers the views point into)

    @staticmethod
    def score(spark_session, config):
        """Forecast every model of io.models into io.forecasts (:152-165).  Round 6: a pipeline over the row groups of
        the model parts (time_series_spark_amd/pipeline.py): the models of group k + 1 are read while group k is on the
        GPU and the forecasts of group k - 1 are formatted and written -- one CSV part per group, each with the header,
        as Spark writes one per task.  convert_forecasts is a lazy plan in the reference (:162), fused by Spark into
        the write; here the native sink formats the converted rows straight from the forecast columns
        (_write_converted_part: the same rows write_forecasts(convert_forecasts(forecast_df)) gives, test_host.py), so
        the converted frame -- 900 000 rows of Python date strings for 10 000 series -- is never built.  Returns None, as
        the reference does.
        With forecast.rollup and io.rollup_forecasts both set, the roll-up frame (rollup_panel) is written as CSV there
        after the forecasts: a second pass over the whole model frame, not pipelined with the first.  With
        forecast.period_totals and io.period_forecasts both set, the period frame (period_panel) is written likewise."""
        from .. import pipeline
        scorer = ProphetScorer(config)
        created = datetime.now(timezone.utc).replace(microsecond=0).isoformat()
        arrays = forecast_arrays(scorer.config)
        gone = scorer._clear_forecasts()
        n_parts = []
        import concurrent.futures
        writers = concurrent.futures.ThreadPoolExecutor(max_workers=SINK_WRITERS)

        def sink(cols):
            # Buffered writes to ONE file take turns on its inode lock, however many threads issue them (measured: a
            # 370 000-row part left the sink's 32 formatting threads waiting for one another's pwrite, 15 of the scorer's
            # 25 ms on 10 000 series): a chunk goes out as several part files, SINK_PART_ROWS rows each, written side by side.
            if cols is not None:
                n = len(cols['yhat'])
                cuts = list(range(0, n, SINK_PART_ROWS)) + [n]
                futs = [writers.submit(scorer._write_converted_part, len(n_parts) + i, cols, created, a, b)
                        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
                n_parts.extend([1] * len(futs))
                for f in futs:
                    f.result()

        try:
            pipeline.run_pipeline(scorer._model_chunks(), [lambda c: arrays(*c[:5]), sink])
        finally:
            writers.shutdown()
            gone()
        if not n_parts:             # no model at all: the header alone, as an empty frame's CSV has
            scorer._write_converted_part(0, {'series_id': np.zeros(0, np.int32), 'dim_id': np.zeros(0, np.int32),
                                             'ds': np.zeros(0, np.int64), 'yhat': np.zeros(0, np.int32)}, created)
        if (scorer.config.get('forecast') or {}).get('rollup') and scorer.config['io'].get('rollup_forecasts'):
            scorer.write_rollup(rollup_panel(scorer.config)(scorer.read_model_dataframe()))
        if period_settings(scorer.config) and scorer.config['io'].get('period_forecasts'):
            scorer.write_periods(period_panel(scorer.config)(scorer.read_model_dataframe()))
