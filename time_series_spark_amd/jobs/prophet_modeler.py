"""Fit side of the drop-in boundary: same names, config keys, column order and error behaviour
as /root/reference/src/jobs/prophet_modeler.py, with the per-series fbprophet fit replaced by
one batched GPU fit of every (series_id, dim_id) group in the frame.

    model_time_series(config)        prophet_modeler.py:22-87   curried grouped-map function
    ProphetModeler.read_input_dataframe                  :102-116
    ProphetModeler.persist_models                        :118-125
    ProphetModeler.model                                 :127-143

Spark is optional (pyspark/JVM are not in this image): the factories return plain
`pdf -> pdf` functions; when pyspark is importable `as_pandas_udf` wraps them with the
reference's output schema for `df.groupby('series_id','dim_id').apply(...)`.  A grouped map
that hands over ONE series per call cannot batch; `model_panel(config)` takes a frame holding
many groups (e.g. grouped by a shard key) and is what ProphetModeler.model uses.
"""
import logging
import os
import time

import numpy as np
import pandas as pd

from .. import _lib, features, forecaster as fc, panel as pk

# prophet_modeler.py:12-17 (names and nullability; types: int, int, timestamp, int)
MODEL_INPUT_SCHEMA = [('series_id', 'int32'), ('dim_id', 'int32'), ('start_time', 'datetime64[ns]'),
                      ('quantity', 'int32')]
# prophet_modeler.py:32-38
MODEL_OUTPUT_COLUMNS = ['series_id', 'dim_id', 'floor', 'cap', 'model']
# fbprophet switches optimiser at this history length; these statuses are pystan RuntimeErrors
NEWTON_BELOW_T = 100
RUNTIME_ERROR_STATUS = (_lib.ST_LSFAIL, _lib.ST_INIT_NONFINITE, _lib.ST_EVAL_LIMIT)
MODEL_OUTPUT_DTYPES = {'series_id': 'int32', 'dim_id': 'int32', 'floor': 'float32', 'cap': 'float32'}


def _prophet_kwargs(config):
    """The reference hard-codes Prophet(growth='logistic', seasonality_mode='multiplicative')
    (prophet_modeler.py:65).  config['model']['prophet'] (optional, not in the reference) may
    override constructor arguments, e.g. for BASELINE config 2."""
    kw = {'growth': 'logistic', 'seasonality_mode': 'multiplicative'}
    kw.update((config.get('model') or {}).get('prophet') or {})
    return kw


# series that share a timestamp vector are fitted through the aligned entry point from this many on (fit_packed);
# config['model']['prophet']['min_aligned_group'] overrides
MIN_ALIGNED_GROUP = 4096


def _hint_kw(h):
    """cost_hints only where there are any (the keyword stays out of calls without them)"""
    return {} if h is None else {'cost_hints': h}


def previous_run_cost(models, sidecar_only=False):
    """Expected cost per (series_id, dim_id) from the models of an earlier run: the iteration count stored in every
    model blob.  models: a frame with series_id, dim_id, model columns, or the path of a model parquet directory
    (what persist_models wrote: the counts are then read from the file it leaves beside the parquet part, the blobs
    only when that file is missing or stale -- and not at all with sidecar_only).  Returns a frame series_id, dim_id,
    cost -- or None when there is nothing usable.
    A launch ends with its longest fits; nothing cheap about a series predicts them except its previous fit."""
    try:
        if isinstance(models, str):
            if not os.path.isdir(models):
                return None
            parts = sorted(f for f in os.listdir(models) if f.endswith('.parquet'))
            if not parts:
                return None
            side = _read_cost_sidecar(models, parts)
            if side is not None or sidecar_only:
                return side
            models = pd.concat([pd.read_parquet(os.path.join(models, f)) for f in parts], ignore_index=True)
        if models is None or len(models) == 0:
            return None
        cost = np.zeros(len(models), dtype=np.int64)
        for _sd, pos, rec in pk.load_models(list(models['model'])):
            cost[np.asarray(pos)] = rec['n_iter']
        return pd.DataFrame({'series_id': models['series_id'].to_numpy().astype(np.int64),
                             'dim_id': models['dim_id'].to_numpy().astype(np.int64), 'cost': cost})
    except Exception as e:                  # hints are an optimisation: a stale or foreign file must not fail the run
        print(f"previous models not usable as scheduling hints: {e}")
        return None


MODEL_ROW_GROUP = 6144          # most rows per parquet row group of a model part (a part is cut into equal groups): what
                                # the scorer's pipeline reads, forecasts and writes at a time
COST_SIDECAR = '_tsf_cost.npz'         # leading underscore: Spark and pyarrow skip it when they read the directory


class _CostVector(object):
    """The iteration counts of a model frame as ONE value of DataFrame.attrs.  pandas compares attrs dicts with `==`
    when frames are concatenated (`__finalize__`): a bare ndarray there raises "truth value of an array is ambiguous"
    as soon as two frames of more than one series meet (round-4 advice); this compares as a whole."""
    __slots__ = ('values',)

    def __init__(self, values):
        self.values = np.asarray(values)

    def __eq__(self, other):
        return isinstance(other, _CostVector) and np.array_equal(self.values, other.values)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None

    def __len__(self):
        return len(self.values)

    def __array__(self, dtype=None, copy=None):
        return self.values if dtype is None else self.values.astype(dtype)


def _write_cost_sidecar(path, parts, sids, dids, cost):
    """The iteration counts of the models persist_models wrote (ModelBatch.cost / model_df.attrs['tsf_cost']) next to
    the parquet parts, with every part's size and mtime: previous_run_cost then reads 10 000 counts in under a
    millisecond instead of parsing 10 000 model blobs (17 ms), and a directory whose parts were replaced since (names,
    sizes or mtimes differ) sends it back to the blobs."""
    if cost is None or len(cost) != len(sids):
        return
    stat = [[os.stat(os.path.join(path, f)).st_size, os.stat(os.path.join(path, f)).st_mtime_ns] for f in parts]
    np.savez(os.path.join(path, COST_SIDECAR), series_id=np.asarray(sids).astype(np.int64),
             dim_id=np.asarray(dids).astype(np.int64), cost=np.asarray(cost, dtype=np.int64),
             part=np.array(list(parts)), stat=np.array(stat, dtype=np.int64).reshape(len(parts), 2))


def _read_cost_sidecar(path, parts):
    f = os.path.join(path, COST_SIDECAR)
    if not parts or not os.path.isfile(f):
        return None
    try:
        z = np.load(f)
        if [str(x) for x in z['part']] != list(parts):
            return None
        stat = np.asarray(z['stat']).reshape(len(parts), 2)
        for f_, (size, mtime) in zip(parts, stat):
            st = os.stat(os.path.join(path, f_))
            if (st.st_size, st.st_mtime_ns) != (int(size), int(mtime)):
                return None
        return pd.DataFrame({'series_id': z['series_id'], 'dim_id': z['dim_id'], 'cost': z['cost']})
    except Exception:
        return None


def _empty_models():
    return pd.DataFrame(columns=MODEL_OUTPUT_COLUMNS)


def check_conditions(kw):
    """model.prophet.seasonalities entries may carry condition_name (fbprophet's add_seasonality(condition_name=...));
    the condition is then a date rule under model.prophet.conditions (features.condition_mask): the reference's input
    schema (series_id, dim_id, ds, y) has no column to take a condition from, so a name without a rule is an error of
    the configuration."""
    rules = kw.get('conditions') or {}
    for s in kw.get('seasonalities') or ():
        name = s.get('condition_name')
        if name is not None and name not in rules:
            raise ValueError("model.prophet.seasonalities: condition_name %r has no rule under model.prophet.conditions"
                             % (name,))
    for rule in rules.values():
        features.normalize_condition_rule(rule)


def bucket_extra(spec, seas, ds, hol_days, hol_extra):
    """The `extra` array of a bucket's rows ds: the holiday indicators (or fbprophet's zero column of a model without
    any seasonality), then the columns of the spec's conditional seasonalities from its date rules."""
    ex = features.holiday_matrix(ds, hol_days) if hol_extra else (np.zeros((1, len(ds))) if not seas else None)
    return fc.conditional_extra(spec, ds, extra=ex)


def bucket_models(panel, kw):
    """The models fbprophet would build for the series of a PackedPanel: series are bucketed by the seasonality set
    fbprophet's 'auto' rules give their own history (each Prophet object decides alone).  Returns (buckets, holidays,
    holiday days, holiday columns); buckets = [(seasonalities, members (sorted), model dict for ModelSpec)]."""
    check_conditions(kw)
    span, min_dt, _ = pk.per_series_stats(panel)
    mode = kw.get('seasonality_mode', 'additive')
    growth = kw.get('growth', 'linear')
    sps = float(kw.get('seasonality_prior_scale', 10.0))
    # the auto rules depend on the series only through three booleans
    sig = ((span < 730 * fc.DAY_NS).astype(np.int8)
           | (((span < 14 * fc.DAY_NS) | ((min_dt >= 0) & (min_dt >= 7 * fc.DAY_NS))).astype(np.int8) << 1)
           | (((span < 2 * fc.DAY_NS) | ((min_dt >= 0) & (min_dt >= fc.DAY_NS))).astype(np.int8) << 2))
    specs = {}
    for code in np.flatnonzero(np.bincount(sig, minlength=8)):
        members = np.flatnonzero(sig == code)
        n0 = int(members[0])
        seas = fc.ModelSpec.auto_from_stats(
            int(span[n0]), int(min_dt[n0]), yearly=kw.get('yearly_seasonality', 'auto'),
            weekly=kw.get('weekly_seasonality', 'auto'), daily=kw.get('daily_seasonality', 'auto'),
            seasonality_mode=mode, seasonality_prior_scale=sps,
            user_seasonalities=kw.get('seasonalities', ()))
        key = tuple((s['name'], s['fourier_order']) for s in seas)
        if key in specs:
            specs[key] = (seas, np.concatenate([specs[key][1], members]))
        else:
            specs[key] = (seas, members)
    # holidays: Prophet(holidays=...) -> indicator columns after the seasonalities,
    # sorted by name, one prior scale per holiday, mode = seasonality_mode
    hol = features.normalize_holidays(kw.get('holidays'), float(kw.get('holidays_prior_scale', 10.0)))
    hol_names, hol_scales, hol_days = features.holiday_columns(hol)
    hol_extra = [{'name': n, 'prior_scale': p, 'mode': mode} for n, p in zip(hol_names, hol_scales)]
    buckets = []
    for key, (seas, members) in specs.items():
        members = np.sort(np.asarray(members))
        if hol_extra:
            model = dict(growth=growth, seasonality_mode=mode, seasonalities=seas, extra=hol_extra, holidays=hol)
        elif not seas:
            # fbprophet adds a zero column when there is no seasonality at all
            model = dict(growth=growth, seasonality_mode=mode, seasonalities=[],
                         extra=[{'name': 'zeros', 'prior_scale': 1.0, 'mode': 'additive'}])
        else:
            model = dict(growth=growth, seasonality_mode=mode, seasonalities=seas)
        if any(s.get('condition_name') is not None for s in seas):
            model['conditions'] = kw.get('conditions')        # (the rules travel with the model: ModelSpec.to_dict)
        buckets.append((seas, members, model))
    return buckets, hol, hol_days, hol_extra


SCREEN_DEFAULTS = {'threshold': 5.0, 'max_share': 0.05, 'min_rows': 10, 'passes': 1}
SCREENED_COLUMNS = ['series_id', 'dim_id', 'ds', 'y', 'resid', 'center', 'scale']


def screen_settings(config):
    """config['model']['screen'] (optional, not in the reference): outlier screening of every fit (fc.fit_screened:
    fit, flag the rows whose residual lies beyond threshold robust scales -- at most max_share of a series' rows --,
    cut them, fit again, `passes` rounds).  None without the section; else the keywords of fc.fit_screened, defaults
    filled in.  An unknown key or a value the library would refuse raises ValueError."""
    sec = (config.get('model') or {}).get('screen')
    if sec is None:
        return None
    if not isinstance(sec, dict):
        raise ValueError('model.screen must be a mapping (threshold, max_share, min_rows, passes)')
    unknown = sorted(set(sec) - set(SCREEN_DEFAULTS))
    if unknown:
        raise ValueError('model.screen: unknown key(s) %s (known: %s)' % (unknown, sorted(SCREEN_DEFAULTS)))
    out = dict(SCREEN_DEFAULTS, **sec)
    out['threshold'], out['max_share'] = float(out['threshold']), float(out['max_share'])
    fc._screen_args(out['threshold'], out['max_share'], out['min_rows'], out['passes'])     # (ValueError)
    out['min_rows'], out['passes'] = int(out['min_rows']), int(out['passes'])
    return out


def _empty_screened():
    return pd.DataFrame({'series_id': np.zeros(0, np.int32), 'dim_id': np.zeros(0, np.int32),
                         'ds': np.zeros(0, 'datetime64[ns]'), 'y': np.zeros(0), 'resid': np.zeros(0),
                         'center': np.zeros(0), 'scale': np.zeros(0)}, columns=SCREENED_COLUMNS)


NOISE_DEFAULTS = {'phi_max': 0.95, 'min_pairs': 8}
NOISE_FIELDS = ['phi', 'phi_raw', 'n_pairs', 'scale', 'status', 'last_resid', 'last_gap', 'last_ds_ns']
NOISE_COLUMNS = ['series_id', 'dim_id'] + NOISE_FIELDS + ['row_step_ns']
_NOISE_DTYPES = {'phi': np.float64, 'phi_raw': np.float64, 'n_pairs': np.int64, 'scale': np.float64, 'status': np.int32,
                 'last_resid': np.float64, 'last_gap': np.int32, 'last_ds_ns': np.int64}


def noise_settings(config):
    """config['model']['noise'] (optional, not in the reference): the AR(1) noise state of every fit (fc.fit_noise_state:
    each series' residual autocorrelation and the residual of its last present row, from the history the fit has just
    seen), for the scorer's forecast.noise.  None without the section; else the keywords phi_max, min_pairs of
    fc.fit_noise_state, defaults filled in (an empty mapping: the defaults).  An unknown key or a value the library
    would refuse raises ValueError."""
    model = config.get('model') or {}
    if 'noise' not in model:
        return None
    sec = {} if model['noise'] is None else model['noise']
    if not isinstance(sec, dict):
        raise ValueError('model.noise must be a mapping (phi_max, min_pairs)')
    unknown = sorted(set(sec) - set(NOISE_DEFAULTS))
    if unknown:
        raise ValueError('model.noise: unknown key(s) %s (known: %s)' % (unknown, sorted(NOISE_DEFAULTS)))
    out = dict(NOISE_DEFAULTS, **sec)
    out['phi_max'] = float(out['phi_max'])
    fc._ar_args(out['phi_max'], out['min_pairs'])            # (ValueError)
    out['min_pairs'] = int(out['min_pairs'])
    return out


def check_noise_io(config):
    """io.noise is where model.noise's table goes: the one without the other is an error of the configuration."""
    if (config.get('io') or {}).get('noise') and noise_settings(config) is None:
        raise ValueError('io.noise needs model.noise')


def _empty_noise():
    cols = {'series_id': np.zeros(0, np.int32), 'dim_id': np.zeros(0, np.int32)}
    cols.update((f, np.zeros(0, _NOISE_DTYPES[f])) for f in NOISE_FIELDS)
    cols['row_step_ns'] = np.zeros(0, np.int64)
    return pd.DataFrame(cols, columns=NOISE_COLUMNS)


def fit_packed(panel, floor, cap, kw, devices=None, cost=None, lap=None, screen=None, removed=None, noise=None,
               noise_out=None):
    """Fit every series of a PackedPanel.  Series are bucketed by the seasonality set
    fbprophet's 'auto' rules give their own history (each Prophet object decides alone), one
    kernel launch per bucket.  Returns (pieces, status, n_iter): pieces = [(members, buffer)] -- the blobs of one fit
    call, uint8 [len(members)][stride] (panel.dump_models_buffer), row i the model of series members[i]; a series whose
    status is negative has no model, and a later piece (fbprophet's Newton retry) supersedes an earlier one.
    cost: optional [N] expected relative cost per series (the iteration counts of the previous run's models):
    scheduling hints for the launches (tsf_set_cost_hints); results do not depend on them.
    screen: screen_settings(config) or None -- every fit call becomes fc.fit_screened with these keywords (same spec,
    same groups, same Newton retry on top); removed: a dict that then receives, per series with flagged rows,
    (ds, y, resid, center, scale) of those rows (a later fit of the series supersedes an earlier one).
    noise: noise_settings(config) or None -- behind every fit call fc.fit_noise_state on the same arrays (with `screen`
    the flagged rows as `excluded`); noise_out: a dict {field: [N] array} (NOISE_FIELDS) that receives each series'
    state (a later fit of the series supersedes an earlier one)."""
    N = panel.N
    lap = lap or (lambda name: None)
    hint = (lambda mem: None) if cost is None else (lambda mem: np.asarray(cost)[mem])
    mode = kw.get('seasonality_mode', 'additive')
    buckets, _, hol_days, hol_extra = bucket_models(panel, kw)
    pieces = []
    status = np.zeros(N, dtype=np.int32)
    n_iter = np.zeros(N, dtype=np.int32)
    # make_future_dataframe starts at history_dates.max(): the last ds of the group INCLUDING rows
    # whose y is null (fbprophet Prophet.fit keeps them in history_dates)
    last_ds = panel.last_ds_all
    algo = str(kw.get('algorithm', 'auto')).lower()
    if algo not in ('auto', 'lbfgs', 'newton'):
        raise ValueError("algorithm must be 'auto', 'lbfgs' or 'newton'")
    opts = _spec_opts(kw)
    min_group = int(kw.get('min_aligned_group', MIN_ALIGNED_GROUP))
    lap('specs')

    def fit_call(spec, mem, ds, y, off, fl, cp, ex):
        """fit_plain, and with `noise` the noise state of its fits"""
        res, flag = fit_plain(spec, mem, ds, y, off, fl, cp, ex)
        if noise is not None:
            est = fc.fit_noise_state(spec, res, ds, y, offsets=off, floor=fl, cap=cp, extra=ex, excluded=flag, **noise)
            for f in NOISE_FIELDS:
                noise_out[f][mem] = getattr(est, f)
            lap('fit_noise_state %d' % len(mem))
        return res

    def fit_plain(spec, mem, ds, y, off, fl, cp, ex):
        """fit_aligned (off None: y [G][T]) / fit_ragged of the series mem -- or, with `screen`, fit_screened;
        -> (FitResult, the flagged rows in y's layout or None)"""
        if screen is None:
            if off is None:
                return fc.fit_aligned(spec, ds, y, floor=fl, cap=cp, extra=ex, devices=devices, **_hint_kw(hint(mem))), None
            return fc.fit_ragged(spec, off, ds, y, floor=fl, cap=cp, extra=ex, devices=devices, **_hint_kw(hint(mem))), None
        sf = fc.fit_screened(spec, ds, y, offsets=off, floor=fl, cap=cp, extra=ex, devices=devices, **screen)
        if removed is not None:
            sc = sf.screen
            for g in range(len(mem)):
                removed.pop(int(mem[g]), None)
            for g in np.flatnonzero(sc.n_flagged > 0):
                if off is None:
                    rows = np.flatnonzero(sc.flag[g])
                    rec = (ds[rows], y[g][rows], sc.resid[g][rows])
                else:
                    rows = int(off[g]) + np.flatnonzero(sc.flag[int(off[g]):int(off[g + 1])])
                    rec = (ds[rows], y[rows], sc.resid[rows])
                removed[int(mem[g])] = rec + (float(sc.center[g]), float(sc.scale[g]))
        return sf.fit, sf.screen.flag

    def run(spec, sd, seas, members):
        """One optimiser over `members`: series that share a timestamp vector are fitted
        together through the aligned entry point (one set of design tables for the group), the
        rest go in one ragged call."""
        # Every group is a launch of its own, and a launch lasts at least as long as its longest fit (milliseconds),
        # while the ragged kernels fit a series for 0.6 us (quadratic form) to 10 us (residual form) more than the
        # aligned ones: a group pays for its launch from a few thousand series on.  A bucket that IS one group keeps
        # the aligned path whatever its size; otherwise small groups join the ragged call (same bits either way).
        groups, rest = pk.group_by_grid(panel, members, min_group=min_group, keep_single=True)
        lap('group_by_grid')
        calls = []
        for gm in groups:
            T = int(panel.lengths[gm[0]])
            a0 = panel.offsets[gm[0]]
            y2d = pk.rows_2d(panel.y, panel.offsets, gm, T)
            ex = bucket_extra(spec, seas, panel.ds_ns[a0:a0 + T], hol_days, hol_extra)
            calls.append((gm, fit_call(
                spec, gm, panel.ds_ns[a0:a0 + T], y2d, None,
                None if floor is None else np.asarray(floor)[gm],
                None if cap is None else np.asarray(cap)[gm], ex)))
            lap('fit_aligned %d' % len(gm))
        if len(rest):
            lens = panel.lengths[rest]
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            # rows of the `rest` series, in order: start of each series repeated over its
            # length plus the position inside the series
            if len(rest) == panel.N and int(panel.offsets[0]) == 0 and int(panel.offsets[-1]) == len(panel.y):
                # every series of the panel, in order (rest is sorted): the packed columns ARE the call's rows --
                # no gather (two copies of the panel: a third of this function's time on a 10 000 x 700 panel)
                ds_r, y_r = panel.ds_ns, panel.y
            else:
                idx = np.repeat(panel.offsets[rest] - off[:-1], lens) + np.arange(off[-1], dtype=np.int64)
                ds_r, y_r = panel.ds_ns[idx], panel.y[idx]
            ex = bucket_extra(spec, seas, ds_r, hol_days, hol_extra)
            calls.append((rest, fit_call(
                spec, rest, ds_r, y_r, off,
                None if floor is None else np.asarray(floor)[rest],
                None if cap is None else np.asarray(cap)[rest], ex)))
            lap('fit_ragged %d' % len(rest))
        for mem, res in calls:
            st = np.asarray(res.status)
            status[mem] = st
            n_iter[mem] = np.asarray(res.n_iter)
            # (optimiser failure -- pystan RuntimeError -- or invalid input: status < 0, no model for the series)
            pieces.append((mem, pk.dump_models_buffer(sd, res.theta, res.y_scale, res.grid, last_ds[mem], st, res.n_iter)))
            lap('blobs')

    for seas, members, model in buckets:
        lbfgs = fc.ModelSpec(algorithm=_lib.ALGO_LBFGS, **model, **opts)
        newton = fc.ModelSpec(algorithm=_lib.ALGO_NEWTON, **model, **opts)
        sd = fc.ModelSpec(**model, **opts).to_dict()      # what predict needs: no optimiser choice
        # fbprophet 0.5: optimizing(algorithm='Newton' if T < 100 else 'LBFGS'), and Newton once
        # more after an L-BFGS RuntimeError (UPSTREAM-RECALL forecaster.py fit).  Every model the
        # library fits has a Newton kernel since round 4 (3 + n_changepoints + K <= 128 = TSF_MAX_P; one parameter
        # per lane up to 64 parameters of one column mode, two per lane beyond that and for mixed modes --
        # newton_kernel2, slow but there: a failed fit of a wide model is retried as the reference would, not dropped).
        modes = {s_.get('mode', mode) for s_ in seas} | ({mode} if hol_extra else set())
        newton_ok = 3 + lbfgs.n_changepoints + lbfgs.K <= 128
        if algo == 'newton' and not newton_ok:
            raise ValueError('algorithm newton needs 3 + n_changepoints + K <= 128')
        short = panel.lengths[members] < NEWTON_BELOW_T
        if algo == 'auto' and not newton_ok and short.any():
            print(f"Newton optimiser unavailable for this model (3 + n_changepoints + K = "
                  f"{3 + lbfgs.n_changepoints + lbfgs.K}, K = {lbfgs.K}, modes {sorted(modes)}): "
                  f"{int(short.sum())} series shorter than {NEWTON_BELOW_T} rows are fitted with L-BFGS")
        if algo == 'newton':
            first_newton, first_lbfgs = members, members[:0]
        elif algo == 'auto' and newton_ok:
            first_newton, first_lbfgs = members[short], members[~short]
        else:
            first_newton, first_lbfgs = members[:0], members
        if len(first_lbfgs):
            run(lbfgs, sd, seas, first_lbfgs)
            failed = first_lbfgs[np.isin(status[first_lbfgs], RUNTIME_ERROR_STATUS)]
            if len(failed) and newton_ok and algo == 'auto':
                run(newton, sd, seas, failed)
        if len(first_newton):
            run(newton, sd, seas, first_newton)
    return pieces, status, n_iter


class ModelBatch(object):
    """The rows of the fit UDF's output (prophet_modeler.py:68-79: series_id, dim_id, floor, cap, model) for a whole
    panel, before they become a frame: key and cap columns, and the model blobs as the buffers the library wrote them
    into (fit_packed's pieces).  to_frame(): the reference's frame, one bytes object per series; to_table(): the same
    rows as a pyarrow table over the same buffers -- what persist_models writes, with no Python object per series."""

    def __init__(self, sids, dids, floor, cap, pieces, status, n_iter):
        N = len(sids)
        self.sids, self.dids, self.floor, self.cap = sids, dids, floor, cap
        self.pieces, self.status, self.n_iter = pieces, status, n_iter
        self.piece_of = np.full(N, -1, dtype=np.int64)       # which piece holds the model of series n (-1: none)
        self.row_of = np.zeros(N, dtype=np.int64)
        for p, (mem, _buf) in enumerate(pieces):
            ok = np.flatnonzero(status[mem] >= 0)
            # (status is the FINAL status: a series that failed under L-BFGS and succeeded in the Newton retry takes the
            # later piece; one that failed in both has status < 0 and no model)
            self.piece_of[mem[ok]] = p
            self.row_of[mem[ok]] = ok
        self.keep = np.flatnonzero(self.piece_of >= 0)

    def __len__(self):
        return len(self.keep)

    @property
    def cost(self):
        return self.n_iter[self.keep]

    def to_frame(self):
        model = np.empty(len(self.sids), dtype=object)
        for p, (_mem, buf) in enumerate(self.pieces):
            sel = np.flatnonzero(self.piece_of == p)
            if len(sel) == 0:
                continue
            body, L = buf.tobytes(), buf.shape[1]
            rows = [body[r * L:(r + 1) * L] for r in self.row_of[sel].tolist()]
            model[sel] = np.array(rows + [None], dtype=object)[:-1]      # (an object array, never a 2-D char array)
        keep = self.keep
        out = pd.DataFrame({'series_id': self.sids[keep], 'dim_id': self.dids[keep],
                            'floor': np.full(len(keep), self.floor), 'cap': self.cap[keep],
                            'model': pd.Series(model[keep], dtype=object)}, columns=MODEL_OUTPUT_COLUMNS)
        # persist_models writes them beside the parquet (scheduling hints of the next run)
        out.attrs['tsf_cost'] = _CostVector(self.cost)
        return out

    def to_table(self):
        import pyarrow as pa
        keep = self.keep
        live = [p for p in range(len(self.pieces)) if (self.piece_of == p).any()]
        if len(live) == 1 and len(keep) == self.pieces[live[0]][1].shape[0] and \
                np.array_equal(self.row_of[keep], np.arange(len(keep))):
            model = pk.model_column_arrow(self.pieces[live[0]][1])          # the usual case: the buffer as it stands
        elif not live:
            model = pa.array([], type=pa.binary())
        else:
            cols, base, start = [], {}, 0
            for p in live:
                cols.append(pk.model_column_arrow(self.pieces[p][1]).cast(pa.large_binary()))
                base[p] = start
                start += self.pieces[p][1].shape[0]
            at = np.array([base[int(p)] for p in self.piece_of[keep]], dtype=np.int64) + self.row_of[keep]
            model = pa.concat_arrays(cols).take(pa.array(at)).cast(pa.binary())
        return pa.table({'series_id': pa.array(np.ascontiguousarray(self.sids[keep], dtype=np.int32)),
                         'dim_id': pa.array(np.ascontiguousarray(self.dids[keep], dtype=np.int32)),
                         'floor': pa.array(np.full(len(keep), self.floor, dtype=np.float32)),
                         'cap': pa.array(np.ascontiguousarray(self.cap[keep], dtype=np.float32)),
                         'model': model})


def _spec_opts(kw):
    out = {}
    for k in ('n_changepoints', 'changepoint_range', 'changepoint_prior_scale',
              'seasonality_prior_scale', 'holidays_prior_scale', 'max_iter', 'history',
              'init_alpha', 'tol_obj', 'tol_rel_obj', 'tol_grad', 'tol_rel_grad', 'tol_param'):
        if k in kw:
            out[k] = kw[k]
    # changepoints: a list of dates, fbprophet's Prophet(changepoints=[...]) -- the trend changes slope at these dates
    # instead of at n_changepoints automatic ones (ModelSpec); the reference job has no such key (it constructs Prophet
    # with the default, prophet_modeler.py:65)
    if kw.get('changepoints') is not None:
        out['changepoints'] = fc.changepoints_ns(kw['changepoints'])
    # converge: 'stan' (default: where Stan's termination tests stop the optimiser -- what Prophet.fit returns) or 'map'
    # (on to the maximum a posteriori estimate itself: include/tsf.h TSF_CONVERGE_MAP); not in the reference
    if 'converge' in kw:
        c = str(kw['converge']).lower()
        if c not in ('stan', 'map'):
            raise ValueError("converge must be 'stan' or 'map'")
        out['converge'] = _lib.CONVERGE_MAP if c == 'map' else _lib.CONVERGE_STAN
        for k in ('map_max_iter', 'map_tol'):
            if k in kw:
                out[k] = kw[k]
    return out


def check_changepoints(kw, panel):
    """fbprophet's set_changepoints raises for a model whose specified changepoints do not all lie inside its history;
    the fit reports such a series as ST_CHANGEPOINT, the jobs raise what fbprophet raises."""
    if kw.get('changepoints') is None or panel.N == 0:
        return
    cp = fc.changepoints_ns(kw['changepoints'])
    if len(cp) == 0:
        return
    first, last = panel.ds_ns[panel.offsets[:-1]], panel.ds_ns[panel.offsets[1:] - 1]
    if (cp[0] < first).any() or (cp[-1] > last).any():
        raise ValueError('Changepoints must fall within training data.')


def _model_packed(config, panel, n_rows, execution_time, previous=None, lap=None):
    """-> ModelBatch"""
    lap = lap or (lambda name: None)
    floor = config['model']['floor']                                   # :56-57
    ymax = pk.per_series_stats(panel)[2]
    cap = ymax * config['model']['cap_multiplier']                     # :59-60
    kw = _prophet_kwargs(config)
    floors = np.full(panel.N, float(floor))
    # ValueError cases propagate exactly as fbprophet's would (SURVEY 8b error convention);
    # a group whose every y is null never reaches the packed panel but fails the same way
    if panel.has_inf or (panel.has_inf is None and np.isinf(panel.y).any()):
        raise ValueError('Found infinity in column y.')
    if panel.dropped_keys or (panel.lengths < 2).any():
        raise ValueError('Dataframe has less than 2 non-NaN rows.')
    if kw['growth'] == 'logistic' and (cap <= floors).any():
        raise ValueError('cap must be greater than floor (which defaults to 0).')
    check_changepoints(kw, panel)
    # config['devices'] (not in the reference): GPUs to spread the series over, e.g. [0, 1, 2, 3]
    # or 'all'; default: TSF_DEVICES, else one GPU
    cost = None
    if previous is not None and len(previous):
        # series this run shares with the previous one get its iteration count, new series the median
        # (one sorted 64-bit key per (series_id, dim_id): a pandas merge of the two key frames costs more than the
        # hints save on a 10 000-series run)
        def key64(sid, did):
            return (np.asarray(sid).astype(np.int64) << 32) | (np.asarray(did).astype(np.int64) & 0xffffffff)
        pkey = key64(previous['series_id'].to_numpy(), previous['dim_id'].to_numpy())
        o = np.argsort(pkey, kind='stable')
        pkey, pcost = pkey[o], previous['cost'].to_numpy()[o]
        k = key64(panel.keys['series_id'].to_numpy(), panel.keys['dim_id'].to_numpy())
        at = np.minimum(np.searchsorted(pkey, k), len(pkey) - 1)
        cost = np.where(pkey[at] == k, pcost[at], int(np.median(pcost))).astype(np.int32)
    lap('checks + hints')
    screen = screen_settings(config)
    removed = {} if screen is not None else None
    noise = noise_settings(config)
    check_noise_io(config)
    noise_out = None if noise is None else {f: np.zeros(panel.N, _NOISE_DTYPES[f]) for f in NOISE_FIELDS}
    pieces, status, n_iter = fit_packed(panel, floors, cap, kw, devices=config.get('devices'), cost=cost, lap=lap,
                                        **({} if screen is None else {'screen': screen, 'removed': removed}),
                                        **({} if noise is None else {'noise': noise, 'noise_out': noise_out}))
    lap('fit_packed tail')
    sids = panel.keys['series_id'].to_numpy()
    dids = panel.keys['dim_id'].to_numpy()
    out = ModelBatch(sids, dids, floor, cap, pieces, status, n_iter)
    if removed is not None:
        out.screened = _screened_frame(sids, dids, removed)
    if noise is not None:
        out.noise = _noise_frame(sids, dids, out.keep, noise_out, pk.per_series_stats(panel)[1], panel.last_ds_all)
    for n in np.flatnonzero(out.piece_of < 0):
        # pystan RuntimeError -> the reference prints and drops the series (:81-85)
        print(f"Runtime error {_lib.STATUS_NAMES.get(int(status[n]), status[n])} for "
              f"series_id: {int(sids[n])}, dim_id: {int(dids[n])}")
    print(f"Modeled {panel.N} series ({n_rows} rows) in {time.time() - execution_time}")
    return out


def _screened_frame(sids, dids, removed):
    """The rows model.screen removed, one per row (SCREENED_COLUMNS), series in panel order, rows in time order."""
    if not removed:
        return _empty_screened()
    order = sorted(removed)
    n_rows = [len(removed[n][0]) for n in order]
    cat = lambda k: np.concatenate([np.asarray(removed[n][k]) for n in order])     # noqa: E731
    rep = lambda v: np.repeat(np.asarray(v), n_rows)                                # noqa: E731
    return pd.DataFrame({'series_id': rep(sids[order]).astype(np.int32), 'dim_id': rep(dids[order]).astype(np.int32),
                         'ds': cat(0).astype('datetime64[ns]'), 'y': cat(1).astype(np.float64), 'resid': cat(2),
                         'center': rep([removed[n][3] for n in order]), 'scale': rep([removed[n][4] for n in order])},
                        columns=SCREENED_COLUMNS)


def _noise_frame(sids, dids, keep, noise_out, min_dt, last_ds_all=None):
    """model.noise's table (NOISE_COLUMNS): one row per fitted series, in model order; row_step_ns is the series'
    smallest spacing (per_series_stats: -1 for a one-row series), what the scorer measures the forecast's lead in."""
    cols = {'series_id': np.asarray(sids)[keep].astype(np.int32), 'dim_id': np.asarray(dids)[keep].astype(np.int32)}
    cols.update((f, noise_out[f][keep]) for f in NOISE_FIELDS)
    step = np.asarray(min_dt, dtype=np.int64)[keep]
    if last_ds_all is not None:
        # The model's history ends at its last date INCLUDING rows whose y is null (fit_packed: last_ds), which the packed
        # panel does not hold: such trailing rows lie behind the last present row like any other absent row.  Where they
        # are whole steps they join last_gap; where not, the series has no row grid the chain could run on (row_step -1).
        tail = np.asarray(last_ds_all, dtype=np.int64)[keep] - cols['last_ds_ns']
        more = tail > 0
        whole = more & (step > 0) & (tail % np.where(step > 0, step, 1) == 0)
        cols['last_gap'] = np.where(whole, cols['last_gap'] + tail // np.where(step > 0, step, 1),
                                    cols['last_gap']).astype(np.int32)
        step = np.where(more & ~whole, -1, step)
        cols['last_ds_ns'] = np.where(more, cols['last_ds_ns'] + tail, cols['last_ds_ns'])
    cols['row_step_ns'] = step
    return pd.DataFrame(cols, columns=NOISE_COLUMNS)


def model_panel(config):
    """Batched form of model_time_series: the frame may hold any number of
    (series_id, dim_id) groups; one output row per fitted group."""

    def model_panel_fn(pdf):
        execution_time = time.time()
        if len(pdf.index) == 0:
            return _empty_models()
        return _model_packed(config, pk.pack_long_frame(pdf), len(pdf.index), execution_time).to_frame()

    return model_panel_fn


def model_arrays(config, previous=None, batch=False):
    """model_panel for columns that never were a DataFrame (what read_model_input returns):
    series_id, dim_id int64; ds_ns int64 ns; y float64 with NaN for nulls.
    previous: previous_run_cost(...) of an earlier run, or None.
    batch: return the ModelBatch (the blobs in the library's buffers: persist_models writes it to parquet without a
    Python object per series) instead of the reference's frame."""

    def model_arrays_fn(sid, did, ds_ns, y):
        from ..pipeline import Laps
        execution_time = time.time()
        if len(y) == 0:
            return None if batch else _empty_models()
        with Laps('model_arrays %d rows' % len(y)) as lap:
            # (an infinite y raises in _model_packed: the packer's own pass over the rows reports it, tsf_pack_flags)
            panel = pk.pack_rows(sid, did, ds_ns, y, key_dtypes=(np.int32, np.int32))
            lap('pack_rows')
            out = _model_packed(config, panel, len(y), execution_time, previous=previous, lap=lap)
            lap('rest')
            return out if batch else out.to_frame()

    return model_arrays_fn


def model_time_series(config):
    """Model time series per dimensions (series_id, dim_id) -- prophet_modeler.py:22.
    Returns the grouped-map function `pdf -> pdf`; the frame of one group gives one row
    [series_id, dim_id, floor, cap, model]."""
    batched = model_panel(config)

    def model_time_series_udf(pdf):
        series_id = int(pdf.iloc[0]['series_id'])
        dim_id = int(pdf.iloc[0]['dim_id'])
        print(f"Modeling series_id: {series_id}, dim_id: {dim_id}"
              f" with {len(pdf.index)} modeling rows")
        return batched(pdf)

    return model_time_series_udf


def as_pandas_udf(fn, columns=MODEL_OUTPUT_COLUMNS):
    """Wrap a `pdf -> pdf` function as a GROUPED_MAP pandas_udf with the reference's output
    schema (prophet_modeler.py:32-40).  Only where pyspark exists."""
    from pyspark.sql.functions import pandas_udf, PandasUDFType
    from pyspark.sql.types import (BinaryType, FloatType, IntegerType, StructField, StructType,
                                   TimestampType)
    types = {'series_id': IntegerType(), 'dim_id': IntegerType(), 'floor': FloatType(),
             'cap': FloatType(), 'model': BinaryType(), 'ds': TimestampType(), 'yhat': IntegerType()}
    schema = StructType([StructField(c, types[c], True) for c in columns])
    return pandas_udf(schema, PandasUDFType.GROUPED_MAP)(fn)


# codecs spark.read.csv would decompress and the native reader does not (.gz and .deflate it inflates itself: zlib)
_COMPRESSED = ('.bz2', '.snappy', '.lz4', '.zst', '.xz')


def find_model_input(root):
    """Data files under `root` with the series_id of the `series_id=<v>` directory above them
    (None if there is none), ordered by (series_id, path): partition directories in numeric
    order hand the packer a table that is already grouped.  As `spark.read.csv(path)` does, every
    non-hidden file counts (names starting with `_` or `.` -- `_SUCCESS`, `.part-0.crc` -- are
    skipped).  `.gz` / `.deflate` parts are read (the native reader inflates them, as Spark's Hadoop codecs
    do transparently); a file in another codec raises (Spark would decompress it; this reader does not)."""
    if os.path.isfile(root):
        return [root], [None]
    found = []

    def walk(d, sid):
        with os.scandir(d) as it:
            entries = sorted(it, key=lambda e: e.name)
        for e in entries:
            if e.is_dir(follow_symlinks=True):
                if e.name.startswith(('_', '.')):
                    continue
                v = sid
                if e.name.startswith('series_id='):
                    v = int(e.name.split('=', 1)[1])
                walk(e.path, v)
            elif e.name.startswith(('_', '.')):
                continue
            elif e.name.endswith(_COMPRESSED):
                raise ValueError('compressed input file %s: decompress it first (Spark reads it, '
                                 'this reader does not)' % e.path)
            else:
                found.append((sid, e.path))

    if os.path.isdir(root):
        walk(root, None)
    found.sort(key=lambda t: ((0, t[0]) if t[0] is not None else (1, 0), t[1]))
    return [f for _, f in found], [v for v, _ in found]


class _CsvTable:
    """Owns one native table (tsf_csv handle); the numpy columns handed out view its memory and keep it alive
    through their .base chain -- no copy of the 32 bytes per row into arrays of Python's own."""

    def __init__(self, handle, n_rows):
        self.handle, self.n_rows = handle, int(n_rows)

    def __del__(self):
        if self.handle:
            _lib.load().tsf_csv_free(self.handle)
            self.handle = None

    def columns(self):
        import ctypes
        L = _lib.load()
        ptrs = [ctypes.c_void_p() for _ in range(4)]
        if L.tsf_csv_columns(self.handle, *[ctypes.byref(p) for p in ptrs]) != 0:
            raise _lib.TsfError('tsf_csv_columns failed')
        out = []
        for p, dt in zip(ptrs, (np.int64, np.int64, np.int64, np.float64)):
            if self.n_rows == 0:
                out.append(np.zeros(0, dt))
                continue
            buf = (ctypes.c_char * (8 * self.n_rows)).from_address(p.value)
            buf._owner = self                   # the ctypes view keeps the table; the array keeps the view
            arr = np.frombuffer(buf, dtype=dt)
            arr.setflags(write=False)           # views of the native table: read-only, as documented (round-4 advice)
            out.append(arr)
        return tuple(out)


def _csv_read_call(n, paths_ptr, sids_ptr, layout, n_threads, name_of, stats, loaded=None):
    """One tsf_csv_read; returns the four columns as views of the native table.  name_of(i): path of file i.
    loaded = (dir handle, first): the files were read during the walk (tsf_csv_discover_load)."""
    import ctypes
    L = _lib.load()
    h, n_rows = ctypes.c_void_p(), ctypes.c_int64()
    ef, el = ctypes.c_int32(-1), ctypes.c_int64(0)
    if loaded is not None:
        rc = L.tsf_csv_read_loaded(loaded[0], int(loaded[1]), n, layout, int(n_threads), ctypes.byref(h),
                                   ctypes.byref(n_rows), ctypes.byref(ef), ctypes.byref(el))
    else:
        rc = L.tsf_csv_read(n, paths_ptr, sids_ptr, layout, int(n_threads), ctypes.byref(h),
                            ctypes.byref(n_rows), ctypes.byref(ef), ctypes.byref(el))
    if rc == _lib.CSV_E_OPEN:
        raise OSError(('corrupt or truncated compressed stream in %s' if el.value == -1 else 'cannot read %s')
                      % name_of(ef.value))
    if rc == _lib.CSV_E_PARSE:
        raise ValueError('%s line %d does not match the model-input schema %s'
                         % (name_of(ef.value), el.value, layout.decode()))
    if rc != 0:
        raise _lib.TsfError('tsf_csv_read failed (%d)' % rc)
    tab = _CsvTable(h, n_rows.value)
    if stats is not None:
        stats['malformed'] = stats.get('malformed', 0) + int(L.tsf_csv_malformed(h))
    return tab.columns()


def _layouts(mode):
    if mode not in ('FAILFAST', 'PERMISSIVE'):
        raise ValueError("mode must be 'FAILFAST' or 'PERMISSIVE'")
    q = b'?' if mode == 'PERMISSIVE' else b''
    return b'dtq' + q, b'sdtq' + q          # files under a partition directory hold 3 columns, the others all 4


def read_model_input(files, root, n_threads=0, part_sid=None, mode='FAILFAST', stats=None):
    """Parse model-input CSV files into (series_id, dim_id, ds_ns, y) arrays (int64, int64,
    int64 ns, float64 with NaN for nulls).  mode: 'FAILFAST' (a line that does not match the schema
    raises, naming file and line) or 'PERMISSIVE' (spark.read.csv's default at prophet_modeler.py:109:
    such a line becomes a row of nulls there -- dim_id included --, whose null y the fit would drop; the
    reader drops the record itself, it never appears under a made-up key; stats['malformed'] counts them).
    A `series_id=<v>` directory between `root` and the
    file supplies series_id for that file (Spark's partition discovery); the file then holds
    the remaining MODEL_INPUT_SCHEMA columns in order.  part_sid: the partition values if the
    caller knows them already (find_model_input).  The arrays are read-only views of the native table."""
    import ctypes
    if not files:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy(), np.zeros(0)
    known = part_sid is not None
    part_sid = list(part_sid) if known else []
    for f in ([] if known else files):
        v = None
        rel = os.path.relpath(os.path.dirname(os.path.abspath(f)),
                              os.path.abspath(root if os.path.isdir(root) else os.path.dirname(root)))
        for seg in rel.split(os.sep):
            if seg.startswith('series_id='):
                v = int(seg.split('=', 1)[1])
        part_sid.append(v)
    out = []
    lay_part, lay_all = _layouts(mode)
    for layout, pick in ((lay_part, [i for i, v in enumerate(part_sid) if v is not None]),
                         (lay_all, [i for i, v in enumerate(part_sid) if v is None])):
        if not pick:
            continue
        paths = (ctypes.c_char_p * len(pick))(*[os.fsencode(files[i]) for i in pick])
        sids = np.array([part_sid[i] if part_sid[i] is not None else 0 for i in pick], dtype=np.int64)
        out.append(_csv_read_call(len(pick), paths, sids.ctypes.data, layout, n_threads,
                                  lambda i, pick=pick: files[pick[i]], stats))
    if len(out) == 1:
        return out[0]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


def read_model_input_dir(root, n_threads=0, mode='FAILFAST', stats=None):
    """find_model_input + read_model_input in one go, natively: the directory walk (tsf_csv_discover: Spark's
    file-listing and partition-discovery rules, the directories read by a pool of threads) hands its path list
    straight to the reader, so no path becomes a Python object unless an error names it.  Same rows, same order,
    same errors as read_model_input(*find_model_input(root))."""
    import ctypes
    L = _lib.load()
    lay_part, lay_all = _layouts(mode)
    d, n, n_part = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32()
    # (the thread that lists a directory reads its files at once: tsf_csv_discover_load)
    rc = L.tsf_csv_discover_load(os.fsencode(root), int(n_threads), ctypes.byref(d), ctypes.byref(n), ctypes.byref(n_part))
    try:
        _raise_discover_error(rc, d)
        if n.value == 0:
            z = np.zeros(0, np.int64)
            return z, z.copy(), z.copy(), np.zeros(0)
        paths, sids = L.tsf_csv_dir_paths(d), L.tsf_csv_dir_series_id(d)
        pp = ctypes.cast(paths, ctypes.POINTER(ctypes.c_char_p))
        out = []
        for layout, lo, hi in ((lay_part, 0, n_part.value), (lay_all, n_part.value, n.value)):
            if hi > lo:
                out.append(_csv_read_call(hi - lo, paths + 8 * lo, sids + 8 * lo, layout, n_threads,
                                          lambda i, lo=lo: os.fsdecode(pp[lo + i]), stats, loaded=(d, lo)))
    finally:
        if d:
            L.tsf_csv_dir_free(d)
    if len(out) == 1:
        return out[0]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


class _CsvRoot:
    """tsf_csv_root_open / _load (include/tsf.h): the input directory's children, read in ranges."""

    def __init__(self, root):
        import ctypes
        L = _lib.load()
        self.handle, n, hive = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32()
        rc = L.tsf_csv_root_open(os.fsencode(root), ctypes.byref(self.handle), ctypes.byref(n), ctypes.byref(hive))
        if rc == _lib.CSV_E_OPEN:
            raise OSError('cannot list %s' % root)
        if rc != 0:
            raise _lib.TsfError('tsf_csv_root_open failed (%d)' % rc)
        self.n_children, self.hive_only = n.value, bool(hive.value)

    def close(self):
        if self.handle:
            _lib.load().tsf_csv_root_free(self.handle)
            self.handle = None

    __del__ = close

    def read(self, first, count, mode='FAILFAST', stats=None, n_threads=0):
        """The rows of children [first, first + count) as (series_id, dim_id, ds_ns, y) -- read_model_input_dir over that
        range.  Raises _Nested when a `series_id=` directory sits below another one (the caller reads the tree whole)."""
        import ctypes
        L = _lib.load()
        lay_part, lay_all = _layouts(mode)
        d, n, n_part, nested = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        rc = L.tsf_csv_root_load(self.handle, int(first), int(count), int(n_threads), ctypes.byref(d), ctypes.byref(n),
                                 ctypes.byref(n_part), ctypes.byref(nested))
        try:
            _raise_discover_error(rc, d)
            if nested.value:
                raise _Nested()
            if n.value == 0:
                z = np.zeros(0, np.int64)
                return z, z.copy(), z.copy(), np.zeros(0)
            paths, sids = L.tsf_csv_dir_paths(d), L.tsf_csv_dir_series_id(d)
            pp = ctypes.cast(paths, ctypes.POINTER(ctypes.c_char_p))
            out = []
            for layout, lo, hi in ((lay_part, 0, n_part.value), (lay_all, n_part.value, n.value)):
                if hi > lo:
                    out.append(_csv_read_call(hi - lo, paths + 8 * lo, sids + 8 * lo, layout, n_threads,
                                              lambda i, lo=lo: os.fsdecode(pp[lo + i]), stats, loaded=(d, lo)))
        finally:
            if d:
                L.tsf_csv_dir_free(d)
        if len(out) == 1:
            return out[0]
        return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


class _Nested(Exception):
    pass


def _raise_discover_error(rc, d):
    L = _lib.load()
    if rc in (_lib.CSV_E_OPEN, _lib.CSV_E_PARSE, _lib.CSV_E_CODEC):
        bad = os.fsdecode(L.tsf_csv_dir_error_path(d))
        if rc == _lib.CSV_E_CODEC:
            raise ValueError('compressed input file %s: decompress it first (Spark reads it, '
                             'this reader does not)' % bad)
        if rc == _lib.CSV_E_PARSE:
            raise ValueError('partition directory %s: series_id is not an integer' % bad)
        raise OSError('cannot list %s' % bad)
    if rc != 0:
        raise _lib.TsfError('tsf_csv_discover failed (%d)' % rc)


# A run over this many partition directories or more is read, fitted and persisted in chunks, as a pipeline
# (ProphetModeler.model); config['io']['chunks'] overrides ('auto', or a number; 1 = the whole input at once).
# Measured on the GPU box (profiles/r06_host/): 10 000 x 730 rows take 58 ms whole and 63 ms in four chunks (every chunk
# pays its walk, its launch -- which lasts as long as its longest fit -- and its Python), 40 000 take 357 ms whole and
# 248 ms in chunks (the chunks' file and table blocks fit the process's block cache and are read into again and again).
PIPELINE_MIN_CHILDREN = 16384
PIPELINE_CHUNK_CHILDREN = 4096
PIPELINE_MAX_CHUNKS = 32


class ProphetModeler:
    """Create models to forecast quantities (prophet_modeler.py:90-143), Spark-free: the frames
    are pandas, the IO is pyarrow/pandas, the fit is one batched GPU call."""

    def __init__(self, config, logger=None):
        self.logger = logger or logging.getLogger(self.__class__.__name__)
        self.config = config

    def read_input_dataframe(self, spark=None):
        """Header-less CSV files under config['io']['input'], Hive-style partition directories
        (`series_id=751/…csv` supplies the series_id column), schema MODEL_INPUT_SCHEMA;
        renames start_time -> ds, quantity -> y (:109-114).  The files are parsed by the native
        reader (tsf_csv_read, include/tsf.h), in parallel, straight into columns."""
        sid, did, ds_ns, y = self.read_input_columns()
        for name, col in (('series_id', sid), ('dim_id', did)):
            if len(col) and (col.min() < -2 ** 31 or col.max() >= 2 ** 31):
                raise ValueError('%s does not fit the int32 column of MODEL_INPUT_SCHEMA' % name)
        yq = y
        if not np.isnan(y).any():
            if len(y) and ((y != np.rint(y)).any() or np.abs(y).max() >= 2 ** 31):
                raise ValueError('quantity is not an int32 column (MODEL_INPUT_SCHEMA)')
            yq = y.astype('int32')                       # nulls keep the column float64
        return pd.DataFrame({'series_id': sid.astype('int32'), 'dim_id': did.astype('int32'),
                             'ds': ds_ns.astype('datetime64[ns]'), 'y': yq},
                            columns=['series_id', 'dim_id', 'ds', 'y'])

    def read_input_columns(self):
        """The same rows as read_input_dataframe, as (series_id, dim_id, ds_ns, y) arrays."""
        root = self.config['io']['input']
        # io.input_mode: 'FAILFAST' (default here: a malformed line raises with file and line) or
        # 'PERMISSIVE' (what spark.read.csv does by default, prophet_modeler.py:109: the line becomes a
        # row of nulls there; here the reader drops the record and counts it)
        mode = str(self.config['io'].get('input_mode', 'FAILFAST')).upper()
        stats = {}
        cols = read_model_input_dir(root, mode=mode, stats=stats)
        if stats.get('malformed'):
            self.logger.warning('%d malformed model-input records dropped (PERMISSIVE)', stats['malformed'])
        return cols

    def persist_models(self, model_df):
        """Parquet, mode='overwrite' (:123-125).  model_df: the reference's model frame, or a ModelBatch (model_arrays(...,
        batch=True)), whose blobs go to the file from the buffers the library wrote them into."""
        wait = self._clear_models()
        part = self._write_part(0, model_df)
        wait()
        if isinstance(model_df, ModelBatch):
            keep = model_df.keep
            _write_cost_sidecar(self.config['io']['models'], [part], model_df.sids[keep], model_df.dids[keep], model_df.cost)
        else:
            _write_cost_sidecar(self.config['io']['models'], [part], model_df['series_id'].to_numpy(),
                                model_df['dim_id'].to_numpy(), model_df.attrs.get('tsf_cost'))

    def persist_screened(self, batches):
        """config['io']['screened'] (optional, with model.screen): the rows the screening removed, as one parquet part
        in that directory (SCREENED_COLUMNS), mode='overwrite' like the models."""
        path = self.config['io'].get('screened')
        if not path:
            return
        if screen_settings(self.config) is None:
            raise ValueError('io.screened needs model.screen')
        frames = [b.screened for b in batches if b is not None and getattr(b, 'screened', None) is not None]
        out = pd.concat(frames, ignore_index=True) if frames else _empty_screened()
        os.makedirs(path, exist_ok=True)
        for f in os.listdir(path):
            if f.endswith('.parquet'):
                os.remove(os.path.join(path, f))
        out.to_parquet(os.path.join(path, 'part-00000.parquet'), index=False)

    def persist_noise(self, batches):
        """config['io']['noise'] (optional, with model.noise): the fits' AR(1) noise state, one row per model
        (NOISE_COLUMNS), as one parquet part in that directory, mode='overwrite' like the models -- what the scorer's
        forecast.noise.table reads."""
        path = self.config['io'].get('noise')
        if not path:
            return
        check_noise_io(self.config)
        frames = [b.noise for b in batches if b is not None and getattr(b, 'noise', None) is not None]
        out = pd.concat(frames, ignore_index=True) if frames else _empty_noise()
        os.makedirs(path, exist_ok=True)
        for f in os.listdir(path):
            if f.endswith('.parquet'):
                os.remove(os.path.join(path, f))
        out.to_parquet(os.path.join(path, 'part-00000.parquet'), index=False)

    def _clear_models(self):
        """-> function that waits until the previous run's files are gone (pipeline.clear_directory)"""
        from ..pipeline import clear_directory
        return clear_directory(self.config['io']['models'])

    def _write_part(self, k, model_df):
        """part-<k>.parquet of the model directory (Spark writes one part per task: a directory of parts is what
        spark.read.parquet / pd.read_parquet read back, prophet_scorer.py:124-126)."""
        import pyarrow as pa
        import pyarrow.parquet as pq
        part = 'part-%05d.parquet' % k
        if isinstance(model_df, ModelBatch):
            table = model_df.to_table()
        else:
            out = model_df.copy()
            out.attrs = {}                          # (pandas would try to store them in the parquet metadata as JSON)
            for c, t in MODEL_OUTPUT_DTYPES.items():
                out[c] = out[c].astype(t)
            table = pa.Table.from_pandas(out, preserve_index=False)
        # blobs of ~1 KB that share a few hundred prefix bytes: the default page compression (snappy) is what shrinks
        # them; dictionary encoding of the binary column only costs time (every blob is distinct)
        n = table.num_rows
        groups = max(1, -(-n // MODEL_ROW_GROUP))
        # (no min / max statistics for the blobs: nobody filters on them, and computing them compares 1 KB strings)
        pq.write_table(table, os.path.join(self.config['io']['models'], part), use_dictionary=False,
                       row_group_size=max(1, -(-n // groups)), write_statistics=['series_id', 'dim_id'])
        return part

    def _chunk_plan(self):
        """(root handle, [(first, count), ...]) when the input is read in chunks, else None: a directory whose children
        are all `series_id=<int>` partition directories (tsf_csv_root_open: ranges of them hold disjoint series), enough
        of them, and io.chunks not 1."""
        root = self.config['io']['input']
        want = self.config['io'].get('chunks', 'auto')
        if want == 1 or not os.path.isdir(root):
            return None
        r = _CsvRoot(root)
        n = r.n_children
        if not r.hive_only or n < 2:
            r.close()
            return None
        if want == 'auto':
            if n < PIPELINE_MIN_CHILDREN:
                k = 1           # one "chunk": the children just listed are read as they are (no second walk of the root)
            else:
                k = min(PIPELINE_MAX_CHUNKS, max(2, n // PIPELINE_CHUNK_CHILDREN))
        else:
            k = max(1, min(int(want), n))
        cuts = [(n * i) // k for i in range(k + 1)]
        return r, [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]

    @staticmethod
    def model(spark_session, config, return_frame=True):
        """Create the trained time series models (:127-143).  spark_session is accepted for
        signature compatibility and may be None.  return_frame=False: return nothing, as the reference's does (the
        drivers; a chunked run then never builds the frame)."""
        scorer = ProphetModeler(config)
        check_noise_io(config)              # (before anything is read or overwritten)
        # A re-run overwrites io.models (:123-125).  Before it does, what the previous run left there gives this run
        # its scheduling hints: the iteration count of every model, the one cheap predictor of how long each fit takes,
        # so that the launches start their longest fits first (the reference's model on 100 000 series: 1.00 -> 0.84 s
        # of fit; cfg2 on 10 000: 9.1 -> 7.3 ms).  Results do not depend on it.
        # config['model']['schedule_from_previous_models'] (not in the reference): 'auto' (default) -- only when
        # persist_models' own side file is there (_tsf_cost.npz, ~1 ms for 10 000 series); true -- else parse the model
        # blobs (17 ms per 10 000: pays from ~100 000 series of the reference's model on); false -- never.
        previous = None
        how = (config.get('model') or {}).get('schedule_from_previous_models', 'auto')
        if how:
            previous = previous_run_cost(config['io']['models'], sidecar_only=(how == 'auto'))
        # Round 6: a Hive-partitioned input of a few thousand partition directories or more runs as a pipeline over ranges
        # of them (time_series_spark_amd/pipeline.py): the files of chunk k + 1 are read and parsed while chunk k is packed
        # and fitted on the GPU and the models of chunk k - 1 go to their parquet part -- Spark's answer to the same problem
        # is many tasks at once (:139-141).  Every series lies in one partition directory, so it is fitted once, on all of
        # its rows, whatever the chunking; one part file per chunk, as Spark writes one per task.
        fit = model_arrays(scorer.config, previous=previous, batch=True)
        plan = scorer._chunk_plan()
        if plan is not None:
            try:
                return scorer._model_chunked(plan, fit, return_frame)
            except _Nested:
                pass            # a partition directory below another one: the tree is read whole
            finally:
                plan[0].close()
        # the columns go from the reader to the packer as arrays; read_input_dataframe gives the
        # same rows as a frame for callers that want one
        batch = fit(*scorer.read_input_columns())
        scorer.persist_screened([batch])
        scorer.persist_noise([batch])
        if batch is None:
            scorer.persist_models(_empty_models())
            return _empty_models() if return_frame else None
        scorer.persist_models(batch)
        return batch.to_frame() if return_frame else None

    def _model_chunked(self, plan, fit, return_frame):
        from .. import pipeline
        root, ranges = plan
        mode = str(self.config['io'].get('input_mode', 'FAILFAST')).upper()
        stats = {}

        def chunks():
            for k, (first, count) in enumerate(ranges):
                yield k, root.read(first, count, mode=mode, stats=stats)

        cleared = []

        def persist(item):
            k, batch = item
            if not cleared:                 # mode='overwrite' (:123-125): the old directory goes when the first part is ready
                cleared.append(self._clear_models())        # (its models were this run's scheduling hints until now)
            return k, batch, (self._write_part(k, batch) if batch is not None and len(batch) else None)

        try:
            done = pipeline.run_pipeline(chunks(), [lambda it: (it[0], fit(*it[1])), persist])
        finally:
            for wait in cleared:
                wait()
        if stats.get('malformed'):
            self.logger.warning('%d malformed model-input records dropped (PERMISSIVE)', stats['malformed'])
        if not cleared:
            self._clear_models()()
        self.persist_screened([b for _k, b, _part in done])
        self.persist_noise([b for _k, b, _part in done])
        live = [(b, part) for _k, b, part in done if part is not None]
        if live:
            _write_cost_sidecar(self.config['io']['models'], [part for _b, part in live],
                                np.concatenate([b.sids[b.keep] for b, _p in live]),
                                np.concatenate([b.dids[b.keep] for b, _p in live]),
                                np.concatenate([b.cost for b, _p in live]))
        if not return_frame:
            return None
        frames = [b.to_frame() for b, _p in live]
        if not frames:
            return _empty_models()
        out = pd.concat(frames, ignore_index=True)
        out.attrs['tsf_cost'] = _CostVector(np.concatenate([b.cost for b, _p in live]))
        return out
