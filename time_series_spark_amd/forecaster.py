"""Batched panel API over the C-ABI: fit_aligned / fit_ragged / predict on numpy arrays.

Stands where the reference calls fbprophet one series at a time
(/root/reference/src/jobs/prophet_modeler.py:65-66, /root/reference/src/jobs/prophet_scorer.py:70)
but takes the whole (series x timestamp x y) panel in one call.  The model options mirror
fbprophet 0.5's ``Prophet.__init__`` / ``set_auto_seasonalities`` (spec in SURVEY.md 8a
U1-U5); the arithmetic runs in libtsf_amd.so on the GPU -- this module only packs arrays.
"""
import ctypes
import os

import numpy as np

from . import _lib, parallel

DAY_NS = 86400 * 10 ** 9


class ModelSpec(object):
    """Model + optimiser settings shared by all series of a call.

    seasonalities: list of dicts {name, period (days), fourier_order, prior_scale, mode}.
    extra: list of dicts {name, prior_scale, mode} for explicit design columns (holiday
    indicators, regressors) whose values the caller supplies.
    changepoints: fbprophet's ``Prophet(changepoints=[...])`` -- the dates at which the trend may change slope, instead
    of ``n_changepoints`` row timestamps spread over the first ``changepoint_range`` of the history.  Anything
    ``numpy.asarray(..., 'datetime64[ns]')`` accepts, or int64 ns since the epoch.  The list is sorted, a date given twice
    is a ValueError (fbprophet would fit two identical trend columns), ``n_changepoints`` becomes its length and
    ``changepoint_range`` is ignored.  A series whose history does not span every date comes back with status
    ST_CHANGEPOINT.  (Semantics restated from recall of fbprophet 0.5: include/tsf.h.)
    A seasonality dict may carry ``condition_name`` -- fbprophet's ``add_seasonality(..., condition_name=...)``: the
    seasonality applies only on the rows where the boolean condition of that name is true.  Such seasonalities are kept
    in ``conditional`` (not in ``seasonalities``) and lowered to ``2 * fourier_order`` explicit columns at the end of
    ``extra`` (include/tsf.h "conditional seasonalities"; fbprophet keeps them among the seasonal columns instead: same
    posterior, another column order); ``conditional_extra`` builds the values of all of ``extra`` for any entry point.
    conditions: optional {condition name: date rule} -- a dict with any of ``weekdays`` (Monday = 0), ``months``
    (1..12), ``ranges`` ([start, end) dates) and ``negate``, combined by AND (features.condition_mask) -- for conditions
    that are functions of the date: they need no array and travel with the model (to_dict / the model blobs).
    """

    def __init__(self, growth='linear', seasonality_mode='additive', n_changepoints=25,
                 changepoint_range=0.8, changepoint_prior_scale=0.05,
                 seasonality_prior_scale=10.0, holidays_prior_scale=10.0,
                 seasonalities=None, extra=None, holidays=None, changepoints=None, conditions=None, **lbfgs):
        if growth not in ('linear', 'logistic'):
            raise ValueError("Parameter 'growth' should be 'linear' or 'logistic'.")
        if seasonality_mode not in ('additive', 'multiplicative'):
            raise ValueError("seasonality_mode must be 'additive' or 'multiplicative'")
        if changepoint_range < 0 or changepoint_range > 1:
            raise ValueError("Parameter 'changepoint_range' must be in [0, 1]")
        self.growth = growth
        self.seasonality_mode = seasonality_mode
        self.changepoints = None if changepoints is None else changepoints_ns(changepoints)
        self.n_changepoints = int(n_changepoints) if self.changepoints is None else len(self.changepoints)
        self.changepoint_range = float(changepoint_range)
        self.changepoint_prior_scale = float(changepoint_prior_scale)
        self.seasonality_prior_scale = float(seasonality_prior_scale)
        self.holidays_prior_scale = float(holidays_prior_scale)
        given = [dict(s) for s in (seasonalities or [])]
        self.seasonalities = [s for s in given if s.get('condition_name') is None]
        self.extra = [dict(e) for e in (extra or [])]
        # conditional seasonalities (condition_name): out of `seasonalities`, lowered to explicit columns behind the
        # caller's own (_lower_conditional); _given_conditional: which entries of the original list they were
        self.conditional = [s for s in given if s.get('condition_name') is not None]
        self._given_conditional = [s.get('condition_name') is not None for s in given]
        self.conditions = {}
        if conditions:
            from . import features
            self.conditions = {str(k): features.normalize_condition_rule(v) for k, v in dict(conditions).items()}
        # normalised holidays (features.normalize_holidays) whose indicator columns are the FIRST
        # len(features.holiday_columns(holidays)[0]) entries of `extra`: carried so that the scorer
        # can rebuild the columns for future dates (fbprophet keeps the holidays frame in the model)
        self.holidays = list(holidays) if holidays else None
        self.lbfgs = dict(lbfgs)
        for k in self.lbfgs:
            if k not in ('max_iter', 'history', 'init_alpha', 'tol_obj', 'tol_rel_obj',
                         'tol_grad', 'tol_rel_grad', 'tol_param', 'eval_form', 'recenter_every',
                         'recenter_ratio', 'algorithm', 'residual_kernel', 'coop_after', 'converge', 'map_max_iter', 'map_tol'):
                raise TypeError('unknown optimiser option %r' % k)
        if self.conditional:
            self._lower_conditional()

    def _lower_conditional(self):
        """Every conditional seasonality becomes 2 * fourier_order entries at the end of `extra` -- behind the holiday
        columns, which stay first, and the caller's regressors --, named '<seasonality>_delim_<j>' (j = 1 .. 2 * order:
        sin 1, cos 1, sin 2, ...), with the SEASONALITY's prior scale and mode (its own, else seasonality_prior_scale /
        seasonality_mode -- not holidays_prior_scale, the default of other extra columns) and a 'seasonality' key that
        names it: component_columns gathers the columns under that name.  fbprophet's validate_column_name, restated,
        on the seasonality's name and on condition_name: no '_delim_', no reserved name, no name used twice."""
        from . import features
        hol = {str(h['holiday']) for h in features.normalize_holidays(self.holidays)} if self.holidays else set()
        reg = {str(e.get('name')) for e in self.extra}
        seas = [str(s.get('name')) for s in self.seasonalities + self.conditional]

        def check(name, own_seasonality=False):
            if '_delim_' in name:
                raise ValueError('Name cannot contain "_delim_"')
            if name in features.RESERVED_NAMES and not (own_seasonality and name in ('daily', 'weekly', 'yearly')):
                raise ValueError('Name "{}" is reserved.'.format(name))
            if name in hol:
                raise ValueError('Name "{}" already used for a holiday.'.format(name))
            if seas.count(name) > int(own_seasonality):
                raise ValueError('Name "{}" already used for a seasonality.'.format(name))
            if name in reg:
                raise ValueError('Name "{}" already used for an added regressor.'.format(name))

        for s in self.conditional:
            if s.get('name') is None:
                raise ValueError('a conditional seasonality needs a name')
            # (a user seasonality may be called 'weekly': it then stands in for the automatic one, auto_from_stats)
            check(str(s['name']), own_seasonality=True)
            if not isinstance(s['condition_name'], str):
                raise ValueError('condition_name must be a string')
            check(s['condition_name'])
            order, period = int(s['fourier_order']), float(s['period'])
            if order < 1:
                raise ValueError('Fourier Order must be > 0')
            if not (np.isfinite(period) and period > 0):
                raise ValueError('period must be finite and > 0')
            scale = float(s.get('prior_scale', self.seasonality_prior_scale))
            if not scale > 0:
                raise ValueError('Prior scale must be > 0')
            mode = s.get('mode', self.seasonality_mode)
            if mode not in ('additive', 'multiplicative'):
                raise ValueError("mode must be 'additive' or 'multiplicative'")
            for j in range(2 * order):
                self.extra.append({'name': '%s_delim_%d' % (s['name'], j + 1), 'prior_scale': scale, 'mode': mode,
                                   'seasonality': str(s['name'])})

    @property
    def n_user_extra(self):
        """The extra columns whose values the caller supplies: all but the lowered conditional seasonalities'."""
        return sum(1 for e in self.extra if 'seasonality' not in e)

    # -- fbprophet set_auto_seasonalities on a timestamp vector --------------------------------
    @staticmethod
    def auto_seasonalities(ds_ns, yearly='auto', weekly='auto', daily='auto',
                           seasonality_mode='additive', seasonality_prior_scale=10.0,
                           user_seasonalities=()):
        """Returns the seasonality list fbprophet 0.5 would build for history timestamps
        ``ds_ns`` (int64 ns, sorted): yearly (365.25 d, order 10) off when span < 730 d;
        weekly (7 d, order 3) off when span < 14 d or the smallest non-zero spacing >= 7 d;
        daily (1 d, order 4) off when span < 2 d or the smallest spacing >= 1 d."""
        ds_ns = np.asarray(ds_ns, dtype=np.int64)
        first, last = int(ds_ns.min()), int(ds_ns.max())
        diffs = np.diff(np.sort(ds_ns))
        nz = diffs[diffs != 0]
        min_dt = int(nz.min()) if nz.size else -1
        return ModelSpec.auto_from_stats(last - first, min_dt, yearly, weekly, daily,
                                         seasonality_mode, seasonality_prior_scale,
                                         user_seasonalities)

    @staticmethod
    def auto_from_stats(span, min_dt, yearly='auto', weekly='auto', daily='auto',
                        seasonality_mode='additive', seasonality_prior_scale=10.0,
                        user_seasonalities=()):
        """Same rules from (span_ns, smallest non-zero spacing in ns or -1 if none)."""
        names = {s['name'] for s in user_seasonalities}

        def order(name, arg, auto_disable, default):
            if isinstance(arg, str) and arg == 'auto':
                if name in names or auto_disable:
                    return 0
                return default
            if arg is True:
                return default
            if arg is False:
                return 0
            return int(arg)

        out = [dict(s) for s in user_seasonalities]
        has_dt = min_dt is not None and min_dt >= 0
        fo = order('yearly', yearly, span < 730 * DAY_NS, 10)
        if fo > 0:
            out.append({'name': 'yearly', 'period': 365.25, 'fourier_order': fo,
                        'prior_scale': seasonality_prior_scale, 'mode': seasonality_mode})
        fo = order('weekly', weekly, (span < 14 * DAY_NS) or (has_dt and min_dt >= 7 * DAY_NS), 3)
        if fo > 0:
            out.append({'name': 'weekly', 'period': 7, 'fourier_order': fo,
                        'prior_scale': seasonality_prior_scale, 'mode': seasonality_mode})
        fo = order('daily', daily, (span < 2 * DAY_NS) or (has_dt and min_dt >= DAY_NS), 4)
        if fo > 0:
            out.append({'name': 'daily', 'period': 1, 'fourier_order': fo,
                        'prior_scale': seasonality_prior_scale, 'mode': seasonality_mode})
        return out

    @property
    def specified_changepoints(self):
        """fbprophet's attribute of the same name: were the changepoint dates given?"""
        return self.changepoints is not None

    @property
    def K(self):
        return sum(2 * int(s['fourier_order']) for s in self.seasonalities) + len(self.extra)

    @property
    def theta_stride(self):
        return 3 + self.n_changepoints + self.K

    def to_c(self):
        s = _lib.default_spec()
        s.growth = _lib.GROWTH_LOGISTIC if self.growth == 'logistic' else _lib.GROWTH_LINEAR
        s.n_changepoints = self.n_changepoints
        s.changepoint_range = self.changepoint_range
        s.changepoint_prior_scale = self.changepoint_prior_scale
        if self.changepoints is not None:
            s.changepoints_specified = 1
            for j, v in enumerate(self.changepoints):
                s.changepoint_ns[j] = int(v)
        if len(self.seasonalities) > _lib.MAX_SEAS or len(self.extra) > _lib.MAX_EXTRA:
            raise ValueError('too many seasonalities (max %d) or extra columns (max %d)'
                             % (_lib.MAX_SEAS, _lib.MAX_EXTRA))
        s.n_seas = len(self.seasonalities)
        for i, se in enumerate(self.seasonalities):
            s.seas_period[i] = float(se['period'])
            s.seas_order[i] = int(se['fourier_order'])
            s.seas_prior_scale[i] = float(se.get('prior_scale', self.seasonality_prior_scale))
            s.seas_mode[i] = int(se.get('mode', self.seasonality_mode) == 'multiplicative')
        s.n_extra = len(self.extra)
        for i, e in enumerate(self.extra):
            s.extra_prior_scale[i] = float(e.get('prior_scale', self.holidays_prior_scale))
            s.extra_mode[i] = int(e.get('mode', self.seasonality_mode) == 'multiplicative')
        for k, v in self.lbfgs.items():
            setattr(s, k, v)
        return s

    def _given_seasonalities(self):
        """The seasonalities as the caller gave them: the conditional ones, with their condition_name, where they stood."""
        if not self.conditional:
            return self.seasonalities
        plain, cond = iter(self.seasonalities), iter(self.conditional)
        if len(self._given_conditional) != len(self.seasonalities) + len(self.conditional):    # (a list edited since)
            return self.seasonalities + self.conditional
        return [next(cond) if c else next(plain) for c in self._given_conditional]

    def to_dict(self):
        """The ORIGINAL form: `seasonalities` holds the conditional ones too, `extra` the caller's columns only, so
        from_dict lowers them again (to the same to_c struct)."""
        return {'growth': self.growth, 'seasonality_mode': self.seasonality_mode,
                'n_changepoints': self.n_changepoints, 'changepoint_range': self.changepoint_range,
                'changepoint_prior_scale': self.changepoint_prior_scale,
                'seasonality_prior_scale': self.seasonality_prior_scale,
                'holidays_prior_scale': self.holidays_prior_scale,
                'seasonalities': self._given_seasonalities(),
                'extra': [e for e in self.extra if 'seasonality' not in e] if self.conditional else self.extra,
                'lbfgs': self.lbfgs,
                **({'conditions': self.conditions} if self.conditions else {}),
                **({'holidays': self.holidays} if self.holidays else {}),
                # ISO strings with nanoseconds: JSON (the model blobs' prefix) and YAML keep them exactly
                **({'changepoints': [str(np.datetime64(int(v), 'ns')) for v in self.changepoints]}
                   if self.changepoints is not None else {})}

    @classmethod
    def from_dict(cls, d):
        d = dict(d)
        lb = d.pop('lbfgs', {})
        return cls(**d, **lb)


def changepoints_ns(changepoints):
    """Changepoint dates as sorted int64 ns since the epoch (ModelSpec(changepoints=...))."""
    a = np.asarray(changepoints)
    if a.size == 0:
        a = np.zeros(0, dtype=np.int64)
    elif a.dtype.kind in 'iu':
        a = a.astype(np.int64)
    else:
        a = a.astype('datetime64[ns]').astype(np.int64)
    a = np.sort(a.reshape(-1))
    if a.size > _lib.MAX_S:
        raise ValueError('at most %d changepoints (got %d)' % (_lib.MAX_S, a.size))
    if a.size > 1 and (np.diff(a) == 0).any():
        raise ValueError('changepoints must be distinct dates')
    return a


def changepoint_dates(fit, n=0):
    """The changepoint dates of series n of a fit as int64 ns -- what fbprophet's add_changepoints_to_plot reads from
    ``m.changepoints``.  Specified dates: the spec's own list (integer ns are not exactly recoverable from the scaled
    double); the automatic rule: start_ns + t_change * t_scale_ns of the series' grid, rounded to the nearest ns."""
    g = fit.grid_of(n)
    S = int(g['S'])
    if fit.spec.specified_changepoints:
        return fit.spec.changepoints[:S].copy()
    t = np.asarray(g['t_change'][:S], dtype=np.float64)
    return int(g['start_ns']) + np.rint(t * float(g['t_scale_ns'])).astype(np.int64)


class FitResult(object):
    """Arrays returned by a fit: theta [N][stride], y_scale [N], fval [N], status [N],
    n_iter [N], n_eval [N], grid (structured array, 1 or N entries)."""

    def __init__(self, spec, theta, y_scale, fval, status, n_iter, n_eval, grid):
        self.spec = spec
        self.theta = theta
        self.y_scale = y_scale
        self.fval = fval
        self.status = status
        self.n_iter = n_iter
        self.n_eval = n_eval
        self.grid = grid

    @property
    def N(self):
        return self.theta.shape[0]

    def grid_of(self, n):
        return self.grid[0 if len(self.grid) == 1 else n]


_ctx_cache = {}


def get_context(device=0, slot=0):
    """Cached tsf_ctx for a GPU.  `slot` distinguishes several contexts on one device (each
    context is single-threaded; the multi-device path gives every worker thread its own)."""
    c = _ctx_cache.get((device, slot))
    if c is None:
        c = _lib.Context(device)
        _ctx_cache[(device, slot)] = c
    return c


# ---- several GPUs from one process --------------------------------------------------------------
# series are independent, so a call is cut into contiguous blocks of series, one per
# device, each driven by its own host thread through its own tsf_ctx (ctypes releases the GIL for
# the duration of the C call); no data crosses between devices and the pieces are concatenated
# on the host.  Results are bit-identical to the single-device call.  bench.py measures the
# other arrangement (one PROCESS per GPU under torch.distributed.run).
MIN_SERIES_PER_DEVICE = 512


def resolve_devices(devices=None):
    """None -> the TSF_DEVICES environment variable ("all", or "0,1,2"; unset = one device,
    the default context); 'all' -> every visible GPU; otherwise a list of device ids (an id
    may repeat: that many contexts on that GPU)."""
    if devices is None:
        devices = os.environ.get('TSF_DEVICES') or None
        if devices is None:
            return None
    if isinstance(devices, str):
        if devices.strip().lower() == 'all':
            devices = list(range(_lib.load().tsf_device_count()))
        else:
            devices = [int(x) for x in devices.split(',') if x.strip() != '']
    devices = [int(d) for d in devices]
    return devices if len(devices) > 1 else None


def _contexts(devices):
    seen = {}
    out = []
    for d in devices:
        k = seen.get(d, 0)
        seen[d] = k + 1
        out.append(get_context(d, slot=k + 1))
    return out


def _cuts(weights, parts):
    """Cut points [parts+1] over len(weights) series so that every block carries about the
    same total weight (rows)."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(weights, dtype=np.int64))])
    want = cum[-1] * np.arange(1, parts) / float(parts)
    inner = np.searchsorted(cum, want, side='left')
    return np.concatenate([[0], inner, [len(weights)]]).astype(np.int64)


def _run_blocks(fn, blocks):
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(blocks)) as ex:
        futs = [ex.submit(fn, *b) for b in blocks]
        return [f.result() for f in futs]


def _merge_fits(spec, parts, shared_grid):
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])   # noqa: E731
    grid = parts[0].grid if shared_grid else np.concatenate([p.grid for p in parts])
    return FitResult(spec, cat('theta'), cat('y_scale'), cat('fval'), cat('status'), cat('n_iter'),
                     cat('n_eval'), grid)


def _merge_interleaved(spec, parts_res, N, parts):
    """Inverse of the i mod parts split of an aligned panel."""
    def put(k):
        first = getattr(parts_res[0], k)
        out = np.zeros((N,) + first.shape[1:], dtype=first.dtype)
        for d, p in enumerate(parts_res):
            out[parallel.shard_indices(N, d, parts)] = getattr(p, k)
        return out
    return FitResult(spec, put('theta'), put('y_scale'), put('fval'), put('status'), put('n_iter'),
                     put('n_eval'), parts_res[0].grid)


def _opt_f64(a, N, name):
    if a is None:
        return None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (N,)))
    return a


_DS_FUTURE_SHAPE = 'ds_future must be [H] or [N][H]'


def _forecast_inputs(spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key=None):
    """What every predict entry is handed, marshalled for the library: (theta, N, y_scale, grid, ds_future, shared, H,
    floor, cap, ex, key), each array contiguous in the library's type, the optional ones None where not given."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    N = theta.shape[0]
    y_scale = np.ascontiguousarray(y_scale, dtype=np.float64)
    grid = np.ascontiguousarray(grid, dtype=_lib.GRID_DTYPE)
    ds_future_ns = np.ascontiguousarray(ds_future_ns, dtype=np.int64)
    shared = ds_future_ns.ndim == 1
    H = ds_future_ns.shape[-1]
    if not shared and ds_future_ns.shape != (N, H):
        raise ValueError(_DS_FUTURE_SHAPE)
    floor = _opt_f64(floor, N, 'floor')
    cap = _opt_f64(cap, N, 'cap')
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra_future, dtype=np.float64)
        want = (len(spec.extra), H) if shared else (N, len(spec.extra), H)
        if ex.shape != want:
            raise ValueError('extra_future must be %r' % (want,))
    key = None if series_key is None else np.ascontiguousarray(series_key, dtype=np.int64)
    if key is not None and key.shape != (N,):
        raise ValueError('series_key must be [N]')
    return theta, N, y_scale, grid, ds_future_ns, shared, H, floor, cap, ex, key


def _alloc_out(N, stride, n_grids):
    theta = np.zeros((N, stride))
    y_scale = np.zeros(N)
    fval = np.zeros(N)
    status = np.zeros(N, dtype=np.int32)
    n_iter = np.zeros(N, dtype=np.int32)
    n_eval = np.zeros(N, dtype=np.int32)
    grid = np.zeros(n_grids, dtype=_lib.GRID_DTYPE)
    out = _lib.TsfFitOut(theta.ctypes.data, y_scale.ctypes.data, fval.ctypes.data,
                         status.ctypes.data, n_iter.ctypes.data, n_eval.ctypes.data,
                         grid.ctypes.data)
    return out, (theta, y_scale, fval, status, n_iter, n_eval, grid)


def fit_aligned(spec, ds_ns, y, floor=None, cap=None, extra=None, ctx=None, devices=None, cost_hints=None):
    """Fit N series observed on the same T timestamps.  y: [N][T] float64/float32/int32.
    devices: see resolve_devices (several GPUs, one host thread each).
    cost_hints: optional [N] expected relative cost per series (the `n_eval` of an earlier fit of the same series):
    the launch starts its longest fits first (tsf_set_cost_hints); results do not depend on it."""
    devs = None if ctx is not None else resolve_devices(devices)
    ch = None if cost_hints is None else np.ascontiguousarray(cost_hints, dtype=np.int32)
    if ch is not None and ch.shape != (len(y),):
        raise ValueError('cost_hints must be [N]')
    if devs and len(y) >= 2 * MIN_SERIES_PER_DEVICE:
        parts = min(len(devs), len(y) // MIN_SERIES_PER_DEVICE)
        fl = _opt_f64(floor, len(y), 'floor')
        cp = _opt_f64(cap, len(y), 'cap')
        # series i goes to device i mod parts (evaluation counts vary 3-40x per series and
        # neighbours in a panel tend to be alike; interleaving evens the devices out where contiguous
        # blocks would not); parallel.shard_indices is the one statement of that layout (bench.py --gpus N
        # deals its ranks the same way)
        y = np.asarray(y)
        blocks = [(c, parallel.shard_indices(len(y), d, parts)) for d, c in enumerate(_contexts(devs[:parts]))]
        res = _run_blocks(lambda c, idx: fit_aligned(
            spec, ds_ns, np.ascontiguousarray(y[idx]), None if fl is None else fl[idx],
            None if cp is None else cp[idx], extra, ctx=c,
            cost_hints=None if ch is None else ch[idx]), blocks)
        return _merge_interleaved(spec, res, len(y), parts)
    ctx = ctx or get_context()
    L = _lib.load()
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    y = np.ascontiguousarray(y)
    if y.ndim != 2 or y.shape[1] != ds_ns.shape[0]:
        raise ValueError('y must be [N][T] with T == len(ds)')
    if ch is not None:
        ctx.check(L.tsf_set_cost_hints(ctx.handle, ch.ctypes.data, ch.shape[0]))
    N, T = y.shape
    cs = spec.to_c()
    floor = _opt_f64(floor, N, 'floor')
    cap = _opt_f64(cap, N, 'cap')
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (len(spec.extra), T):
            raise ValueError('extra must be [n_extra][T]')
    out, arrs = _alloc_out(N, spec.theta_stride, 1)
    rc = L.tsf_fit_aligned(ctx.handle, ctypes.byref(cs), N, T, ds_ns.ctypes.data, y.ctypes.data,
                           _lib.y_dtype_code(y), _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex),
                           ctypes.byref(out))
    ctx.check(rc)
    return FitResult(spec, *arrs)


def fit_ragged(spec, offsets, ds_ns, y, floor=None, cap=None, extra=None, ctx=None, devices=None, cost_hints=None):
    """Fit N series of different lengths / timestamps; series n owns rows
    offsets[n]:offsets[n+1] of ds_ns / y (each slice sorted by ds, NaN rows removed).
    cost_hints: as in fit_aligned."""
    devs = None if ctx is not None else resolve_devices(devices)
    ch = None if cost_hints is None else np.ascontiguousarray(cost_hints, dtype=np.int32)
    if ch is not None and ch.shape != (len(offsets) - 1,):
        raise ValueError('cost_hints must be [N]')
    if devs and len(offsets) - 1 >= 2 * MIN_SERIES_PER_DEVICE:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        N = len(offsets) - 1
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        cuts = _cuts(np.diff(offsets), parts)
        fl = _opt_f64(floor, N, 'floor')
        cp = _opt_f64(cap, N, 'cap')
        ex = None if extra is None else np.asarray(extra)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:])
                  if b > a]

        def one(c, a, b):
            r0, r1 = int(offsets[a]), int(offsets[b])
            return fit_ragged(spec, offsets[a:b + 1] - r0, ds_ns[r0:r1], y[r0:r1],
                              None if fl is None else fl[a:b], None if cp is None else cp[a:b],
                              None if ex is None else ex[:, r0:r1], ctx=c,
                              cost_hints=None if ch is None else ch[a:b])
        return _merge_fits(spec, _run_blocks(one, blocks), shared_grid=False)
    ctx = ctx or get_context()
    L = _lib.load()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    y = np.ascontiguousarray(y)
    N = len(offsets) - 1
    if y.ndim != 1 or y.shape[0] != ds_ns.shape[0] or offsets[-1] != y.shape[0]:
        raise ValueError('ds / y must be 1-D with offsets[-1] rows')
    cs = spec.to_c()
    floor = _opt_f64(floor, N, 'floor')
    cap = _opt_f64(cap, N, 'cap')
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (len(spec.extra), y.shape[0]):
            raise ValueError('extra must be [n_extra][total_rows]')
    out, arrs = _alloc_out(N, spec.theta_stride, N)
    if ch is not None:
        ctx.check(L.tsf_set_cost_hints(ctx.handle, ch.ctypes.data, ch.shape[0]))
    rc = L.tsf_fit_ragged(ctx.handle, ctypes.byref(cs), N, offsets.ctypes.data, ds_ns.ctypes.data,
                          y.ctypes.data, _lib.y_dtype_code(y), _lib._ptr(floor), _lib._ptr(cap),
                          _lib._ptr(ex), ctypes.byref(out))
    ctx.check(rc)
    return FitResult(spec, *arrs)


# ---- conditional seasonalities: the one construction path of their columns ---------------------------

def _condition_rows(spec, shape, ds_ns, conditions):
    """uint8 [n_cond][...shape] and the condition row of each conditional seasonality: a condition given as an array
    wins, else the spec's date rule of that name; fbprophet's two messages where neither exists / a value is no
    boolean (setup_dataframe)."""
    from . import features
    names = []
    for s in spec.conditional:
        if s['condition_name'] not in names:
            names.append(s['condition_name'])
    conditions = conditions or {}
    rows = np.zeros((len(names),) + shape, dtype=np.uint8)
    for r, name in enumerate(names):
        if name in conditions:
            v = np.asarray(conditions[name])
            if v.shape != shape:
                raise ValueError("condition %r must have the shape of ds %r" % (name, shape))
            if v.dtype != np.bool_:
                try:                                                # (NaN, 2, 'yes', None: no boolean)
                    f = np.asarray(v, dtype=np.float64) if v.dtype.kind not in 'USMm' else None
                    ok = f is not None and bool(((f == 0) | (f == 1)).all())
                except (TypeError, ValueError):
                    ok = False
                if not ok:
                    raise ValueError("Found non-boolean in column %r" % name)
                v = v.astype(bool)
            rows[r] = v
        elif name in spec.conditions:
            rows[r] = features.condition_mask(spec.conditions[name], ds_ns)
        else:
            raise ValueError("Condition %r missing from dataframe" % name)
    return rows, [names.index(s['condition_name']) for s in spec.conditional]


def conditional_extra(spec, ds_ns, conditions=None, extra=None, offsets=None, ctx=None):
    """The full `extra` array of `spec` -- the caller's columns in front, the columns of the conditional seasonalities
    behind them (include/tsf.h tsf_cond_columns) -- for any entry point that takes `extra` / `extra_future`.

    ds_ns [T] (an aligned panel's or a shared future's timestamps), conditions {name: bool [T]}, extra [n_user_extra][T]
    -> [n_extra][T]; ds_ns ragged [rows] with offsets (fit_ragged's layout; a column value depends on its own row
    alone, so the offsets are only checked) -> [n_extra][rows]; ds_ns [N][H], conditions [N][H] each, extra
    [N][n_user_extra][H] -> [N][n_extra][H], predict's per-series future layout.  A condition not given falls back on the
    spec's date rule of that name (ModelSpec(conditions=...)).  A spec without conditional seasonalities: `extra` as
    given.  One upload of ds and the masks, one launch, one download."""
    if not spec.conditional:
        return extra
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    if ds_ns.ndim not in (1, 2):
        raise ValueError('ds must be [T], ragged [rows] or [N][H]')
    if offsets is not None:
        offsets = np.asarray(offsets, dtype=np.int64)
        if ds_ns.ndim != 1 or len(offsets) < 1 or offsets[-1] != ds_ns.shape[0]:
            raise ValueError('ds must be 1-D with offsets[-1] rows')
    nu, ne = spec.n_user_extra, len(spec.extra)
    C = ne - nu
    ex = None
    if nu:
        ex = np.asarray(extra, dtype=np.float64)
        want = (nu,) + ds_ns.shape if ds_ns.ndim == 1 else (ds_ns.shape[0], nu, ds_ns.shape[1])
        if ex.shape != want:
            raise ValueError('extra must be %r: the caller\'s %d columns' % (want, nu))
    cond, which = _condition_rows(spec, ds_ns.shape, ds_ns, conditions)
    cs = _lib.TsfCondSeas()
    if len(spec.conditional) > _lib.MAX_SEAS or ne > _lib.MAX_EXTRA:
        raise ValueError('too many seasonalities (max %d) or extra columns (max %d)' % (_lib.MAX_SEAS, _lib.MAX_EXTRA))
    cs.n = len(spec.conditional)
    for i, s in enumerate(spec.conditional):
        cs.period[i], cs.order[i], cs.cond[i] = float(s['period']), int(s['fourier_order']), which[i]
    rows = ds_ns.size
    flat = ds_ns.ndim == 1
    out = np.empty((ne, rows)) if flat else np.empty((ds_ns.shape[0], ne, ds_ns.shape[1]))
    cols = out[nu:] if flat else np.empty((C, rows))       # (flat: written in place, at the stride of the whole block)
    cond = np.ascontiguousarray(cond.reshape(len(cond), rows))
    ctx = ctx or get_context()
    ctx.check(_lib.load().tsf_cond_columns(ctx.handle, ctypes.byref(cs), rows, ds_ns.ctypes.data, cond.shape[0],
                                           cond.ctypes.data, cols.ctypes.data, rows))
    if flat:
        if nu:
            out[:nu] = ex
    else:
        if nu:
            out[:, :nu] = ex
        out[:, nu:] = cols.reshape(C, ds_ns.shape[0], ds_ns.shape[1]).transpose(1, 0, 2)
    return out


def predict(spec, theta, y_scale, grid, ds_future_ns, floor=None, cap=None, extra_future=None,
            want_int=False, ctx=None, devices=None, noise_ar=None):
    """yhat [N][H] (float64) and, if want_int, the reference's int-truncated + floor-clamped
    column (prophet_scorer.py:73-84).  ds_future_ns: [H] (shared) or [N][H].  noise_ar: a NoiseAR.conditioned() object
    -- yhat plus the conditional mean of the AR(1) noise given the history's last residual (tsf_noise_ar_mean; one
    numpy add, series with phi == 0 untouched): the corrected point forecast without a draw, the yhat of the drawing
    calls with the same noise_ar."""
    if noise_ar is not None:
        start = _noise_ar_phi(noise_ar, len(np.asarray(theta)), ds_future_ns)
        if not isinstance(start, _NoiseArArmed):
            raise ValueError('predict takes noise_ar only as a NoiseAR.conditioned() object: a phi alone does not move yhat')
        if want_int:
            raise ValueError('noise_ar together with want_int: the integer column is the uncorrected forecast\'s')
        yhat = predict(spec, theta, y_scale, grid, ds_future_ns, floor=floor, cap=cap, extra_future=extra_future,
                       ctx=ctx, devices=devices)
        mean = noise_ar_mean(start.phi, start.resid, start.steps, yhat.shape[1])
        return np.where((start.phi != 0.0)[:, None], yhat + mean, yhat)
    devs = None if ctx is not None else resolve_devices(devices)
    if devs and len(theta) >= 2 * MIN_SERIES_PER_DEVICE:
        N = len(theta)
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        cuts = _cuts(np.ones(N, np.int64), parts)
        fl = _opt_f64(floor, N, 'floor')
        cp = _opt_f64(cap, N, 'cap')
        fut = np.asarray(ds_future_ns)
        exf = None if extra_future is None else np.asarray(extra_future)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:])]

        def one(c, a, b):
            return predict(spec, theta[a:b], np.asarray(y_scale)[a:b],
                           grid if len(grid) == 1 else grid[a:b],
                           fut if fut.ndim == 1 else fut[a:b],
                           None if fl is None else fl[a:b], None if cp is None else cp[a:b],
                           exf if (exf is None or fut.ndim == 1) else exf[a:b], want_int=want_int, ctx=c)
        res = _run_blocks(one, blocks)
        if want_int:
            return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
        return np.concatenate(res)
    ctx = ctx or get_context()
    L = _lib.load()
    theta, N, y_scale, grid, ds_future_ns, shared, H, floor, cap, ex, _ = _forecast_inputs(
        spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future)
    cs = spec.to_c()
    yhat = np.zeros((N, H))
    yint = np.zeros((N, H), dtype=np.int32) if want_int else None
    rc = L.tsf_predict(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                       grid.ctypes.data, len(grid), ds_future_ns.ctypes.data, int(shared),
                       _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex), yhat.ctypes.data,
                       _lib._ptr(yint))
    ctx.check(rc)
    return (yhat, yint) if want_int else yhat


def predict_intervals(spec, theta, y_scale, grid, ds_future_ns, floor=None, cap=None, extra_future=None,
                      series_key=None, uncertainty_samples=1000, interval_width=0.8, seed=0, ctx=None, noise_ar=None):
    """(yhat, yhat_lower, yhat_upper), each [N][H]: fbprophet's predict_uncertainty -- which the
    reference computes inside model.predict (prophet_scorer.py:70) and drops (:86) -- with a seeded
    counter-based generator (include/tsf.h tsf_predict_intervals).  series_key [N] int64: what the
    random streams are keyed by (e.g. a hash of (series_id, dim_id)), so that a series gets the same
    interval whatever batch it is in; default: its index in this call.  noise_ar: see residual_autocorrelation."""
    ctx = ctx or get_context()
    L = _lib.load()
    theta, N, y_scale, grid, ds_future_ns, shared, H, floor, cap, ex, key = _forecast_inputs(
        spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key)
    phi = _noise_ar_phi(noise_ar, N, ds_future_ns)
    cs = spec.to_c()
    yhat, lo, hi = np.zeros((N, H)), np.zeros((N, H)), np.zeros((N, H))
    _set_noise_ar(ctx, phi)
    rc = L.tsf_predict_intervals(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                                 grid.ctypes.data, len(grid), ds_future_ns.ctypes.data, int(shared),
                                 _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex), _lib._ptr(key),
                                 int(uncertainty_samples), float(interval_width), int(seed),
                                 yhat.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    ctx.check(rc)
    return yhat, lo, hi


# ---- forecast components ----------------------------------------------------------------------------
# fbprophet 0.5's Prophet.predict returns the decomposition beside yhat: trend, one column per seasonality /
# holiday / regressor, the group totals, each with _lower / _upper (regressor_column_matrix, add_group_component,
# predict_seasonal_components, predict_uncertainty; restated from recall, parity with the real package not pinned).
# The library computes any set of components given as design-column masks (include/tsf.h tsf_predict_components);
# component_columns names the sets fbprophet forms for a model.

def component_columns(spec):
    """[(name, mask, scaled)] of the components fbprophet 0.5 forms for `spec`, in its column order: the columns of
    pandas.crosstab over (design column, component), i.e. sorted by name, then 'additive_terms' / 'multiplicative_terms'
    appended if they have no column (regressor_column_matrix adds them empty, behind the others).  mask: bit j =
    original design column j; scaled: the component is additive (times y_scale).  Components: one per seasonality; one
    per holiday (the name before '_delim_' of the leading extra columns features.holiday_columns(spec.holidays) names)
    and 'holidays'; one per other extra column (a regressor) except the 'zeros' placeholder, and
    'extra_regressors_additive' / '_multiplicative' where non-empty; 'additive_terms' and 'multiplicative_terms'.
    The extra columns of a conditional seasonality (their 'seasonality' key) form one component of its name, counted
    in its mode's total like any seasonality, not among the regressors."""
    from . import features
    ADD, MUL = 'additive', 'multiplicative'
    masks, modes = {}, {}
    total = {ADD: 0, MUL: 0}
    reg = {ADD: 0, MUL: 0}

    def put(name, bits, mode):
        masks[name] = masks.get(name, 0) | bits
        modes[name] = mode
        total[mode] |= bits

    col = 0
    for se in spec.seasonalities:
        w = 2 * int(se['fourier_order'])
        if w:
            put(se['name'], ((1 << w) - 1) << col, se.get('mode', spec.seasonality_mode))
        col += w
    n_hol = len(features.holiday_columns(features.normalize_holidays(spec.holidays))[0]) if spec.holidays else 0
    hol = 0
    for e, ex in enumerate(spec.extra):
        bit, mode = 1 << (col + e), ex.get('mode', spec.seasonality_mode)
        if e < n_hol:
            put(ex['name'].split('_delim_')[0], bit, mode)
            hol |= bit
        elif 'seasonality' in ex:             # a lowered conditional seasonality's column: a seasonality, not a regressor
            put(ex['seasonality'], bit, mode)
        elif ex['name'] == 'zeros':           # fbprophet's placeholder column: in its mode's total, no component of its own
            total[mode] |= bit
        else:
            put(ex['name'], bit, mode)
            reg[mode] |= bit
    if hol:
        masks['holidays'], modes['holidays'] = hol, spec.seasonality_mode
    for mode in (ADD, MUL):
        if reg[mode]:
            masks['extra_regressors_' + mode], modes['extra_regressors_' + mode] = reg[mode], mode
        if total[mode]:
            masks[mode + '_terms'], modes[mode + '_terms'] = total[mode], mode
    names = sorted(masks)
    for mode in (ADD, MUL):
        if not total[mode]:
            names.append(mode + '_terms')
            masks[mode + '_terms'], modes[mode + '_terms'] = 0, mode
    return [(n, masks[n], int(modes[n] == ADD)) for n in names]


class Components(object):
    """What predict_components returns: names [C]; yhat, trend [N][H]; comp [N][C][H] and terms (name -> its [N][H]
    view of comp); trend_lower / trend_upper / yhat_lower / yhat_upper [N][H] with intervals, else None."""

    def __init__(self, spec, names, yhat, trend, comp, yhat_lower=None, yhat_upper=None, trend_lower=None,
                 trend_upper=None, floor=None, cap=None):
        self.spec, self.names = spec, list(names)
        self.yhat, self.trend, self.comp = yhat, trend, comp
        self.terms = {name: comp[:, i, :] for i, name in enumerate(self.names)}
        self.yhat_lower, self.yhat_upper = yhat_lower, yhat_upper
        self.trend_lower, self.trend_upper = trend_lower, trend_upper
        self.floor, self.cap = floor, cap

    @property
    def intervals(self):
        return self.yhat_lower is not None

    def frame(self, n, ds, cap=None, floor=None):
        """Series n as a DataFrame in fbprophet 0.5's predict() layout: ds, trend, cap and floor (logistic growth; default:
        the values predict_components was given), yhat_lower, yhat_upper, trend_lower, trend_upper (with intervals), then
        per component c: c, c_lower, c_upper (a MAP fit has one beta: all three equal), yhat last."""
        import pandas as pd
        ds = np.asarray(ds)
        if ds.dtype.kind != 'M':
            ds = ds.astype(np.int64).view('datetime64[ns]')
        cols = {'ds': ds, 'trend': self.trend[n]}
        if self.spec.growth == 'logistic':
            cap = self.cap[n] if cap is None and self.cap is not None else cap
            if cap is None:
                raise ValueError('logistic growth: cap is needed')
            floor = (self.floor[n] if self.floor is not None else 0.0) if floor is None else floor
            cols['cap'] = np.broadcast_to(np.asarray(cap, dtype=np.float64), ds.shape)
            cols['floor'] = np.broadcast_to(np.asarray(floor, dtype=np.float64), ds.shape)
        if self.intervals:
            for k in ('yhat_lower', 'yhat_upper', 'trend_lower', 'trend_upper'):
                cols[k] = getattr(self, k)[n]
        for name in self.names:
            v = self.terms[name][n]
            cols[name], cols[name + '_lower'], cols[name + '_upper'] = v, v, v
        cols['yhat'] = self.yhat[n]
        return pd.DataFrame(cols, columns=list(cols))


def predict_components(spec, theta, y_scale, grid, ds_future_ns, floor=None, cap=None, extra_future=None,
                       intervals=False, series_key=None, uncertainty_samples=1000, interval_width=0.8, seed=0,
                       ctx=None, devices=None, columns=None):
    """Trend, yhat and the components of component_columns(spec) (or `columns`: [(name, mask, scaled)]) for every
    series (include/tsf.h tsf_predict_components) -> Components.  yhat is predict's bit for bit; with intervals,
    yhat_lower / yhat_upper are predict_intervals' (same series_key, samples, width, seed) and trend_lower /
    trend_upper the same percentiles of the sampled trend.  devices: as predict."""
    cols = component_columns(spec) if columns is None else [tuple(c) for c in columns]
    devs = None if ctx is not None else resolve_devices(devices)
    if devs and len(theta) >= 2 * MIN_SERIES_PER_DEVICE:
        N = len(theta)
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        cuts = _cuts(np.ones(N, np.int64), parts)
        fl = _opt_f64(floor, N, 'floor')
        cp = _opt_f64(cap, N, 'cap')
        fut = np.asarray(ds_future_ns)
        exf = None if extra_future is None else np.asarray(extra_future)
        key = None if series_key is None else np.asarray(series_key, dtype=np.int64)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:])]

        def one(c, a, b):
            return predict_components(spec, theta[a:b], np.asarray(y_scale)[a:b],
                                      grid if len(grid) == 1 else grid[a:b], fut if fut.ndim == 1 else fut[a:b],
                                      None if fl is None else fl[a:b], None if cp is None else cp[a:b],
                                      exf if (exf is None or fut.ndim == 1) else exf[a:b], intervals=intervals,
                                      # (the default key is the series' index in the whole call)
                                      series_key=np.arange(a, b, dtype=np.int64) if key is None else key[a:b],
                                      uncertainty_samples=uncertainty_samples, interval_width=interval_width,
                                      seed=seed, ctx=c, columns=cols)
        res = _run_blocks(one, blocks)
        cat = lambda k: None if getattr(res[0], k) is None else np.concatenate([getattr(r, k) for r in res])  # noqa: E731
        return Components(spec, res[0].names, cat('yhat'), cat('trend'), cat('comp'), cat('yhat_lower'),
                          cat('yhat_upper'), cat('trend_lower'), cat('trend_upper'), fl, cp)
    ctx = ctx or get_context()
    L = _lib.load()
    theta, N, y_scale, grid, ds_future_ns, shared, H, floor, cap, ex, key = _forecast_inputs(
        spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key)
    cs = spec.to_c()
    C = len(cols)
    masks = np.array([int(m) for _, m, _ in cols], dtype=np.uint64)
    scaled = np.array([int(s) for _, _, s in cols], dtype=np.int32)
    yhat, trend, comp = np.zeros((N, H)), np.zeros((N, H)), np.zeros((N, C, H))
    iv = [np.zeros((N, H)) for _ in range(4)] if intervals else [None] * 4
    rc = L.tsf_predict_components(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                                  grid.ctypes.data, len(grid), ds_future_ns.ctypes.data, int(shared),
                                  _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex), C, masks.ctypes.data,
                                  scaled.ctypes.data, _lib._ptr(key), int(uncertainty_samples) if intervals else 0,
                                  float(interval_width), int(seed), yhat.ctypes.data, trend.ctypes.data,
                                  comp.ctypes.data, *[_lib._ptr(a) for a in iv])
    ctx.check(rc)
    return Components(spec, [c[0] for c in cols], yhat, trend, comp, *iv, floor=floor, cap=cap)


# ---- forecast quantiles, cumulative quantiles, predictive samples ----------------------------------
# The predictive distribution behind predict_intervals' one symmetric pair (include/tsf.h tsf_predict_quantiles): any
# set of levels from one draw and one sort per row, the same levels of each sample's running sum over the future rows,
# and the raw draws (fbprophet 0.5's Prophet.predictive_samples; restated from recall, parity not pinned).

def quantile_columns(quantiles, prefix='yhat_q'):
    """Column names of quantile levels: 0.1 -> 'yhat_q10', 0.975 -> 'yhat_q97.5' ('%s%s' % (prefix, format(100 * p,
    'g'))).  ValueError for a level that is not finite or outside [0, 1], for two levels with the same name and for
    more than MAX_QUANT levels."""
    levels = [float(p) for p in np.asarray(quantiles, dtype=np.float64).reshape(-1)]
    if len(levels) > _lib.MAX_QUANT:
        raise ValueError('at most %d quantile levels (got %d)' % (_lib.MAX_QUANT, len(levels)))
    names = []
    for p in levels:
        if not (np.isfinite(p) and 0.0 <= p <= 1.0):
            raise ValueError('quantile level %r: must be finite and in [0, 1]' % (p,))
        name = '%s%s' % (prefix, format(100 * p, 'g'))
        if name in names:
            raise ValueError('quantile levels: two levels are named %s' % name)
        names.append(name)
    return names


class Quantiles(object):
    """What predict_quantiles returns: yhat [N][H]; quantiles [Q] (the levels as given); q [N][Q][H]; cum_q and
    trend_q [N][Q][H] or None."""

    def __init__(self, yhat, quantiles, q, cum_q=None, trend_q=None):
        self.yhat, self.quantiles, self.q, self.cum_q, self.trend_q = yhat, quantiles, q, cum_q, trend_q

    def frame(self, n, ds):
        """Series n as a DataFrame: ds, yhat, yhat_q<..> per level, then yhat_cum_q<..> and trend_q<..> where computed
        (names: quantile_columns)."""
        import pandas as pd
        ds = np.asarray(ds)
        if ds.dtype.kind != 'M':
            ds = ds.astype(np.int64).view('datetime64[ns]')
        cols = {'ds': ds, 'yhat': self.yhat[n]}
        for prefix, arr in (('yhat_q', self.q), ('yhat_cum_q', self.cum_q), ('trend_q', self.trend_q)):
            if arr is not None:
                for i, name in enumerate(quantile_columns(self.quantiles, prefix)):
                    cols[name] = arr[n, i]
        return pd.DataFrame(cols, columns=list(cols))


def _predict_quantiles_call(spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key,
                            uncertainty_samples, seed, levels, want, ctx, noise_ar=None):
    """One tsf_predict_quantiles call -> dict of the outputs named in `want` (and yhat)."""
    ctx = ctx or get_context()
    L = _lib.load()
    theta, N, y_scale, grid, ds_future_ns, shared, H, floor, cap, ex, key = _forecast_inputs(
        spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key)
    phi = _noise_ar_phi(noise_ar, N, ds_future_ns)
    cs = spec.to_c()
    levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    Q, S = len(levels), int(uncertainty_samples)
    res = {'yhat': np.zeros((N, H))}
    for k in ('q', 'cum_q', 'trend_q'):
        if k in want:
            res[k] = np.zeros((N, Q, H))
    for k in ('samples', 'trend_samples'):
        if k in want:
            if not 2 <= S <= 4096:          # (the library refuses it too; here before an array is sized by it)
                raise ValueError('uncertainty_samples must be in [2, 4096]')
            res[k] = np.zeros((N, H, S))
    out = _lib.TsfQuantileOut(**{k: v.ctypes.data for k, v in res.items()})
    _set_noise_ar(ctx, phi)
    rc = L.tsf_predict_quantiles(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                                 grid.ctypes.data, len(grid), ds_future_ns.ctypes.data, int(shared),
                                 _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex), _lib._ptr(key), S, int(seed),
                                 Q, levels.ctypes.data if Q else None, ctypes.byref(out))
    ctx.check(rc)
    return res


def predict_quantiles(spec, theta, y_scale, grid, ds_future_ns, quantiles, floor=None, cap=None, extra_future=None,
                      series_key=None, uncertainty_samples=1000, seed=0, cumulative=False, trend=False, ctx=None,
                      noise_ar=None):
    """Quantiles of the simulated futures of every series -> Quantiles (include/tsf.h tsf_predict_quantiles): q [N][Q][H]
    per future row at the levels `quantiles` (in [0, 1]; 0.5 the median); with cumulative, cum_q: the same levels of each
    sample's running sum over the future rows (row h: the total of rows 0..h, e.g. demand over a lead time); with trend,
    trend_q: of the sampled trend.  The draws are predict_intervals' (same series_key, samples, seed): levels
    (1 - w) / 2, (1 + w) / 2 give its yhat_lower / yhat_upper at width w bit for bit; yhat is predict's.  noise_ar: phi
    [N] or a NoiseAR (residual_autocorrelation) -- the observation noise of each sample's rows is then an AR(1) chain
    (include/tsf.h "serially correlated observation noise"): q keeps its law, cum_q widens as a real total's spread does."""
    want = ['q'] + (['cum_q'] if cumulative else []) + (['trend_q'] if trend else [])
    levels = np.array(quantiles, dtype=np.float64).reshape(-1)
    r = _predict_quantiles_call(spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key,
                                uncertainty_samples, seed, levels, want, ctx, noise_ar=noise_ar)
    return Quantiles(r['yhat'], levels, r['q'], r.get('cum_q'), r.get('trend_q'))


def predictive_samples(spec, theta, y_scale, grid, ds_future_ns, floor=None, cap=None, extra_future=None,
                       series_key=None, uncertainty_samples=1000, seed=0, ctx=None, noise_ar=None):
    """fbprophet 0.5's Prophet.predictive_samples for a panel: {'yhat': [N][H][S], 'trend': [N][H][S]}, the raw draws
    behind predict_intervals / predict_quantiles (sample s at index s, whatever S is; the trend before the observation
    noise).  For one series [n] is fbprophet's (H, S) layout.  N * H * S * 16 bytes of host memory."""
    r = _predict_quantiles_call(spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future, series_key,
                                uncertainty_samples, seed, [], ['samples', 'trend_samples'], ctx, noise_ar=noise_ar)
    return {'yhat': r['samples'], 'trend': r['trend_samples']}


# ---- scoring observed values against the predictive distribution -----------------------------------
# The other half of predict_quantiles (include/tsf.h tsf_score_actuals): given the values observed on the forecast
# rows, the PIT, the sample CRPS and the pinball losses per row, their means and the coverage of every level per series,
# from the same draws and the same sort per row; only [N][H]-sized answers leave the device.

SCORE_ROW_FIELDS = ('pit', 'crps', 'q', 'pinball')
SCORE_SERIES_FIELDS = ('n_obs', 'mean_crps', 'mean_pinball', 'coverage')
_SCORE_LEVEL_FIELDS = ('q', 'pinball', 'mean_pinball', 'coverage')


class Scores(object):
    """What score_actuals returns (include/tsf.h tsf_score_out): y and yhat [N][H]; quantiles [Q] (the levels as
    given); per row pit, crps [N][H] and q, pinball [N][Q][H]; per series n_obs [N] (int32), mean_crps [N],
    mean_pinball, coverage [N][Q].  q, pinball, mean_pinball and coverage are None without levels.  Rows whose y is NaN
    (not observed) have NaN in pit, crps and pinball and count in no mean."""

    def __init__(self, y, yhat, quantiles, pit=None, crps=None, q=None, pinball=None, n_obs=None, mean_crps=None,
                 mean_pinball=None, coverage=None):
        self.y, self.yhat, self.quantiles = y, yhat, quantiles
        self.pit, self.crps, self.q, self.pinball = pit, crps, q, pinball
        self.n_obs, self.mean_crps, self.mean_pinball, self.coverage = n_obs, mean_crps, mean_pinball, coverage

    def frame(self, n, ds):
        """Series n as a DataFrame: ds, y, yhat, pit, crps, then yhat_q<..> and pinball_q<..> per level (names:
        quantile_columns)."""
        import pandas as pd
        ds = np.asarray(ds)
        if ds.dtype.kind != 'M':
            ds = ds.astype(np.int64).view('datetime64[ns]')
        cols = {'ds': ds, 'y': self.y[n], 'yhat': self.yhat[n]}
        for k in ('pit', 'crps'):
            if getattr(self, k) is not None:
                cols[k] = getattr(self, k)[n]
        if self.q is not None or self.pinball is not None:
            for i, (qn, pn) in enumerate(zip(quantile_columns(self.quantiles), quantile_columns(self.quantiles, 'pinball_q'))):
                if self.q is not None:
                    cols[qn] = self.q[n, i]
                if self.pinball is not None:
                    cols[pn] = self.pinball[n, i]
        return pd.DataFrame(cols, columns=list(cols))

    def anomalies(self, alpha):
        """Boolean mask [N][H]: rows whose observed value lies in the two-sided alpha tail of their predictive
        distribution, pit < alpha / 2 or pit > 1 - alpha / 2; False on rows that were not observed.  The PIT comes from
        uncertainty_samples draws, so its resolution is 0.5 / uncertainty_samples: an alpha below 1 / uncertainty_samples
        flags only values outside every draw, and none finer than that can be told apart."""
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError('alpha must be in (0, 1)')
        if self.pit is None:
            raise ValueError('anomalies needs the pit output')
        with np.errstate(invalid='ignore'):
            return (self.pit < alpha / 2.0) | (self.pit > 1.0 - alpha / 2.0)


def _checked_forecast_inputs(spec, theta, y_scale, grid, ds_ns, floor, cap, extra_future, series_key):
    """_forecast_inputs with every shape checked here: (theta, N, y_scale, grid, ds, shared, H, floor, cap, ex, key), a
    ValueError for any argument of the wrong shape.  The library is not touched."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.ndim != 2 or theta.shape[1] != spec.theta_stride:
        raise ValueError('theta must be [N][%d]' % spec.theta_stride)
    N = theta.shape[0]
    y_scale = np.ascontiguousarray(y_scale, dtype=np.float64)
    if y_scale.shape != (N,):
        raise ValueError('y_scale must be [N]')
    grid = np.ascontiguousarray(grid, dtype=_lib.GRID_DTYPE)
    if grid.ndim != 1 or len(grid) not in (1, N):
        raise ValueError('grid must hold 1 or N records')
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    shared = ds_ns.ndim == 1
    H = ds_ns.shape[-1]
    if ds_ns.ndim not in (1, 2) or H < 1 or (not shared and ds_ns.shape != (N, H)):
        raise ValueError('ds must be [H] or [N][H], H >= 1')
    floor = _opt_f64(floor, N, 'floor')
    cap = _opt_f64(cap, N, 'cap')
    ex = None
    if spec.extra:
        if extra_future is None:
            raise ValueError('extra_future is required: the spec has extra columns')
        ex = np.ascontiguousarray(extra_future, dtype=np.float64)
        shape = (len(spec.extra), H) if shared else (N, len(spec.extra), H)
        if ex.shape != shape:
            raise ValueError('extra_future must be %r' % (shape,))
    key = None if series_key is None else np.ascontiguousarray(series_key, dtype=np.int64)
    if key is not None and key.shape != (N,):
        raise ValueError('series_key must be [N]')
    return theta, N, y_scale, grid, ds_ns, shared, H, floor, cap, ex, key


def _score_actuals_call(spec, theta, y_scale, grid, ds_ns, y_obs, floor, cap, extra_future, series_key,
                        uncertainty_samples, seed, levels, want, ctx, noise_ar=None):
    """One tsf_score_actuals call -> dict of the outputs named in `want` (and yhat).  Every argument-shape error is
    raised before the library is loaded."""
    theta, N, y_scale, grid, ds_ns, shared, H, floor, cap, ex, key = _checked_forecast_inputs(
        spec, theta, y_scale, grid, ds_ns, floor, cap, extra_future, series_key)
    y_obs = np.ascontiguousarray(y_obs, dtype=np.float64)
    if y_obs.shape != (N, H):
        raise ValueError('y_obs must be [N][H] = %r (got %r)' % ((N, H), y_obs.shape))
    if np.isinf(y_obs).any():
        raise ValueError('y_obs holds an infinite value: an observed value must be finite (NaN = not observed)')
    phi = _noise_ar_phi(noise_ar, N, ds_ns)
    levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    quantile_columns(levels)            # (ValueError for a bad level, two levels of one name, too many)
    Q, S = len(levels), int(uncertainty_samples)
    unknown = set(want) - set(SCORE_ROW_FIELDS + SCORE_SERIES_FIELDS)
    if unknown:
        raise ValueError('unknown outputs %s' % sorted(unknown))
    if not Q and set(want) & set(_SCORE_LEVEL_FIELDS):
        raise ValueError('q, pinball, mean_pinball and coverage need quantile levels')
    shapes = {'pit': (N, H), 'crps': (N, H), 'q': (N, Q, H), 'pinball': (N, Q, H), 'mean_crps': (N,),
              'mean_pinball': (N, Q), 'coverage': (N, Q)}
    res = {'yhat': np.zeros((N, H))}
    for k in want:
        res[k] = np.zeros(N, np.int32) if k == 'n_obs' else np.zeros(shapes[k])
    ctx = ctx or get_context()
    L = _lib.load()
    cs = spec.to_c()
    out = _lib.TsfScoreOut(**{k: v.ctypes.data for k, v in res.items()})
    _set_noise_ar(ctx, phi)
    rc = L.tsf_score_actuals(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                             grid.ctypes.data, len(grid), ds_ns.ctypes.data, int(shared), _lib._ptr(floor),
                             _lib._ptr(cap), _lib._ptr(ex), _lib._ptr(key), S, int(seed), y_obs.ctypes.data, Q,
                             levels.ctypes.data if Q else None, ctypes.byref(out))
    ctx.check(rc)
    res['y'] = y_obs
    return res


def score_actuals(spec, theta, y_scale, grid, ds_ns, y_obs, quantiles=(), floor=None, cap=None, extra_future=None,
                  series_key=None, uncertainty_samples=1000, seed=0, ctx=None, noise_ar=None):
    """Observed values scored against the predictive distribution of every series -> Scores (include/tsf.h
    tsf_score_actuals).  ds_ns [H] or [N][H]: the rows that were forecast; y_obs [N][H]: what was observed on them, NaN =
    not observed.  Per row: pit (the probability integral transform: uniform where the distribution is calibrated, in
    steps of 0.5 / uncertainty_samples), crps (the sample CRPS, in the units of y, lower is better) and, with levels
    `quantiles`, q and pinball; per series: n_obs, mean_crps, mean_pinball, coverage (the share of observed rows at or
    below each quantile).  The draws are predict_quantiles' (same series_key, samples, seed, noise_ar): q is its q bit
    for bit."""
    levels = np.array(quantiles, dtype=np.float64).reshape(-1)
    want = ['pit', 'crps', 'n_obs', 'mean_crps'] + (list(_SCORE_LEVEL_FIELDS) if len(levels) else [])
    r = _score_actuals_call(spec, theta, y_scale, grid, ds_ns, y_obs, floor, cap, extra_future, series_key,
                            uncertainty_samples, seed, levels, want, ctx, noise_ar=noise_ar)
    return Scores(r.pop('y'), r.pop('yhat'), levels, **r)


# ---- totals over row windows: quantiles and scores of calendar-period totals ------------------------
# "P10 / P50 / P90 of next week's total, of each calendar month, of every rolling 7-row block" (include/tsf.h "totals
# over row windows"): every draw's rows summed over each window on the device, the sums sorted, and where the rows'
# observed values are given, the observed totals scored against them.  The library sees row indices; which rows make a
# week or a month is decided here, from a calendar (period_windows) or by counting rows (row_windows).

PERIOD_FREQS = ('D', 'W', 'M', 'Q', 'Y')


class Windows(object):
    """K row windows: start, end [K] int32 (row indices, end exclusive, 0 <= start < end) and label_ns [K] int64 or None
    (the first timestamp of each window where they were formed from a calendar).  Windows may overlap, repeat and come
    in any order.  n_rows [K]: the rows in each window -- period_windows does not guess which end periods are complete,
    this is there for the caller to judge."""

    def __init__(self, start, end, label_ns=None):
        start, end = np.asarray(start), np.asarray(end)
        if start.ndim != 1 or start.shape != end.shape or start.dtype.kind not in 'iu' or end.dtype.kind not in 'iu':
            raise ValueError('windows: start and end must be equally long 1-d integer arrays')
        if not 1 <= len(start) <= _lib.MAX_WINDOWS:
            raise ValueError('windows: between 1 and %d windows (got %d)' % (_lib.MAX_WINDOWS, len(start)))
        if (start < 0).any() or (start >= end).any() or end.max() > 2 ** 31 - 1:
            raise ValueError('windows: every window needs 0 <= start < end')
        self.start = np.ascontiguousarray(start, dtype=np.int32)
        self.end = np.ascontiguousarray(end, dtype=np.int32)
        self.label_ns = None if label_ns is None else np.ascontiguousarray(label_ns, dtype=np.int64)
        if self.label_ns is not None and self.label_ns.shape != self.start.shape:
            raise ValueError('windows: label_ns must be as long as start')

    def __len__(self):
        return len(self.start)

    @property
    def n_rows(self):
        return self.end - self.start

    def check(self, H):
        """ValueError where a window ends behind row H"""
        if int(self.end.max()) > H:
            raise ValueError('windows: a window ends at row %d, behind the %d forecast rows' % (int(self.end.max()), H))
        return self


def row_windows(H, width, step=None):
    """Windows by counting rows of an [H] forecast.  Without step: consecutive blocks of `width` rows, the last one
    shorter where width does not divide H.  With step: rolling windows of `width` rows starting every `step` rows, the
    complete ones only."""
    H, width = int(H), int(width)
    if H < 1 or width < 1:
        raise ValueError('row_windows: H and width must be >= 1')
    if step is None:
        start = np.arange(0, H, width)
        return Windows(start, np.minimum(start + width, H))
    if int(step) < 1 or width > H:
        raise ValueError('row_windows: step must be >= 1 and width <= H')
    start = np.arange(0, H - width + 1, int(step))
    return Windows(start, start + width)


def _period_index(ds_ns, freq):
    """the calendar period of every timestamp as an integer that grows with time: days, Monday-based weeks, months,
    quarters or years since 1970"""
    days = np.floor_divide(ds_ns, DAY_NS)
    if freq == 'D':
        return days
    if freq == 'W':
        return np.floor_divide(days + 3, 7)             # 1970-01-01 was a Thursday: the Monday before is day -3
    t = ds_ns.view('datetime64[ns]')
    if freq == 'Y':
        return t.astype('datetime64[Y]').astype(np.int64)
    months = t.astype('datetime64[M]').astype(np.int64)
    return months if freq == 'M' else np.floor_divide(months, 3)


def period_windows(ds_ns, freq):
    """Windows of calendar periods over one shared calendar ds_ns [H] (int64 ns, non-decreasing): freq 'D' | 'W' | 'M' |
    'Q' | 'Y', weeks starting on Monday as pandas' default to_period('W').  A window is a maximal run of consecutive
    rows in one period; label_ns is its first timestamp.  The first and the last period may be incomplete: n_rows says
    how many rows each has.  ValueError for a calendar that is not 1-d (per-series calendars: form row windows per
    series) or decreases somewhere."""
    if freq not in PERIOD_FREQS:
        raise ValueError('freq must be one of %s' % (PERIOD_FREQS,))
    ds = np.asarray(ds_ns)
    if ds.dtype.kind == 'M':
        ds = ds.astype('datetime64[ns]').view(np.int64)
    ds = np.ascontiguousarray(ds, dtype=np.int64)
    if ds.ndim != 1 or len(ds) < 1:
        raise ValueError('period_windows: ds must be one shared calendar [H], H >= 1')
    if (np.diff(ds) < 0).any():
        raise ValueError('period_windows: ds must be non-decreasing')
    p = _period_index(ds, freq)
    start = np.concatenate([[0], np.flatnonzero(np.diff(p)) + 1])
    return Windows(start, np.concatenate([start[1:], [len(ds)]]), ds[start])


def window_totals(y, windows):
    """y [N][H] -> [N][K]: the total of every window, added one row at a time in row order from the window's first row
    (the library's order of adds); NaN where any row of the window is NaN."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError('window_totals: y must be [N][H]')
    windows.check(y.shape[1])
    out = np.empty((y.shape[0], len(windows)))
    for k, (a, b) in enumerate(zip(windows.start, windows.end)):
        c = y[:, a].copy()
        for h in range(a + 1, b):
            c = c + y[:, h]
        out[:, k] = c
    return out


WINDOW_FIELDS = ('total', 'q', 'pit', 'crps', 'pinball', 'n_obs', 'mean_crps', 'mean_pinball', 'coverage')
_WINDOW_SCORE_FIELDS = ('pit', 'crps', 'pinball', 'n_obs', 'mean_crps', 'mean_pinball', 'coverage')


class WindowQuantiles(object):
    """What predict_windows and Rollup.windows return (include/tsf.h tsf_window_out): windows (K of them); ds (the
    calendar [H] or [N][H]); yhat [N][H]; total [N][K] (the sum of yhat over each window); quantiles [Q] (the levels as
    given); q [N][Q][K] or None without levels.  With observed values: y [N][K] (the observed totals, NaN = not
    observed), pit, crps [N][K], pinball [N][Q][K], n_obs [N] (int32), mean_crps [N], mean_pinball, coverage [N][Q];
    None otherwise.  For a roll-up N is the number of groups."""

    def __init__(self, windows, ds, yhat, quantiles, total=None, q=None, y=None, pit=None, crps=None, pinball=None,
                 n_obs=None, mean_crps=None, mean_pinball=None, coverage=None):
        self.windows, self.ds, self.yhat, self.quantiles, self.total, self.q, self.y = windows, ds, yhat, quantiles, total, q, y
        self.pit, self.crps, self.pinball = pit, crps, pinball
        self.n_obs, self.mean_crps, self.mean_pinball, self.coverage = n_obs, mean_crps, mean_pinball, coverage

    def frame(self, n):
        """Series (group) n as a DataFrame, one row per window: period_start, period_end (the timestamps of the window's
        first and last row), n_rows, yhat (the window's total), y, yhat_q<..> per level, pit, crps, pinball_q<..> per
        level; the columns of what was not computed are left out (names: quantile_columns)."""
        import pandas as pd
        w = self.windows
        ds = self.ds if self.ds.ndim == 1 else self.ds[n]
        first = ds[w.start] if w.label_ns is None else w.label_ns
        cols = {'period_start': first.view('datetime64[ns]'), 'period_end': ds[w.end - 1].view('datetime64[ns]'),
                'n_rows': w.n_rows, 'yhat': self.total[n]}
        if self.y is not None:
            cols['y'] = self.y[n]
        if self.q is not None:
            for i, name in enumerate(quantile_columns(self.quantiles)):
                cols[name] = self.q[n, i]
        for k in ('pit', 'crps'):
            if getattr(self, k) is not None:
                cols[k] = getattr(self, k)[n]
        if self.pinball is not None:
            for i, name in enumerate(quantile_columns(self.quantiles, 'pinball_q')):
                cols[name] = self.pinball[n, i]
        return pd.DataFrame(cols, columns=list(cols))


def _window_call_args(windows, H, N, y_win, levels, want):
    """What the two window calls check of their own arguments before the library is loaded -> (levels, y_win, res):
    the outputs named in `want` allocated."""
    if not isinstance(windows, Windows):
        raise ValueError('windows must be a Windows (row_windows, period_windows)')
    windows.check(H)
    K = len(windows)
    levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    quantile_columns(levels)            # (ValueError for a bad level, two levels of one name, too many)
    Q = len(levels)
    unknown = set(want) - set(WINDOW_FIELDS + ('yhat',))
    if unknown:
        raise ValueError('unknown outputs %s' % sorted(unknown))
    if not want:
        raise ValueError('no output wanted')
    if not Q and set(want) & set(_SCORE_LEVEL_FIELDS):
        raise ValueError('q, pinball, mean_pinball and coverage need quantile levels')
    if y_win is None:
        if set(want) & set(_WINDOW_SCORE_FIELDS):
            raise ValueError('pit, crps, pinball and the per-series means need observed values')
    else:
        y_win = np.ascontiguousarray(y_win, dtype=np.float64)
        if y_win.shape != (N, K):
            raise ValueError('y_win must be [N][K] = %r (got %r)' % ((N, K), y_win.shape))
        if np.isinf(y_win).any():
            raise ValueError('an observed window total is infinite: it must be finite (NaN = not observed)')
    shapes = {'yhat': (N, H), 'total': (N, K), 'q': (N, Q, K), 'pit': (N, K), 'crps': (N, K), 'pinball': (N, Q, K),
              'mean_crps': (N,), 'mean_pinball': (N, Q), 'coverage': (N, Q)}
    res = {k: np.zeros(N, np.int32) if k == 'n_obs' else np.zeros(shapes[k]) for k in want}
    return levels, y_win, res


def _predict_windows_call(spec, theta, y_scale, grid, ds_ns, windows, y_win, floor, cap, extra_future, series_key,
                          uncertainty_samples, seed, levels, want, ctx, noise_ar=None):
    """One tsf_predict_windows call -> dict of the outputs named in `want` (any of 'yhat' and WINDOW_FIELDS).  y_win
    [N][K] or None.  Every argument-shape error is raised before the library is loaded."""
    theta, N, y_scale, grid, ds_ns, shared, H, floor, cap, ex, key = _checked_forecast_inputs(
        spec, theta, y_scale, grid, ds_ns, floor, cap, extra_future, series_key)
    levels, y_win, res = _window_call_args(windows, H, N, y_win, levels, want)
    phi = _noise_ar_phi(noise_ar, N, ds_ns)
    Q, S = len(levels), int(uncertainty_samples)
    ctx = ctx or get_context()
    L = _lib.load()
    cs = spec.to_c()
    out = _lib.TsfWindowOut(**{k: v.ctypes.data for k, v in res.items()})
    _set_noise_ar(ctx, phi)
    rc = L.tsf_predict_windows(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                               grid.ctypes.data, len(grid), ds_ns.ctypes.data, int(shared), _lib._ptr(floor),
                               _lib._ptr(cap), _lib._ptr(ex), _lib._ptr(key), S, int(seed), len(windows),
                               windows.start.ctypes.data, windows.end.ctypes.data, _lib._ptr(y_win), Q,
                               levels.ctypes.data if Q else None, ctypes.byref(out))
    ctx.check(rc)
    return res


def _window_want(levels, scored):
    """the outputs of the public window calls: everything the levels and the observed values allow"""
    want = ['yhat', 'total'] + (['q'] if len(levels) else [])
    if scored:
        want += ['pit', 'crps', 'n_obs', 'mean_crps'] + (['pinball', 'mean_pinball', 'coverage'] if len(levels) else [])
    return want


def _observed_totals(y_obs, N, H, windows):
    """y_obs [N][H] (NaN = not observed) -> the observed window totals [N][K]; None for None"""
    if y_obs is None:
        return None
    y_obs = np.asarray(y_obs, dtype=np.float64)
    if y_obs.shape != (N, H):
        raise ValueError('y_obs must be [N][H] = %r (got %r)' % ((N, H), y_obs.shape))
    if np.isinf(y_obs).any():
        raise ValueError('y_obs holds an infinite value: an observed value must be finite (NaN = not observed)')
    return window_totals(y_obs, windows)


def predict_windows(spec, theta, y_scale, grid, ds_future_ns, windows, quantiles, y_obs=None, floor=None, cap=None,
                    extra_future=None, series_key=None, uncertainty_samples=1000, seed=0, ctx=None, noise_ar=None):
    """Quantiles of the TOTAL over each of `windows` (row_windows, period_windows) of the simulated futures of every
    series -> WindowQuantiles (include/tsf.h tsf_predict_windows): yhat [N][H], total [N][K] (the sum of yhat over the
    window), q [N][Q][K] at the levels `quantiles`.  With y_obs [N][H], the values observed on the forecast rows (NaN =
    not observed; a window with such a row is not scored), the observed totals are scored against the distribution of the
    window total: pit, crps, pinball per window, n_obs, mean_crps, mean_pinball, coverage per series.  The draws are
    predict_quantiles' (same series_key, samples, seed, noise_ar): one-row windows give its q bit for bit, windows from
    row 0 its cum_q.  noise_ar (residual_autocorrelation): the remedy where a window total's interval is too narrow
    because the residuals of neighbouring rows move together."""
    levels = np.array(quantiles, dtype=np.float64).reshape(-1)
    theta = np.asarray(theta)
    ds = np.ascontiguousarray(ds_future_ns, dtype=np.int64)
    if not isinstance(windows, Windows):
        raise ValueError('windows must be a Windows (row_windows, period_windows)')
    y_win = _observed_totals(y_obs, theta.shape[0], ds.shape[-1] if ds.ndim else 0, windows)
    r = _predict_windows_call(spec, theta, y_scale, grid, ds, windows, y_win, floor, cap, extra_future, series_key,
                              uncertainty_samples, seed, levels, _window_want(levels, y_win is not None), ctx,
                              noise_ar=noise_ar)
    return WindowQuantiles(windows, ds, r.pop('yhat'), levels, y=y_win, **r)


# ---- serially correlated observation noise: AR(1) per series -----------------------------------------
# The residuals of neighbouring rows of a real fit move together, and the draws' noise is independent from row to row,
# so the spread of a total over several rows (cum_q, a window, a roll-up's running sum) is too narrow (include/tsf.h
# "serially correlated observation noise").  residual_autocorrelation estimates each series' lag-one ROW autocorrelation
# from the fit's own history; noise_ar= on the drawing calls makes every sample's noise an AR(1) chain along its rows.

class NoiseAR(object):
    """What residual_autocorrelation returns, per series: phi [N] (clipped to [0, phi_max]: what noise_ar= takes),
    phi_raw [N] (NaN without pairs), n_pairs [N] int64, scale [N] (the residual root mean square), status [N]
    (_lib.AR_*); the residuals' state at the end of the history (residual_last): last_resid [N] (the last present row's
    residual, y units), last_gap [N] int32 (the rows behind it), and, from fit_residual_autocorrelation, last_ds_ns [N]
    int64 (the date of each series' final history row, present or not; the smallest int64 for an empty series).  The
    last three are None on an object built without them."""

    def __init__(self, phi, phi_raw, n_pairs, scale, status, last_resid=None, last_gap=None, last_ds_ns=None):
        self.phi, self.phi_raw, self.n_pairs, self.scale, self.status = phi, phi_raw, n_pairs, scale, status
        self.last_resid, self.last_gap, self.last_ds_ns = last_resid, last_gap, last_ds_ns

    def conditioned(self, lead=1):
        """What noise_ar= takes for a chain that starts conditioned on the history's last residual (include/tsf.h
        "the conditioned start"): phi, resid = last_resid and steps = last_gap + lead.  lead (an int or [N], >= 1): the
        rows from the end of the history to the first future row -- 1 where the forecast begins at the next row."""
        if self.last_resid is None or self.last_gap is None:
            raise ValueError('this NoiseAR has no last_resid / last_gap (residual_last; residual_autocorrelation fills them)')
        N = len(self.phi)
        lead = np.asarray(lead)
        if lead.ndim > 1 or (lead.ndim == 1 and lead.shape != (N,)) or not np.issubdtype(lead.dtype, np.integer):
            raise ValueError('lead must be an int or [N] ints')
        if (lead < 1).any():
            raise ValueError('lead must be >= 1: the first future row lies behind the history')
        steps = np.asarray(self.last_gap, dtype=np.int64) + lead
        return NoiseARStart(self.phi, self.last_resid, steps, self.last_ds_ns)

    def frame(self, keys=None, last=False):
        """One row per series: series (the index, or `keys` [N]), phi, phi_raw, n_pairs, scale, status; with last=True
        the columns last_resid, last_gap (and last_ds_ns where known) behind them."""
        import pandas as pd
        N = len(self.phi)
        series = np.arange(N, dtype=np.int64) if keys is None else np.asarray(keys)
        if series.shape[0] != N:
            raise ValueError('keys must be [N]')
        cols = {'series': list(series) if series.ndim > 1 else series, 'phi': self.phi, 'phi_raw': self.phi_raw,
                'n_pairs': self.n_pairs, 'scale': self.scale, 'status': self.status}
        if last:
            if self.last_resid is None or self.last_gap is None:
                raise ValueError('this NoiseAR has no last_resid / last_gap')
            cols['last_resid'], cols['last_gap'] = self.last_resid, self.last_gap
            if self.last_ds_ns is not None:
                cols['last_ds_ns'] = self.last_ds_ns
        return pd.DataFrame(cols, columns=list(cols))

    @classmethod
    def from_frame(cls, df):
        """The inverse of frame(keys, last=True), bit for bit: a NoiseAR from the columns phi, phi_raw, n_pairs, scale,
        status, last_resid, last_gap (and last_ds_ns where the frame has it), in the frame's row order.  The `series`
        column is the caller's to join on."""
        need = ('phi', 'phi_raw', 'n_pairs', 'scale', 'status', 'last_resid', 'last_gap')
        missing = [c for c in need if c not in df.columns]
        if missing:
            raise ValueError('from_frame: the frame lacks %s (frame(keys, last=True) writes them)' % ', '.join(missing))
        col = lambda name, dt: np.ascontiguousarray(df[name].to_numpy(), dtype=dt)       # noqa: E731
        return cls(col('phi', np.float64), col('phi_raw', np.float64), col('n_pairs', np.int64), col('scale', np.float64),
                   col('status', np.int32), col('last_resid', np.float64), col('last_gap', np.int32),
                   col('last_ds_ns', np.int64) if 'last_ds_ns' in df.columns else None)


class NoiseARStart(object):
    """NoiseAR.conditioned(): phi [N], resid [N] (y units), steps [N] int32 (>= 1: rows from the last present history
    row to the first future row), last_ds_ns [N] int64 or None -- what noise_ar= takes for the conditioned start."""

    def __init__(self, phi, resid, steps, last_ds_ns=None):
        self.phi = np.ascontiguousarray(phi, dtype=np.float64)
        self.resid = np.ascontiguousarray(resid, dtype=np.float64)
        steps = np.asarray(steps)
        N = len(self.phi)
        if self.phi.shape != (N,) or self.resid.shape != (N,) or steps.shape != (N,):
            raise ValueError('phi, resid and steps must be [N]')
        if not np.isfinite(self.resid).all():
            raise ValueError('resid must be finite')
        if not np.issubdtype(steps.dtype, np.integer) or (steps < 1).any() or (steps > np.iinfo(np.int32).max).any():
            raise ValueError('steps must be integers in [1, 2^31 - 1]')
        self.steps = np.ascontiguousarray(steps, dtype=np.int32)
        self.last_ds_ns = None if last_ds_ns is None else np.ascontiguousarray(last_ds_ns, dtype=np.int64)
        if self.last_ds_ns is not None and self.last_ds_ns.shape != (N,):
            raise ValueError('last_ds_ns must be [N]')


class _NoiseArArmed(object):
    """a checked NoiseARStart on its way to the library (_noise_ar_phi -> _set_noise_ar)"""

    def __init__(self, start):
        self.phi, self.resid, self.steps = start.phi, start.resid, start.steps


def noise_ar_mean(phi, resid, steps, H):
    """The conditional mean [N][H] of the AR(1) noise in y units (include/tsf.h tsf_noise_ar_mean; host only):
    mean[i][0] = resid[i] * phi[i]^steps[i], mean[i][h] = phi[i] * mean[i][h - 1]."""
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    resid = np.ascontiguousarray(resid, dtype=np.float64)
    steps = np.ascontiguousarray(steps, dtype=np.int32)
    N = len(phi)
    if phi.shape != (N,) or resid.shape != (N,) or steps.shape != (N,) or int(H) < 0:
        raise ValueError('phi, resid and steps must be [N], H >= 0')
    mean = np.zeros((N, int(H)))
    if _lib.load().tsf_noise_ar_mean(N, _lib._ptr(phi), _lib._ptr(resid), _lib._ptr(steps), int(H), _lib._ptr(mean)) != 0:
        raise ValueError('tsf_noise_ar_mean: |phi| < 1, finite resid and steps >= 1 are required')
    return mean


def _ar_args(phi_max, min_pairs):
    """tsf_ar_args, refused here as the library refuses them (before it is loaded)."""
    if not 0.0 <= phi_max < 1.0:
        raise ValueError('phi_max must be in [0, 1)')
    if int(min_pairs) != min_pairs or min_pairs < 1:
        raise ValueError('min_pairs must be an integer >= 1')
    a = _lib.TsfArArgs()
    a.phi_max, a.min_pairs, a.reserved_ = float(phi_max), int(min_pairs), 0
    return a


def residual_autocorrelation(y, fitted, offsets=None, phi_max=0.95, min_pairs=8, ctx=None):
    """The lag-one residual autocorrelation of each series (include/tsf.h tsf_residual_autocorr): y [N][T], or 1-D with
    offsets [N+1] (float64 / float32 / int32); fitted: y's shape (each fit's forecast of its own history:
    fitted_history).  Lag one ROW, not one unit of time; uncentred; estimated in sample; phi_raw = (the mean of
    r_t r_{t-1} over the pairs of neighbouring finite rows) / (the mean of r_t^2), phi its clip to [0, phi_max].  Returns
    a NoiseAR."""
    fitted = np.ascontiguousarray(fitted, dtype=np.float64)
    y, offsets, N, T = _screen_panel(y, offsets, (fitted,), ('fitted',))
    if offsets is None and T < 1:
        raise ValueError('aligned panel: y must be [N][T], T >= 1')
    code = _lib.y_dtype_code(y)
    a = _ar_args(phi_max, min_pairs)
    ctx = ctx or get_context()
    phi, raw, scale = np.zeros(N), np.zeros(N), np.zeros(N)
    n_pairs, status = np.zeros(N, np.int64), np.zeros(N, np.int32)
    out = _lib.TsfArOut(phi.ctypes.data, raw.ctypes.data, n_pairs.ctypes.data, scale.ctypes.data, status.ctypes.data)
    last_resid, last_gap, last_status = np.zeros(N), np.zeros(N, np.int32), np.zeros(N, np.int32)
    last = _lib.TsfArLastOut(last_resid.ctypes.data, last_gap.ctypes.data, last_status.ctypes.data)
    # (both kernels on one copy of the panel: tsf_residual_autocorr's outputs bit for bit, and tsf_residual_last's)
    ctx.check(_lib.load().tsf_residual_autocorr_last(ctx.handle, N, T, _lib._ptr(offsets), y.ctypes.data, code,
                                                     fitted.ctypes.data, ctypes.byref(a), ctypes.byref(out), ctypes.byref(last)))
    return NoiseAR(phi, raw, n_pairs, scale, status, last_resid, last_gap)


def residual_last(y, fitted, offsets=None, ctx=None):
    """The residuals' state at the end of each series' history (include/tsf.h tsf_residual_last): y, fitted, offsets as
    residual_autocorrelation takes them -> (last_resid [N], last_gap [N] int32, status [N] int32): the residual of the
    last present (finite) row, the rows behind it, and _lib.AR_OK or _lib.AR_NO_ROW (then +0.0 and the row count)."""
    fitted = np.ascontiguousarray(fitted, dtype=np.float64)
    y, offsets, N, T = _screen_panel(y, offsets, (fitted,), ('fitted',))
    if offsets is None and T < 1:
        raise ValueError('aligned panel: y must be [N][T], T >= 1')
    code = _lib.y_dtype_code(y)
    ctx = ctx or get_context()
    last_resid, last_gap, status = np.zeros(N), np.zeros(N, np.int32), np.zeros(N, np.int32)
    out = _lib.TsfArLastOut(last_resid.ctypes.data, last_gap.ctypes.data, status.ctypes.data)
    ctx.check(_lib.load().tsf_residual_last(ctx.handle, N, T, _lib._ptr(offsets), y.ctypes.data, code, fitted.ctypes.data,
                                            ctypes.byref(out)))
    return last_resid, last_gap, status


def fit_residual_autocorrelation(spec, res, ds_ns, y, offsets=None, floor=None, cap=None, extra=None, phi_max=0.95,
                                 min_pairs=8, ctx=None):
    """residual_autocorrelation of a panel's fits `res` (the FitResult of this panel): fitted is predict on the
    history's own dates (fitted_history), aligned ds_ns [T] or ragged with offsets.  last_resid and last_gap come from
    the same fitted (one more launch), last_ds_ns from ds_ns: the date of each series' final history row."""
    fitted = fitted_history(spec, res, ds_ns, offsets, floor, cap, extra, ctx=ctx)
    est = residual_autocorrelation(y, fitted, offsets, phi_max=phi_max, min_pairs=min_pairs, ctx=ctx)
    ds = np.asarray(ds_ns, dtype=np.int64)
    N = len(est.phi)
    if offsets is None:
        est.last_ds_ns = np.full(N, ds[-1], dtype=np.int64)
    else:
        off = np.asarray(offsets, dtype=np.int64)
        est.last_ds_ns = np.full(N, np.iinfo(np.int64).min, dtype=np.int64)
        some = off[1:] > off[:-1]
        est.last_ds_ns[some] = ds[off[1:][some] - 1]
    return est


def fit_noise_state(spec, res, ds_ns, y, offsets=None, floor=None, cap=None, extra=None, excluded=None, phi_max=0.95,
                    min_pairs=8, ctx=None):
    """fit_residual_autocorrelation's NoiseAR, field by field and bit for bit, in one launch (include/tsf.h
    tsf_noise_state): the panel as fit_aligned (ds_ns [T], y [N][T], extra [n_extra][T]) or, with offsets [N+1], as
    fit_ragged took it, and its FitResult `res`.  The fitted values are formed row by row on the device and never
    stored; nothing of the panel's size comes back.  excluded (uint8 / bool, y's shape; 1 = the row is absent, as if y
    were NaN there): a screened fit summarised on the rows its final fit saw (ScreenedFit.screen.flag).  A series whose
    fit status is negative has no fitted values: phi 0, AR_NO_PAIRS, no last row, last_gap = its row count."""
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.uint8)
    y, offsets, N, T = _screen_panel(y, offsets, (ex,), ('excluded',))
    if offsets is None and T < 1:
        raise ValueError('aligned panel: y must be [N][T], T >= 1')
    ds = np.ascontiguousarray(ds_ns, dtype=np.int64)
    rows = T if offsets is None else y.shape[0]
    if ds.shape != (rows,):
        raise ValueError('ds must be [T] (aligned) or [total_rows] (ragged)')
    a = _ar_args(phi_max, min_pairs)
    theta = np.ascontiguousarray(res.theta, dtype=np.float64)
    y_scale = np.ascontiguousarray(res.y_scale, dtype=np.float64)
    grid = np.ascontiguousarray(res.grid, dtype=_lib.GRID_DTYPE)
    status = np.ascontiguousarray(res.status, dtype=np.int32)
    if theta.shape != (N, spec.theta_stride) or y_scale.shape != (N,) or status.shape != (N,) or len(grid) not in (1, N):
        raise ValueError('res must be the FitResult of this panel: theta [N][stride], y_scale, status [N], grid [1] or [N]')
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    xt = None
    if spec.extra:
        xt = np.ascontiguousarray(extra, dtype=np.float64)
        if xt.shape != (len(spec.extra), rows):
            raise ValueError('extra must be [n_extra][len(ds)]')
    ctx = ctx or get_context()
    cs = spec.to_c()
    phi, raw, scale, last_resid = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    n_pairs, last_ds = np.zeros(N, np.int64), np.zeros(N, np.int64)
    st, last_gap, last_status = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    out = _lib.TsfNoiseStateOut(phi.ctypes.data, raw.ctypes.data, n_pairs.ctypes.data, scale.ctypes.data, st.ctypes.data,
                                last_resid.ctypes.data, last_gap.ctypes.data, last_status.ctypes.data, last_ds.ctypes.data)
    ctx.check(_lib.load().tsf_noise_state(ctx.handle, ctypes.byref(cs), N, T, _lib._ptr(offsets), ds.ctypes.data,
                                          y.ctypes.data, _lib.y_dtype_code(y), _lib._ptr(fl), _lib._ptr(cp), _lib._ptr(xt),
                                          theta.ctypes.data, y_scale.ctypes.data, grid.ctypes.data, len(grid),
                                          status.ctypes.data, _lib._ptr(ex), ctypes.byref(a), ctypes.byref(out)))
    return NoiseAR(phi, raw, n_pairs, scale, st, last_resid, last_gap, last_ds)


def predict_conditioned(spec, theta, y_scale, grid, ds_future_ns, start, floor=None, cap=None, extra_future=None,
                        want_int=True, ctx=None):
    """The corrected point forecast with its integer column (include/tsf.h tsf_predict_conditioned): start, a
    NoiseAR.conditioned() object -> (yhat, yhat_int) with want_int, else yhat.  yhat has the bits of
    predict(noise_ar=start); yhat_int is the reference's post-step (truncate, saturate, clamp to floor) on that
    corrected value -- what predict refuses to give, its integer column being the uncorrected forecast's.  A series
    with phi == 0 gets predict(want_int=True)'s two outputs."""
    if not isinstance(start, NoiseARStart):
        raise ValueError('start must be a NoiseAR.conditioned() object')
    theta, N, y_scale, grid, ds, shared, H, floor, cap, ex, _ = _forecast_inputs(
        spec, theta, y_scale, grid, ds_future_ns, floor, cap, extra_future)
    if start.phi.shape != (N,):
        raise ValueError('start must hold N series')
    if not (np.isfinite(start.phi).all() and (np.abs(start.phi) < 1.0).all()):
        raise ValueError('noise_ar values must be finite with |phi| < 1')
    if start.last_ds_ns is not None and H and (ds[..., 0] <= start.last_ds_ns).any():
        raise ValueError('a conditioned noise_ar needs future rows after the history: a first future row lies at or '
                         'before last_ds_ns')
    ctx = ctx or get_context()
    cs = spec.to_c()
    yhat = np.zeros((N, H))
    yint = np.zeros((N, H), dtype=np.int32) if want_int else None
    ctx.check(_lib.load().tsf_predict_conditioned(ctx.handle, ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data,
                                                  grid.ctypes.data, len(grid), ds.ctypes.data, int(shared), _lib._ptr(floor),
                                                  _lib._ptr(cap), _lib._ptr(ex), start.phi.ctypes.data,
                                                  start.resid.ctypes.data, start.steps.ctypes.data, yhat.ctypes.data,
                                                  _lib._ptr(yint)))
    return (yhat, yint) if want_int else yhat


def noise_lead(last_ds_ns, row_step_ns, ds_future_ns):
    """(lead [N] int64, ok [N] bool): the rows from the end of each history to its first future row -- what
    NoiseAR.conditioned(lead=) takes -- where the future continues the history's row grid.  last_ds_ns, row_step_ns [N];
    ds_future_ns [H] (shared) or [N][H].  ok: row_step_ns > 0, the series' future rows uniformly spaced by its
    row_step_ns, and the first one a positive whole number of steps after last_ds_ns; lead is that number (0 where not
    ok).  The chain runs on rows: a weekly forecast of a daily history is not ok.  Pure numpy."""
    last = np.asarray(last_ds_ns, dtype=np.int64).reshape(-1)
    step = np.asarray(row_step_ns, dtype=np.int64).reshape(-1)
    N = len(last)
    fut = np.asarray(ds_future_ns, dtype=np.int64)
    if step.shape != (N,) or fut.ndim not in (1, 2) or fut.shape[-1] < 1 or (fut.ndim == 2 and fut.shape[0] != N):
        raise ValueError('last_ds_ns, row_step_ns must be [N], ds_future [H] or [N][H] with H >= 1')
    fut = np.broadcast_to(fut, (N, fut.shape[-1]))
    ok = (step > 0) & (last != np.iinfo(np.int64).min)
    ok &= (np.diff(fut, axis=1) == step[:, None]).all(axis=1)
    first = fut[:, 0]
    ok &= first > last                                      # (compared first: the difference below cannot wrap)
    ahead = np.where(ok, first - np.where(ok, last, first), 0)
    safe = np.where(ok, step, 1)
    ok &= ahead % safe == 0
    return np.where(ok, ahead // safe, 0).astype(np.int64), ok


def _noise_ar_phi(noise_ar, N, ds_future_ns):
    """phi [N] of a noise_ar= keyword (an array or a NoiseAR), or None; every error is a ValueError raised here.  The
    chain runs in row order, so with it the future rows of every series must be strictly increasing."""
    if noise_ar is None:
        return None
    if isinstance(noise_ar, NoiseARStart):
        phi = _noise_ar_phi(noise_ar.phi, N, ds_future_ns)
        if noise_ar.last_ds_ns is not None:
            ds = np.asarray(ds_future_ns, dtype=np.int64)
            first = ds[..., 0] if ds.ndim and ds.shape[-1] else None
            if first is not None and (first <= noise_ar.last_ds_ns).any():
                raise ValueError('a conditioned noise_ar needs future rows after the history: a first future row lies at or '
                                 'before last_ds_ns')
        return _NoiseArArmed(noise_ar)
    phi = noise_ar.phi if isinstance(noise_ar, NoiseAR) else noise_ar
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    if phi.shape != (N,):
        raise ValueError('noise_ar must be [N] (or a NoiseAR of N series)')
    if not (np.isfinite(phi).all() and (np.abs(phi) < 1.0).all()):
        raise ValueError('noise_ar values must be finite with |phi| < 1')
    ds = np.asarray(ds_future_ns, dtype=np.int64)
    if ds.ndim and ds.shape[-1] > 1 and not (np.diff(ds, axis=-1) > 0).all():
        raise ValueError('noise_ar needs strictly increasing future rows per series: the chain is row-ordered')
    return phi


def _set_noise_ar(ctx, phi):
    """tsf_set_noise_ar for the library call that follows at once (the setting is consumed by it); None: nothing."""
    if isinstance(phi, _NoiseArArmed):
        a = phi
        ctx.check(_lib.load().tsf_set_noise_ar(ctx.handle, a.phi.ctypes.data, len(a.phi)))
        ctx.check(_lib.load().tsf_set_noise_ar_start(ctx.handle, a.resid.ctypes.data, a.steps.ctypes.data, len(a.phi)))
    elif phi is not None:
        ctx.check(_lib.load().tsf_set_noise_ar(ctx.handle, phi.ctypes.data, len(phi)))


# ---- group roll-ups: predictive quantiles of sums over series --------------------------------------
# The distribution of a total over several series (include/tsf.h "group roll-ups"): the members' draws summed sample by
# sample on the device, across specs and calls, then sorted.  By default members are taken as independent given their
# fits: where their errors are positively correlated in reality the spread is too narrow.  residual_correlation
# estimates each group's correlation from the fits' history and Rollup(noise_corr=) draws with it.

def rollup_groups(labels):
    """Group labels -> (unique_sorted_labels, dense_index int64 [N]): the `group` argument of Rollup.add.  labels: one
    integer array [N], or a tuple of them (a group per distinct combination; the unique labels are then [G][len(tuple)],
    sorted by the first array, then the second, ...).  Pure numpy."""
    if isinstance(labels, tuple):
        cols = [np.asarray(a) for a in labels]
        if not cols or any(c.ndim != 1 or c.shape != cols[0].shape for c in cols):
            raise ValueError('labels: a tuple of equally long 1-d integer arrays')
        lab = np.stack(cols, axis=1)
    else:
        lab = np.asarray(labels)
        if lab.ndim != 1:
            raise ValueError('labels: a 1-d integer array or a tuple of them')
    if lab.size and lab.dtype.kind not in 'iu':
        raise ValueError('labels must be integers')
    if lab.shape[0] == 0:
        return lab.astype(np.int64), np.zeros(0, dtype=np.int64)
    uniq, inv = np.unique(lab, axis=0, return_inverse=True)
    return uniq, np.ascontiguousarray(inv, dtype=np.int64).reshape(-1)


class RollupQuantiles(object):
    """What Rollup.quantiles returns: yhat [G][H] (the sum of the members' yhat); count [G] (members added); quantiles [Q]
    (the levels as given); q [G][Q][H]; cum_q [G][Q][H] or None."""

    def __init__(self, yhat, count, quantiles, q, cum_q=None):
        self.yhat, self.count, self.quantiles, self.q, self.cum_q = yhat, count, quantiles, q, cum_q

    def frame(self, g, ds):
        """Group g as a DataFrame: ds, yhat, yhat_q<..> per level, then yhat_cum_q<..> where computed (names:
        quantile_columns)."""
        import pandas as pd
        ds = np.asarray(ds)
        if ds.dtype.kind != 'M':
            ds = ds.astype(np.int64).view('datetime64[ns]')
        cols = {'ds': ds, 'yhat': self.yhat[g]}
        for prefix, arr in (('yhat_q', self.q), ('yhat_cum_q', self.cum_q)):
            if arr is not None:
                for i, name in enumerate(quantile_columns(self.quantiles, prefix)):
                    cols[name] = arr[g, i]
        return pd.DataFrame(cols, columns=list(cols))


class NoiseCorrelation(object):
    """What residual_correlation returns: per group rho [G] (clipped to [0, rho_max]: what Rollup(noise_corr=) takes),
    rho_raw [G] (NaN without pairs), n_pairs [G] int64, n_used [G] int32, status [G] (_lib.CORR_*); per series scale [N]
    (the residual root mean square; NaN: the series is unused)."""

    def __init__(self, rho, rho_raw, n_pairs, n_used, status, scale):
        self.rho, self.rho_raw, self.n_pairs, self.n_used, self.status, self.scale = rho, rho_raw, n_pairs, n_used, status, scale

    def frame(self, labels=None):
        """One row per group: group (the dense index, or `labels` [G]: rollup_groups' unique labels), rho, rho_raw,
        n_pairs, n_used, status."""
        import pandas as pd
        G = len(self.rho)
        group = np.arange(G, dtype=np.int64) if labels is None else np.asarray(labels)
        if group.shape[0] != G:
            raise ValueError('labels must be [n_groups]')
        cols = {'group': list(group) if group.ndim > 1 else group, 'rho': self.rho, 'rho_raw': self.rho_raw,
                'n_pairs': self.n_pairs, 'n_used': self.n_used, 'status': self.status}
        return pd.DataFrame(cols, columns=list(cols))


def _corr_args(rho_max, min_rows):
    """tsf_corr_args, refused here as the library refuses them (before it is loaded)."""
    if not 0.0 <= rho_max <= 1.0:
        raise ValueError('rho_max must be in [0, 1]')
    if int(min_rows) != min_rows or min_rows < 2:
        raise ValueError('min_rows must be an integer >= 2')
    a = _lib.TsfCorrArgs()
    a.rho_max, a.min_rows, a.reserved_ = float(rho_max), int(min_rows), 0
    return a


def residual_correlation(y, fitted, group, n_groups, rho_max=0.95, min_rows=8, ctx=None):
    """The residual correlation of each group (include/tsf.h tsf_residual_corr) of an aligned panel: y [N][T] (float64 /
    float32 / int32), fitted [N][T] (each fit's forecast of its own history: fitted_history), group [N] dense indices in
    [0, n_groups) or -1 for a series that takes no part.  Per series the residuals are standardised by their root mean
    square over the finite rows; per group rho_raw is the mean of e_i e_j over the member pairs and rows where both are
    present, rho its clip to [0, rho_max].  Returns a NoiseCorrelation."""
    y = np.ascontiguousarray(y)
    if y.ndim != 2 or y.shape[1] < 1:
        raise ValueError('y must be [N][T], T >= 1 (aligned panels only)')
    N, T = y.shape
    fitted = np.ascontiguousarray(fitted, dtype=np.float64)
    if fitted.shape != y.shape:
        raise ValueError('fitted must have the shape of y')
    G = int(n_groups)
    if G < 1:
        raise ValueError('n_groups must be >= 1')
    group = np.ascontiguousarray(group, dtype=np.int64)
    if group.shape != (N,):
        raise ValueError('group must be [N]')
    if N and (group.min() < -1 or group.max() >= G):
        raise ValueError('group values must be in [-1, %d)' % G)
    code = _lib.y_dtype_code(y)
    a = _corr_args(rho_max, min_rows)
    ctx = ctx or get_context()
    rho, raw, scale = np.zeros(G), np.zeros(G), np.zeros(N)
    n_pairs, n_used, status = np.zeros(G, np.int64), np.zeros(G, np.int32), np.zeros(G, np.int32)
    out = _lib.TsfCorrOut(rho.ctypes.data, raw.ctypes.data, n_pairs.ctypes.data, n_used.ctypes.data, status.ctypes.data,
                          scale.ctypes.data)
    ctx.check(_lib.load().tsf_residual_corr(ctx.handle, N, T, y.ctypes.data, code, fitted.ctypes.data, group.ctypes.data, G,
                                            ctypes.byref(a), ctypes.byref(out)))
    return NoiseCorrelation(rho, raw, n_pairs, n_used, status, scale)


def fit_residual_correlation(spec, res, ds_ns, y, group, n_groups, floor=None, cap=None, extra=None, rho_max=0.95,
                             min_rows=8, ctx=None):
    """residual_correlation of an aligned panel's fits `res` (fit_aligned's FitResult of this panel): fitted is predict on
    the history's own dates ds_ns [T] (fitted_history)."""
    fitted = fitted_history(spec, res, ds_ns, None, floor, cap, extra, ctx=ctx)
    return residual_correlation(y, fitted, group, n_groups, rho_max=rho_max, min_rows=min_rows, ctx=ctx)


def _noise_corr_args(noise_corr, group_key, G):
    """(rho [G], group_key [G] or None) of Rollup(noise_corr=, group_key=); every error is a ValueError raised here."""
    rho = noise_corr.rho if isinstance(noise_corr, NoiseCorrelation) else noise_corr
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    if rho.shape != (G,):
        raise ValueError('noise_corr must be [n_groups] (or a NoiseCorrelation of n_groups groups)')
    if not (np.isfinite(rho).all() and rho.min() >= 0.0 and rho.max() <= 1.0):
        raise ValueError('noise_corr values must be finite and in [0, 1]')
    if group_key is not None:
        group_key = np.ascontiguousarray(group_key, dtype=np.int64)
        if group_key.shape != (G,):
            raise ValueError('group_key must be [n_groups]')
    return rho, group_key


def _rollup_add_args(spec, theta, y_scale, grid, group, series_key, floor, cap, extra_future, G, H):
    """The arguments of one Rollup.add as the library takes them; every shape error is a ValueError raised here, before
    the library is touched."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.ndim != 2:
        raise ValueError('theta must be [N][stride]')
    N = theta.shape[0]
    if series_key is None:
        raise ValueError('series_key is required: the index-in-call default would give two add calls the same streams')
    key = np.ascontiguousarray(series_key, dtype=np.int64)
    if key.shape != (N,):
        raise ValueError('series_key must be [N]')
    group = np.ascontiguousarray(group, dtype=np.int64)
    if group.shape != (N,):
        raise ValueError('group must be [N]')
    if N and (group.min() < 0 or group.max() >= G):
        raise ValueError('group values must be in [0, %d)' % G)
    y_scale = np.ascontiguousarray(y_scale, dtype=np.float64)
    if y_scale.shape != (N,):
        raise ValueError('y_scale must be [N]')
    grid = np.ascontiguousarray(grid, dtype=_lib.GRID_DTYPE)
    floor = _opt_f64(floor, N, 'floor')
    cap = _opt_f64(cap, N, 'cap')
    ex, shared = None, 1
    if spec.extra:
        if extra_future is None:
            raise ValueError('extra_future is required: the spec has extra columns')
        ex = np.ascontiguousarray(extra_future, dtype=np.float64)
        shared = int(ex.ndim == 2)
        shape = (len(spec.extra), H) if shared else (N, len(spec.extra), H)
        if ex.shape != shape:
            raise ValueError('extra_future must be [n_extra][H] or [N][n_extra][H]')
    return N, theta, y_scale, grid, group, key, floor, cap, ex, shared


def _rollup_c_args(spec, args):
    """What tsf_rollup_add, tsf_rollup_set_totals and tsf_rollup_reconcile take behind the handle, from
    _rollup_add_args' tuple (whose arrays the caller keeps alive over the call)."""
    N, theta, y_scale, grid, group, key, floor, cap, ex, shared = args
    cs = spec.to_c()
    return (ctypes.byref(cs), N, theta.ctypes.data, y_scale.ctypes.data, grid.ctypes.data, len(grid), _lib._ptr(floor),
            _lib._ptr(cap), _lib._ptr(ex), shared, key.ctypes.data, group.ctypes.data)


class Rollup(object):
    """One tsf_rollup: n_groups accumulators of uncertainty_samples summed draws per row of ds_future_ns [H], filled by
    add (once per spec, any number of calls) and read by quantiles / samples at any time.  A context manager; close()
    frees the device memory (before its context is closed).  Shape and level errors raise ValueError before the library
    is touched.  Where the totals are fitted directly as well: set_totals, then reconcile (the members) and
    reconciled_totals (include/tsf.h "reconciliation"); with levels above the groups: set_tree, set_node_totals,
    solve_tree, then reconcile_tree and tree_totals (include/tsf.h "tree reconciliation").  noise_corr: rho [n_groups] in [0, 1] or a NoiseCorrelation
    (residual_correlation) -- the members' observation noise is then drawn with that correlation within each group
    (include/tsf.h "correlated group roll-ups"; group_key [n_groups]: the keys of the groups' factor streams, default the
    group index); such a roll-up cannot be reconciled.  None: the members are independent, as always."""

    def __init__(self, ds_future_ns, n_groups, uncertainty_samples=1000, seed=0, ctx=None, noise_corr=None, group_key=None):
        self._h = None
        ds = np.ascontiguousarray(ds_future_ns, dtype=np.int64)
        if ds.ndim != 1 or ds.shape[0] < 1:
            raise ValueError('ds_future must be [H], H >= 1: a roll-up has one calendar')
        if int(n_groups) < 1:
            raise ValueError('n_groups must be >= 1')
        if not 2 <= int(uncertainty_samples) <= 4096:
            raise ValueError('uncertainty_samples must be in [2, 4096]')
        self.ds_future_ns, self.G, self.H, self.S = ds, int(n_groups), ds.shape[0], int(uncertainty_samples)
        self.seed = int(seed)
        if noise_corr is None and group_key is not None:
            raise ValueError('group_key without noise_corr')
        corr = None if noise_corr is None else _noise_corr_args(noise_corr, group_key, self.G)
        self._has_corr = False
        self._tree_set = None
        self._ctx = ctx or get_context()
        h = ctypes.c_void_p()
        self._ctx.check(_lib.load().tsf_rollup_create(self._ctx.handle, self.G, self.H, ds.ctypes.data, self.S, self.seed,
                                                      ctypes.byref(h)))
        self._h = h
        if corr is not None:
            self.set_noise_corr(*corr)

    def set_noise_corr(self, rho, group_key=None):
        """tsf_rollup_set_noise_corr: rho [n_groups] in [0, 1] (or a NoiseCorrelation), before anything is added."""
        h = self._handle()
        rho, group_key = _noise_corr_args(rho, group_key, self.G)
        self._ctx.check(_lib.load().tsf_rollup_set_noise_corr(h, rho.ctypes.data, _lib._ptr(group_key)))
        self._has_corr = True

    def _handle(self):
        if not self._h:
            raise ValueError('the roll-up is closed')
        return self._h

    def close(self):
        if getattr(self, '_h', None):
            _lib.load().tsf_rollup_free(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, spec, theta, y_scale, grid, group, series_key, floor=None, cap=None, extra_future=None, noise_ar=None):
        """Adds N series of one spec: group [N] (dense indices in [0, n_groups): rollup_groups), series_key [N]
        (required: the streams of two add calls must differ; the scorer's is (series_id << 32) ^ dim_id).  extra_future:
        [n_extra][H] shared by the series, or [N][n_extra][H].  noise_ar: phi [N] or a NoiseAR -- these members' draws
        chain their observation noise along the rows (residual_autocorrelation); not on a roll-up with noise_corr."""
        h = self._handle()
        args = _rollup_add_args(spec, theta, y_scale, grid, group, series_key, floor, cap, extra_future, self.G, self.H)
        if noise_ar is not None and self._has_corr:
            raise ValueError('noise_ar on a roll-up with noise_corr: the correlated add regenerates the independent noise')
        _set_noise_ar(self._ctx, _noise_ar_phi(noise_ar, args[0], self.ds_future_ns))
        self._ctx.check(_lib.load().tsf_rollup_add(h, *_rollup_c_args(spec, args)))

    def _group_outs(self, Q, want, n=None):
        """-> (dict of a tsf_rollup_out's arrays: yhat, count and those of q, cum_q, samples named in `want`; the struct);
        n: the number of groups or nodes read (None: n_groups)"""
        n = self.G if n is None else n
        res = {'yhat': np.zeros((n, self.H)), 'count': np.zeros(n, dtype=np.int64)}
        for k in ('q', 'cum_q'):
            if k in want:
                res[k] = np.zeros((n, Q, self.H))
        if 'samples' in want:
            res['samples'] = np.zeros((n, self.H, self.S))
        return res, _lib.TsfRollupOut(**{k: v.ctypes.data for k, v in res.items()})

    def _read(self, levels, want):
        h = self._handle()
        levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        Q = len(levels)
        res, out = self._group_outs(Q, want)
        self._ctx.check(_lib.load().tsf_rollup_quantiles(h, Q, levels.ctypes.data if Q else None, ctypes.byref(out)))
        return res

    def quantiles(self, levels, cumulative=False):
        """-> RollupQuantiles at the levels (in [0, 1]) of what has been added so far; with cumulative, cum_q: the same
        levels of each summed sample's running sum over the rows.  The accumulators are not modified."""
        self._handle()
        quantile_columns(levels)                # (a bad level list: ValueError before the library is touched)
        levels = np.array(levels, dtype=np.float64).reshape(-1)
        if len(levels) == 0:
            raise ValueError('at least one quantile level')
        r = self._read(levels, ['q'] + (['cum_q'] if cumulative else []))
        return RollupQuantiles(r['yhat'], r['count'], levels, r['q'], r.get('cum_q'))

    def samples(self):
        """-> [G][H][S]: the summed draws themselves (sample s of a group: the sum of sample s of its members)."""
        return self._read([], ['samples'])['samples']

    def _windows_call(self, windows, y_win, levels, want):
        """One tsf_rollup_windows call -> dict of the outputs named in `want` (any of 'yhat' and WINDOW_FIELDS); y_win
        [G][K] or None.  Every argument-shape error is raised before the library is called."""
        h = self._handle()
        levels, y_win, res = _window_call_args(windows, self.H, self.G, y_win, levels, want)
        Q = len(levels)
        out = _lib.TsfWindowOut(**{k: v.ctypes.data for k, v in res.items()})
        self._ctx.check(_lib.load().tsf_rollup_windows(h, len(windows), windows.start.ctypes.data, windows.end.ctypes.data,
                                                       _lib._ptr(y_win), Q, levels.ctypes.data if Q else None,
                                                       ctypes.byref(out)))
        return res

    def windows(self, windows, quantiles, y_obs=None):
        """-> WindowQuantiles of the group totals over each of `windows` (row_windows, period_windows of the roll-up's
        calendar) from what has been added so far, a group in the place of a series; with y_obs [G][H], the observed
        group totals per row (NaN = not observed), scored as predict_windows scores a series.  The accumulators are not
        modified."""
        levels = np.array(quantiles, dtype=np.float64).reshape(-1)
        if not isinstance(windows, Windows):
            raise ValueError('windows must be a Windows (row_windows, period_windows)')
        y_win = _observed_totals(y_obs, self.G, self.H, windows)
        r = self._windows_call(windows, y_win, levels, _window_want(levels, y_win is not None))
        return WindowQuantiles(windows, self.ds_future_ns, r.pop('yhat'), levels, y=y_win, **r)

    # -- reconciliation (include/tsf.h "reconciliation") --

    def set_totals(self, spec, theta, y_scale, grid, group, series_key, floor=None, cap=None, extra_future=None):
        """The directly fitted totals of one spec: series n is the total of group[n] (at most one total per group, over
        all calls).  Forecast on the roll-up's calendar like the members of add; series_key [Gt] is required and must
        differ from every member's key (a shared key is a shared stream)."""
        h = self._handle()
        args = _rollup_add_args(spec, theta, y_scale, grid, group, series_key, floor, cap, extra_future, self.G, self.H)
        N, group = args[0], args[4]
        if len(np.unique(group)) != N:
            raise ValueError('group: a group appears twice (one total per group)')
        self._ctx.check(_lib.load().tsf_rollup_set_totals(h, *_rollup_c_args(spec, args)))

    def reconcile(self, spec, theta, y_scale, grid, group, series_key, share, quantiles=(), cumulative=False,
                  samples=False, floor=None, cap=None, extra_future=None):
        """The second pass over members that were added (same arguments and keys as in add), after every add and
        set_totals: draw' = draw + share[n] * (total's draw - sum of the group's member draws) -> Reconciled (a
        Quantiles: yhat [N][H], q and cum_q [N][Q][H] at the levels `quantiles`; .samples [N][H][S] where asked for).
        share [N] in [0, 1] (reconcile_shares); a group without a total leaves its members as they are."""
        return self._second_pass('tsf_rollup_reconcile', spec, theta, y_scale, grid, group, series_key, share, quantiles,
                                 cumulative, samples, floor, cap, extra_future)

    def _second_pass(self, entry, spec, theta, y_scale, grid, group, series_key, share, quantiles, cumulative, samples,
                     floor, cap, extra_future):
        """reconcile and reconcile_tree: the checks, the outputs and the call of `entry`, which take the same arguments"""
        h = self._handle()
        args = _rollup_add_args(spec, theta, y_scale, grid, group, series_key, floor, cap, extra_future, self.G, self.H)
        N = args[0]
        share = np.ascontiguousarray(share, dtype=np.float64)
        if share.shape != (N,):
            raise ValueError('share must be [N]')
        if N and not (np.isfinite(share).all() and share.min() >= 0.0 and share.max() <= 1.0):
            raise ValueError('share values must be finite and in [0, 1]')
        quantile_columns(quantiles)             # (a bad level list: ValueError before the library is touched)
        levels = np.array(quantiles, dtype=np.float64).reshape(-1)
        Q = len(levels)
        if Q == 0 and (cumulative or not samples):
            raise ValueError('nothing requested: give quantile levels or samples=True (cumulative needs levels)')
        res = {'yhat': np.zeros((N, self.H))}
        if Q:
            res['q'] = np.zeros((N, Q, self.H))
            if cumulative:
                res['cum_q'] = np.zeros((N, Q, self.H))
        if samples:
            res['samples'] = np.zeros((N, self.H, self.S))
        out = _lib.TsfReconcileOut(**{k: v.ctypes.data for k, v in res.items()})
        self._ctx.check(getattr(_lib.load(), entry)(h, *_rollup_c_args(spec, args), share.ctypes.data, Q,
                                                    levels.ctypes.data if Q else None, ctypes.byref(out)))
        return Reconciled(res['yhat'], levels, res.get('q'), res.get('cum_q'), res.get('samples'))

    def reconciled_totals(self, share_total, levels, cumulative=False, samples=False):
        """-> RollupQuantiles of acc + share_total[g] * (total's draws - acc) per group (share_total [G] in [0, 1]:
        reconcile_shares); with samples, (RollupQuantiles, [G][H][S]).  The accumulators are not modified."""
        h = self._handle()
        mu = np.ascontiguousarray(share_total, dtype=np.float64)
        if mu.shape != (self.G,):
            raise ValueError('share_total must be [n_groups]')
        if not (np.isfinite(mu).all() and mu.min() >= 0.0 and mu.max() <= 1.0):
            raise ValueError('share_total values must be finite and in [0, 1]')
        quantile_columns(levels)
        levels = np.array(levels, dtype=np.float64).reshape(-1)
        Q = len(levels)
        if Q == 0:
            raise ValueError('at least one quantile level')
        res, out = self._group_outs(Q, ['q'] + (['cum_q'] if cumulative else []) + (['samples'] if samples else []))
        self._ctx.check(_lib.load().tsf_rollup_reconciled_totals(h, mu.ctypes.data, Q, levels.ctypes.data, ctypes.byref(out)))
        r = RollupQuantiles(res['yhat'], res['count'], levels, res['q'], res.get('cum_q'))
        return (r, res['samples']) if samples else r

    # -- tree reconciliation (include/tsf.h "tree reconciliation") --

    def _tree(self):
        if self._tree_set is None:
            raise ValueError('the roll-up has no tree: set_tree first')
        return self._tree_set

    def set_tree(self, tree):
        """Declares the levels above the groups: a RollupTree (rollup_tree) whose level 1 is this roll-up's n_groups.
        Once per roll-up; not on a roll-up with noise_corr."""
        h = self._handle()
        if not isinstance(tree, RollupTree):
            raise ValueError('tree must be a RollupTree (rollup_tree)')
        if self._tree_set is not None:
            raise ValueError('the roll-up has a tree already')
        if self._has_corr:
            raise ValueError('a tree on a roll-up with noise_corr: correlated draws are not reconciled')
        if tree.n_nodes[0] != self.G:
            raise ValueError('the tree has %d groups, the roll-up %d' % (tree.n_nodes[0], self.G))
        if tree.n_levels < 2:
            raise ValueError('a tree needs at least one level above the groups')
        n_nodes = np.ascontiguousarray(tree.n_nodes[1:], dtype=np.int64)
        parent = np.ascontiguousarray(np.concatenate(tree.parent), dtype=np.int64)
        self._ctx.check(_lib.load().tsf_rollup_set_tree(h, len(n_nodes), n_nodes.ctypes.data, parent.ctypes.data))
        self._tree_set = tree

    def set_node_totals(self, level, spec, theta, y_scale, grid, node, series_key, floor=None, cap=None,
                        extra_future=None):
        """The directly fitted totals of nodes of one level in [2, L] (level 1: set_totals): series n is the total of
        node[n] of that level (at most one total per node, over all calls); series_key [Gt] is required and must differ
        from every other key of the hierarchy."""
        h = self._handle()
        tree = self._tree()
        if not 2 <= int(level) <= tree.n_levels:
            raise ValueError('level must be in [2, %d] (level 1: set_totals)' % tree.n_levels)
        args = _rollup_add_args(spec, theta, y_scale, grid, node, series_key, floor, cap, extra_future,
                                tree.n_nodes[int(level) - 1], self.H)
        if len(np.unique(args[4])) != args[0]:
            raise ValueError('node: a node appears twice (one total per node)')
        self._ctx.check(_lib.load().tsf_rollup_set_node_totals(h, int(level), *_rollup_c_args(spec, args)))

    def solve_tree(self, shares):
        """The two sweeps over what has been added, with a TreeShares (reconcile_tree_shares) of this tree, after every
        add, set_totals and set_node_totals.  Any of those afterwards invalidates it."""
        h = self._handle()
        tree = self._tree()
        if not isinstance(shares, TreeShares):
            raise ValueError('shares must be a TreeShares (reconcile_tree_shares)')
        mu, kappa = np.concatenate(shares.mu), np.concatenate(shares.kappa)
        if [len(a) for a in shares.mu] != list(tree.n_nodes) or [len(a) for a in shares.kappa] != list(tree.n_nodes):
            raise ValueError('shares: not of this tree (nodes per level differ)')
        for a in (mu, kappa):
            if not (np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0):
                raise ValueError('mu and kappa values must be finite and in [0, 1]')
        self._ctx.check(_lib.load().tsf_rollup_solve_tree(h, mu.ctypes.data, kappa.ctypes.data))

    def reconcile_tree(self, spec, theta, y_scale, grid, group, series_key, share, quantiles=(), cumulative=False,
                       samples=False, floor=None, cap=None, extra_future=None):
        """The second pass over members that were added, after solve_tree: draw' = draw + share[n] * (c - acc) of the
        member's group -> Reconciled, with reconcile's arguments and outputs.  share [N]: TreeShares.share."""
        self._handle()
        self._tree()
        return self._second_pass('tsf_rollup_reconcile_tree', spec, theta, y_scale, grid, group, series_key, share,
                                 quantiles, cumulative, samples, floor, cap, extra_future)

    def tree_totals(self, level, levels, cumulative=False, samples=False, nodes=None):
        """-> RollupQuantiles of the reconciled nodes of one level in [1, L] (count: the members added below each node);
        with samples, (RollupQuantiles, [n][H][S]).  nodes: (first, count), a range of the level's nodes (None: all)."""
        h = self._handle()
        tree = self._tree()
        if not 1 <= int(level) <= tree.n_levels:
            raise ValueError('level must be in [1, %d]' % tree.n_levels)
        n_level = tree.n_nodes[int(level) - 1]
        n0, n = (0, n_level) if nodes is None else (int(nodes[0]), int(nodes[1]))
        if n0 < 0 or n < 1 or n0 + n > n_level:
            raise ValueError('nodes: (first, count) within the level\'s %d nodes, count >= 1' % n_level)
        quantile_columns(levels)
        levels = np.array(levels, dtype=np.float64).reshape(-1)
        Q = len(levels)
        if Q == 0:
            raise ValueError('at least one quantile level')
        res, out = self._group_outs(Q, ['q'] + (['cum_q'] if cumulative else []) + (['samples'] if samples else []), n)
        self._ctx.check(_lib.load().tsf_rollup_tree_totals(h, int(level), n0, n, Q, levels.ctypes.data, ctypes.byref(out)))
        r = RollupQuantiles(res['yhat'], res['count'], levels, res['q'], res.get('cum_q'))
        return (r, res['samples']) if samples else r


class Reconciled(Quantiles):
    """What Rollup.reconcile returns: a Quantiles (yhat [N][H]; quantiles [Q]; q, cum_q [N][Q][H] or None; frame(n, ds)
    with predict_quantiles' column names) of the reconciled draws, and samples [N][H][S] or None."""

    def __init__(self, yhat, quantiles, q, cum_q=None, samples=None):
        Quantiles.__init__(self, yhat, quantiles, q, cum_q)
        self.samples = samples


def reconcile_shares(group, n_groups, weight=None, total_weight='struct'):
    """Weights -> (share [N], share_total [G]) for Rollup.reconcile / reconciled_totals: a thin binding of
    tsf_reconcile_shares (host only).  group [N]: dense indices in [0, n_groups).  weight [N]: the members' forecast error
    variances (None: all 1).  total_weight: the totals' -- 'ols' (all 1), 'struct' (the group's member count: a total
    is as uncertain as its members together; a group without members gets none) or an array [G] (NaN: the group has no
    total).  share = w / (v + W), share_total = W / (v + W), W the group's sum of w."""
    G = int(n_groups)
    group = np.ascontiguousarray(group, dtype=np.int64)
    if group.ndim != 1:
        raise ValueError('group must be [N]')
    N = group.shape[0]
    if G < 1:
        raise ValueError('n_groups must be >= 1')
    if N and (group.min() < 0 or group.max() >= G):
        raise ValueError('group values must be in [0, %d)' % G)
    w = None
    if weight is not None:
        w = np.ascontiguousarray(weight, dtype=np.float64)
        if w.shape != (N,):
            raise ValueError('weight must be [N]')
        if not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError('weight values must be finite and positive')
    if isinstance(total_weight, str):
        if total_weight == 'ols':
            v = np.ones(G)
        elif total_weight == 'struct':
            v = np.bincount(group, minlength=G).astype(np.float64)
            v[v == 0] = np.nan
        else:
            raise ValueError("total_weight must be 'ols', 'struct' or an array [n_groups]")
    else:
        v = np.ascontiguousarray(total_weight, dtype=np.float64)
        if v.shape != (G,):
            raise ValueError('total_weight must be [n_groups]')
        if not ((np.isfinite(v) & (v > 0)) | np.isnan(v)).all():
            raise ValueError('total_weight values must be finite and positive (NaN: no total)')
    share, share_total = np.zeros(N), np.zeros(G)
    rc = _lib.load().tsf_reconcile_shares(N, group.ctypes.data if N else None, _lib._ptr(w) if N else None, G,
                                          v.ctypes.data, share.ctypes.data if N else None, share_total.ctypes.data)
    if rc != 0:
        raise _lib.TsfError('tsf_reconcile_shares refused its arguments (%d)' % rc)
    return share, share_total


def aggregate_aligned(y, group, n_groups):
    """The histories of the totals to fit: y [N][T] on one calendar, group [N] -> [G][T] float64.  A pure numpy loop of
    tot[g] = tot[g] + y[n] in ascending n from zeros (so the order of the adds is fixed); NaN propagates.  Ragged panels
    are out of scope."""
    y = np.asarray(y, dtype=np.float64)
    group = np.asarray(group, dtype=np.int64)
    G = int(n_groups)
    if y.ndim != 2:
        raise ValueError('y must be [N][T]')
    if group.shape != (y.shape[0],):
        raise ValueError('group must be [N]')
    if G < 1 or (len(group) and (group.min() < 0 or group.max() >= G)):
        raise ValueError('group values must be in [0, n_groups), n_groups >= 1')
    tot = np.zeros((G, y.shape[1]))
    for n in range(y.shape[0]):
        g = int(group[n])
        tot[g] = tot[g] + y[n]
    return tot


class RollupTree(object):
    """The levels of a hierarchy above its members, host only (include/tsf.h "tree reconciliation"): group [N] (each
    member's node of level 1, dense in [0, n_nodes[0])), n_nodes [L] (nodes per level 1 .. L), parent (L - 1 int64
    arrays: parent[k][c] is the node of level k + 2 above node c of level k + 1), labels (the unique labels per level,
    or None).  A node needs no child and a group no member: such a node is empty and stays 0.  Every error is a
    ValueError."""

    def __init__(self, group, n_nodes, parent, labels=None):
        self.group = np.ascontiguousarray(group, dtype=np.int64)
        self.n_nodes = [int(n) for n in n_nodes]
        self.parent = [np.ascontiguousarray(p, dtype=np.int64) for p in parent]
        self.labels = labels
        if self.group.ndim != 1:
            raise ValueError('group must be [N]')
        if not 1 <= len(self.n_nodes) <= 1 + _lib.TREE_MAX_LEVELS:
            raise ValueError('a tree has 1 to %d levels of nodes' % (1 + _lib.TREE_MAX_LEVELS))
        if min(self.n_nodes) < 1:
            raise ValueError('every level needs at least one node')
        if len(self.parent) != len(self.n_nodes) - 1:
            raise ValueError('parent: one array per level below the top')
        if len(self.group) and (self.group.min() < 0 or self.group.max() >= self.n_nodes[0]):
            raise ValueError('group values must be in [0, %d)' % self.n_nodes[0])
        for k, p in enumerate(self.parent):
            if p.shape != (self.n_nodes[k],):
                raise ValueError('parent[%d] must be [%d]: one parent per node of level %d' % (k, self.n_nodes[k], k + 1))
            if p.min() < 0 or p.max() >= self.n_nodes[k + 1]:
                raise ValueError('parent[%d] values must be in [0, %d)' % (k, self.n_nodes[k + 1]))

    @property
    def n_levels(self):
        return len(self.n_nodes)

    def member_counts(self):
        """-> per level, the number of members below each node (int64 [n_nodes[k]])"""
        cnt = [np.bincount(self.group, minlength=self.n_nodes[0]).astype(np.int64)]
        for k, p in enumerate(self.parent):
            cnt.append(np.bincount(p, weights=cnt[-1], minlength=self.n_nodes[k + 1]).astype(np.int64))
        return cnt


def rollup_tree(level_labels):
    """One label array [N] per level (each member's group label, that group's parent label, and so on upwards; each an
    integer array or a tuple of them, as in rollup_groups) -> RollupTree with dense indices per level and the unique
    labels.  A label with two different parents is a ValueError.  Pure numpy."""
    if not isinstance(level_labels, (list, tuple)) or len(level_labels) < 1:
        raise ValueError('level_labels: a list of label arrays, one per level')
    uniq, idx = [], []
    for lab in level_labels:
        u, i = rollup_groups(lab)
        if idx and len(i) != len(idx[0]):
            raise ValueError('level_labels: the label arrays differ in length')
        uniq.append(u)
        idx.append(i)
    if len(idx[0]) == 0:
        raise ValueError('level_labels: no members')
    parent = []
    for k in range(1, len(idx)):
        p = np.full(len(uniq[k - 1]), -1, dtype=np.int64)
        p[idx[k - 1]] = idx[k]
        if not np.array_equal(p[idx[k - 1]], idx[k]):
            raise ValueError('level %d: a label has two different parents' % k)
        parent.append(p)
    return RollupTree(idx[0], [len(u) for u in uniq], parent, labels=uniq)


class TreeShares(object):
    """What reconcile_tree_shares returns: share [N] (Rollup.reconcile_tree) and, as one array per level 1 .. L, mu, e
    and kappa (Rollup.solve_tree takes the object)."""

    def __init__(self, share, mu, e, kappa):
        self.share, self.mu, self.e, self.kappa = share, mu, e, kappa


def reconcile_tree_shares(tree, weight=None, node_weight='struct'):
    """Weights -> TreeShares: a thin binding of tsf_reconcile_tree_shares (host only).  weight [N]: the members' forecast
    error variances (None: all 1).  node_weight: the variances of the nodes' fitted totals -- 'ols' (all 1), 'struct'
    (the number of members below the node; a node without members gets none) or one array per level 1 .. L (NaN: the
    node has no total)."""
    if not isinstance(tree, RollupTree):
        raise ValueError('tree must be a RollupTree (rollup_tree)')
    N = len(tree.group)
    w = None
    if weight is not None:
        w = np.ascontiguousarray(weight, dtype=np.float64)
        if w.shape != (N,):
            raise ValueError('weight must be [N]')
        if not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError('weight values must be finite and positive')
    if isinstance(node_weight, str):
        if node_weight == 'ols':
            v = [np.ones(n) for n in tree.n_nodes]
        elif node_weight == 'struct':
            v = [np.where(c > 0, c, np.nan).astype(np.float64) for c in tree.member_counts()]
        else:
            raise ValueError("node_weight must be 'ols', 'struct' or one array per level")
    else:
        v = [np.ascontiguousarray(a, dtype=np.float64) for a in node_weight]
        if [a.shape for a in v] != [(n,) for n in tree.n_nodes]:
            raise ValueError('node_weight: one array [n_nodes] per level')
    v = np.concatenate(v)
    if not ((np.isfinite(v) & (v > 0)) | np.isnan(v)).all():
        raise ValueError('node_weight values must be finite and positive (NaN: no total)')
    M = len(v)
    n_nodes = np.ascontiguousarray(tree.n_nodes[1:], dtype=np.int64)
    parent = np.ascontiguousarray(np.concatenate(tree.parent + [np.zeros(0, dtype=np.int64)]), dtype=np.int64)
    share, mu, e, kappa = np.zeros(N), np.zeros(M), np.zeros(M), np.zeros(M)
    rc = _lib.load().tsf_reconcile_tree_shares(N, tree.group.ctypes.data if N else None, _lib._ptr(w) if N else None,
                                               tree.n_nodes[0], len(n_nodes), n_nodes.ctypes.data, parent.ctypes.data,
                                               v.ctypes.data, share.ctypes.data if N else None, mu.ctypes.data,
                                               e.ctypes.data, kappa.ctypes.data)
    if rc != 0:
        raise _lib.TsfError('tsf_reconcile_tree_shares refused its arguments (%d)' % rc)
    cuts = np.cumsum(tree.n_nodes)[:-1]
    return TreeShares(share, np.split(mu, cuts), np.split(e, cuts), np.split(kappa, cuts))


def predict_reconciled(spec, theta, y_scale, grid, ds_future_ns, labels, quantiles, series_key, total_theta,
                       total_y_scale, total_grid, total_key, total_spec=None, weight=None, total_weight='struct',
                       floor=None, cap=None, extra_future=None, total_floor=None, total_cap=None,
                       total_extra_future=None, uncertainty_samples=1000, seed=0, cumulative=False, ctx=None):
    """The one-spec convenience, in the manner of predict_rollup: rollup_groups(labels), one Rollup.add of the members,
    set_totals of the G directly fitted totals (total g belongs to the g-th unique label; total_spec: the members' spec
    where None), reconcile_shares, reconcile, reconciled_totals, close -> (unique_labels, Reconciled of the members,
    RollupQuantiles of the totals)."""
    quantile_columns(quantiles)
    if len(np.asarray(quantiles).reshape(-1)) == 0:
        raise ValueError('at least one quantile level')
    uniq, group = rollup_groups(labels)
    if len(group) == 0:
        raise ValueError('nothing to reconcile: no series')
    ds = np.asarray(ds_future_ns)
    if ds.ndim != 1 or ds.shape[0] < 1:
        raise ValueError('ds_future must be [H], H >= 1: a roll-up has one calendar')
    G, H = len(uniq), ds.shape[0]
    tspec = total_spec or spec
    tgroup = np.arange(G, dtype=np.int64)
    _rollup_add_args(spec, theta, y_scale, grid, group, series_key, floor, cap, extra_future, G, H)
    if np.asarray(total_theta).ndim != 2 or np.asarray(total_theta).shape[0] != G:
        raise ValueError('total_theta must be [G][stride]: one total per unique label')
    _rollup_add_args(tspec, total_theta, total_y_scale, total_grid, tgroup, total_key, total_floor, total_cap,
                     total_extra_future, G, H)
    if set(np.asarray(total_key, dtype=np.int64).tolist()) & set(np.asarray(series_key, dtype=np.int64).tolist()):
        raise ValueError('total_key: a total shares a key (a stream) with a member')
    share, share_total = reconcile_shares(group, G, weight=weight, total_weight=total_weight)
    with Rollup(ds_future_ns, G, uncertainty_samples=uncertainty_samples, seed=seed, ctx=ctx) as r:
        r.add(spec, theta, y_scale, grid, group, series_key, floor=floor, cap=cap, extra_future=extra_future)
        r.set_totals(tspec, total_theta, total_y_scale, total_grid, tgroup, total_key, floor=total_floor, cap=total_cap,
                     extra_future=total_extra_future)
        members = r.reconcile(spec, theta, y_scale, grid, group, series_key, share, quantiles=quantiles,
                              cumulative=cumulative, floor=floor, cap=cap, extra_future=extra_future)
        return uniq, members, r.reconciled_totals(share_total, quantiles, cumulative=cumulative)


def predict_rollup(spec, theta, y_scale, grid, ds_future_ns, labels, quantiles, series_key, floor=None, cap=None,
                   extra_future=None, uncertainty_samples=1000, seed=0, cumulative=False, ctx=None, noise_corr=None,
                   group_key=None, noise_ar=None):
    """The one-spec convenience: rollup_groups(labels), one Rollup.add, quantiles, close ->
    (unique_labels, RollupQuantiles).  noise_corr, group_key: as in Rollup, per unique label in sorted order; noise_ar:
    as in Rollup.add (not together with noise_corr)."""
    if noise_ar is not None and noise_corr is not None:
        raise ValueError('noise_ar together with noise_corr: the correlated add regenerates the independent noise')
    quantile_columns(quantiles)
    if len(np.asarray(quantiles).reshape(-1)) == 0:
        raise ValueError('at least one quantile level')
    uniq, group = rollup_groups(labels)
    if len(group) == 0:
        raise ValueError('nothing to roll up: no series')
    ds = np.asarray(ds_future_ns)
    if ds.ndim != 1 or ds.shape[0] < 1:
        raise ValueError('ds_future must be [H], H >= 1: a roll-up has one calendar')
    _rollup_add_args(spec, theta, y_scale, grid, group, series_key, floor, cap, extra_future, len(uniq), ds.shape[0])
    with Rollup(ds_future_ns, len(uniq), uncertainty_samples=uncertainty_samples, seed=seed, ctx=ctx, noise_corr=noise_corr,
                group_key=group_key) as r:
        r.add(spec, theta, y_scale, grid, group, series_key, floor=floor, cap=cap, extra_future=extra_future,
              noise_ar=noise_ar)
        return uniq, r.quantiles(quantiles, cumulative=cumulative)


# ---- temporal reconciliation: daily forecasts and directly fitted period totals --------------------------------
# Reconciliation along time inside each series (include/tsf.h "temporal reconciliation"): the rows of a daily forecast are
# the members, the forecast of a model fitted on the weekly or monthly totals of the same history is the total, each
# window of rows is a group.  period_history makes the histories to fit the period model on, temporal_shares the shares,
# predict_temporal the coherent forecast of both.

def _most_frequent_rows(windows):
    """the row count most windows have (the larger one on a tie): what a complete period of the calendar holds"""
    rows, counts = np.unique(windows.n_rows, return_counts=True)
    return int(rows[np.flatnonzero(counts == counts.max())[-1]])


def period_history(ds_ns, y, freq, full_rows=None):
    """The history's totals over the calendar periods `freq` (period_windows) -> (ds_period [Tk], y_period [N][Tk],
    windows): the panel to fit the period model on.  ds_ns [T] one shared calendar, y [N][T].  A period is kept only where
    it has full_rows rows (None: the row count most periods have), so an incomplete first or last period and a period
    with a missing day are left out rather than fitted as a low total; ds_period is each kept window's first timestamp,
    windows the kept Windows over the T rows.  The totals are window_totals' (NaN where a row is NaN).  Host numpy."""
    w = period_windows(ds_ns, freq)
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 2 or y.shape[1] != int(w.end.max()):
        raise ValueError('period_history: y must be [N][T] on the calendar ds [T]')
    full = _most_frequent_rows(w) if full_rows is None else int(full_rows)
    keep = np.flatnonzero(w.n_rows == full)
    if len(keep) == 0:
        raise ValueError('period_history: no period has %d rows' % full)
    kept = Windows(w.start[keep], w.end[keep], w.label_ns[keep])
    return kept.label_ns.copy(), window_totals(y, kept), kept


class TemporalShares(object):
    """What temporal_shares returns: windows (K of them), share [N][H], share_total [N][K] (NaN: the window is not
    reconciled for that series)."""

    def __init__(self, windows, share, share_total):
        self.windows, self.share, self.share_total = windows, share, share_total


def _disjoint(windows, H):
    """ValueError where two windows share a row"""
    windows.check(H)
    cover = np.zeros(H + 1, dtype=np.int64)
    np.add.at(cover, windows.start, 1)
    np.add.at(cover, windows.end, -1)
    if (np.cumsum(cover) > 1).any():
        raise ValueError('windows: two windows share a row (temporal reconciliation needs disjoint windows)')


def temporal_shares(windows, N, H, weight=None, period_weight='struct', active=None):
    """Weights -> TemporalShares for predict_temporal: a thin binding of tsf_temporal_shares (host only).  weight: the
    forecast error variances of the rows, [H] or [N][H] (None: all 1).  period_weight: the period forecasts' -- 'struct'
    (the window's row count: a period total is as uncertain as its rows together), 'ols' (all 1) or an array [K] or
    [N][K].  active [K] or [N][K] bool: the windows to reconcile (None: those with the row count most windows have, so
    that a partial first or last week of the horizon is left as it is).  share = w / (v + W), share_total = W / (v + W),
    W the window's sum of w; a window that is not active gets share 0 and share_total NaN."""
    if not isinstance(windows, Windows):
        raise ValueError('windows must be a Windows (row_windows, period_windows)')
    N, H, K = int(N), int(H), len(windows)
    if N < 0 or H < 1:
        raise ValueError('N must be >= 0 and H >= 1')
    _disjoint(windows, H)
    w = None
    if weight is not None:
        w = np.asarray(weight, dtype=np.float64)
        if w.shape not in ((H,), (N, H)):
            raise ValueError('weight must be [H] or [N][H]')
        if not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError('weight values must be finite and positive')
        w = np.ascontiguousarray(np.broadcast_to(w, (N, H)))
    if isinstance(period_weight, str):
        if period_weight == 'struct':
            v = windows.n_rows.astype(np.float64)
        elif period_weight == 'ols':
            v = np.ones(K)
        else:
            raise ValueError("period_weight must be 'struct', 'ols' or an array [K] or [N][K]")
    else:
        v = np.asarray(period_weight, dtype=np.float64)
        if v.shape not in ((K,), (N, K)):
            raise ValueError('period_weight must be [K] or [N][K]')
        if not ((np.isfinite(v) & (v > 0)) | np.isnan(v)).all():
            raise ValueError('period_weight values must be finite and positive (NaN: the window is not reconciled)')
    v = np.array(np.broadcast_to(v, (N, K)), dtype=np.float64, order='C')
    if active is None:
        act = windows.n_rows == _most_frequent_rows(windows)
    else:
        act = np.asarray(active)
        if act.dtype != np.bool_ or act.shape not in ((K,), (N, K)):
            raise ValueError('active must be bool [K] or [N][K]')
    v[~np.broadcast_to(act, (N, K))] = np.nan
    share, share_total = np.zeros((N, H)), np.zeros((N, K))
    rc = _lib.load().tsf_temporal_shares(N, H, K, windows.start.ctypes.data, windows.end.ctypes.data, _lib._ptr(w),
                                         v.ctypes.data if N else None, share.ctypes.data if N else None,
                                         share_total.ctypes.data if N else None)
    if rc != 0:
        raise _lib.TsfError('tsf_temporal_shares refused its arguments (%d)' % rc)
    return TemporalShares(windows, share, share_total)


TEMPORAL_FIELDS = ('q', 'cum_q', 'total', 'win_q', 'samples', 'win_samples')


class TemporalQuantiles(Quantiles):
    """What predict_temporal returns: a Quantiles of the reconciled rows (yhat [N][H]; quantiles [Q]; q, cum_q [N][Q][H]
    or None) with ds (the daily calendar), windows (K of them), total [N][K] (the reconciled point forecast of every
    window's total), win_q [N][Q][K] (the quantiles of the reconciled window totals), and samples [N][H][S], win_samples
    [N][K][S] or None."""

    def __init__(self, windows, ds, yhat, quantiles, q, cum_q=None, total=None, win_q=None, samples=None, win_samples=None):
        Quantiles.__init__(self, yhat, quantiles, q, cum_q)
        self.windows, self.ds, self.total, self.win_q = windows, ds, total, win_q
        self.samples, self.win_samples = samples, win_samples

    def frame(self, n):
        """The rows of series n in Quantiles.frame's layout: ds, yhat, yhat_q<..>, yhat_cum_q<..>."""
        return Quantiles.frame(self, n, self.ds if self.ds.ndim == 1 else self.ds[n])

    def window_frame(self, n):
        """The periods of series n in WindowQuantiles.frame's layout, one row per window."""
        return WindowQuantiles(self.windows, self.ds, self.yhat, self.quantiles, total=self.total, q=self.win_q).frame(n)


def _temporal_phi(noise_ar, N, ds_ns, name):
    """_noise_ar_phi with the temporal entry's range: phi in [0, 1)"""
    if isinstance(noise_ar, NoiseARStart):
        raise ValueError('%s: predict_temporal keeps the stationary start (a conditioned noise_ar is not taken)' % name)
    phi = _noise_ar_phi(noise_ar, N, ds_ns)
    if phi is not None and (phi < 0).any():
        raise ValueError('%s values must be in [0, 1)' % name)
    return phi


def _predict_temporal_call(spec, theta, y_scale, grid, ds_ns, windows, period_spec, period_theta, period_y_scale,
                           period_grid, ds_period_ns, shares, levels, series_key, period_key, want, floor=None, cap=None,
                           extra_future=None, period_floor=None, period_cap=None, period_extra_future=None, noise_ar=None,
                           period_noise_ar=None, uncertainty_samples=1000, seed=0, ctx=None):
    """One tsf_predict_temporal call -> dict of yhat and the outputs named in `want` (TEMPORAL_FIELDS).  Every
    argument-shape error is raised before the library is loaded."""
    for name, v in (('noise_ar', noise_ar), ('period_noise_ar', period_noise_ar)):
        if isinstance(v, NoiseARStart):
            raise ValueError('%s: predict_temporal keeps the stationary start (a conditioned noise_ar is not taken)' % name)
    theta, N, y_scale, grid, ds_ns, shared, H, floor, cap, ex, key = _checked_forecast_inputs(
        spec, theta, y_scale, grid, ds_ns, floor, cap, extra_future, series_key)
    if not isinstance(windows, Windows):
        raise ValueError('windows must be a Windows (row_windows, period_windows)')
    _disjoint(windows, H)
    K = len(windows)
    ptheta, Np, py_scale, pgrid, ds_p, pshared, Hp, pfloor, pcap, pex, pkey = _checked_forecast_inputs(
        period_spec, period_theta, period_y_scale, period_grid, ds_period_ns, period_floor, period_cap,
        period_extra_future, period_key)
    if Np != N:
        raise ValueError('period_theta must be [N][stride]: one period model per series')
    if Hp != K:
        raise ValueError('ds_period must be [K] or [N][K]: one row per window (K = %d, got %d)' % (K, Hp))
    if key is None or pkey is None:
        raise ValueError('series_key and period_key are required')
    if not isinstance(shares, TemporalShares):
        raise ValueError('shares must be a TemporalShares (temporal_shares)')
    share = np.ascontiguousarray(shares.share, dtype=np.float64)
    share_total = np.ascontiguousarray(shares.share_total, dtype=np.float64)
    if share.shape != (N, H) or share_total.shape != (N, K):
        raise ValueError('shares must hold share [N][H] = %r and share_total [N][K] = %r' % ((N, H), (N, K)))
    levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    quantile_columns(levels)            # (ValueError for a bad level, two levels of one name, too many)
    Q, S = len(levels), int(uncertainty_samples)
    unknown = set(want) - set(TEMPORAL_FIELDS)
    if unknown:
        raise ValueError('unknown outputs %s' % sorted(unknown))
    if not set(want) - {'total'}:
        raise ValueError('no output wanted but yhat and total')
    if not Q and set(want) & {'q', 'cum_q', 'win_q'}:
        raise ValueError('q, cum_q and win_q need quantile levels')
    if not 2 <= S <= 4096:
        raise ValueError('uncertainty_samples must be in [2, 4096]')
    phi = _temporal_phi(noise_ar, N, ds_ns, 'noise_ar')
    pphi = _temporal_phi(period_noise_ar, N, ds_p, 'period_noise_ar')
    shapes = {'q': (N, Q, H), 'cum_q': (N, Q, H), 'total': (N, K), 'win_q': (N, Q, K), 'samples': (N, H, S),
              'win_samples': (N, K, S)}
    res = {'yhat': np.zeros((N, H))}
    res.update((k, np.zeros(shapes[k])) for k in want)
    ctx = ctx or get_context()
    L = _lib.load()
    cs, cps = spec.to_c(), period_spec.to_c()
    out = _lib.TsfTemporalOut(**{k: v.ctypes.data for k, v in res.items()})
    rc = L.tsf_predict_temporal(
        ctx.handle,
        ctypes.byref(cs), N, H, theta.ctypes.data, y_scale.ctypes.data, grid.ctypes.data, len(grid), ds_ns.ctypes.data,
        int(shared), _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex), key.ctypes.data, _lib._ptr(phi),
        ctypes.byref(cps), K, ptheta.ctypes.data, py_scale.ctypes.data, pgrid.ctypes.data, len(pgrid), ds_p.ctypes.data,
        int(pshared), _lib._ptr(pfloor), _lib._ptr(pcap), _lib._ptr(pex), pkey.ctypes.data, _lib._ptr(pphi),
        S, int(seed), windows.start.ctypes.data, windows.end.ctypes.data, share.ctypes.data, share_total.ctypes.data, Q,
        levels.ctypes.data if Q else None, ctypes.byref(out))
    ctx.check(rc)
    return res


def predict_temporal(spec, theta, y_scale, grid, ds_future_ns, windows, period_spec, period_theta, period_y_scale,
                     period_grid, ds_period_ns, shares, quantiles, series_key, period_key, cumulative=False, samples=False,
                     floor=None, cap=None, extra_future=None, period_floor=None, period_cap=None,
                     period_extra_future=None, noise_ar=None, period_noise_ar=None, uncertainty_samples=1000, seed=0,
                     ctx=None):
    """The daily forecast of every series and the forecast of its period model made coherent -> TemporalQuantiles
    (include/tsf.h tsf_predict_temporal).  The first five arguments are the daily model as in predict_quantiles; windows
    (period_windows(ds_future_ns, 'W'), ...) are disjoint row windows of its H rows; period_spec ... ds_period_ns are the
    model fitted on the period totals (period_history) and its K future rows, one per window (windows.label_ns);
    shares: temporal_shares(windows, N, H, ...).  Sample by sample the incoherence d = period draw - the window's sum of
    daily draws is shared out: row + share * d, total + share_total * d, so the reconciled rows of a window sum to the
    reconciled total, and q, cum_q (with cumulative) and win_q are quantiles of coherent draws.  series_key and
    period_key [N] are both required and should not share a value (the two models' streams would be shared).  With
    samples, the reconciled draws [N][H][S] and window totals [N][K][S] are returned as well."""
    levels = np.array(quantiles, dtype=np.float64).reshape(-1)
    if len(levels) == 0:
        raise ValueError('at least one quantile level')
    want = ['q', 'total', 'win_q'] + (['cum_q'] if cumulative else []) + (['samples', 'win_samples'] if samples else [])
    r = _predict_temporal_call(spec, theta, y_scale, grid, ds_future_ns, windows, period_spec, period_theta, period_y_scale,
                               period_grid, ds_period_ns, shares, levels, series_key, period_key, want, floor=floor,
                               cap=cap, extra_future=extra_future, period_floor=period_floor, period_cap=period_cap,
                               period_extra_future=period_extra_future, noise_ar=noise_ar,
                               period_noise_ar=period_noise_ar, uncertainty_samples=uncertainty_samples, seed=seed, ctx=ctx)
    return TemporalQuantiles(windows, np.ascontiguousarray(ds_future_ns, dtype=np.int64), r['yhat'], levels, r['q'],
                             r.get('cum_q'), r['total'], r['win_q'], r.get('samples'), r.get('win_samples'))


# ---- diagnostics used by the parity tests -----------------------------------------------------

def eval_aligned(spec, ds_ns, y, theta, floor=None, cap=None, extra=None, ctx=None):
    """-log posterior and gradient at theta [N][stride] for an aligned panel."""
    ctx = ctx or get_context()
    L = _lib.load()
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    y = np.ascontiguousarray(y)
    N, T = y.shape
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    cs = spec.to_c()
    floor = _opt_f64(floor, N, 'floor')
    cap = _opt_f64(cap, N, 'cap')
    ex = np.ascontiguousarray(extra, dtype=np.float64) if spec.extra else None
    f = np.zeros(N)
    g = np.zeros_like(theta)
    rc = L.tsf_eval(ctx.handle, ctypes.byref(cs), N, T, ds_ns.ctypes.data, y.ctypes.data,
                    _lib.y_dtype_code(y), _lib._ptr(floor), _lib._ptr(cap), _lib._ptr(ex),
                    theta.ctypes.data, f.ctypes.data, g.ctypes.data)
    ctx.check(rc)
    return f, g


def eval_quadratic(spec, ds_ns, y, theta_ref, theta, extra=None, ctx=None):
    """-log posterior and gradient at theta [N][stride] in the QUADRATIC evaluation form built around the
    reference point theta_ref [N][stride] (include/tsf.h tsf_eval_quadratic): what fit_quad_kernel
    evaluates at the trial points of its line searches."""
    ctx = ctx or get_context()
    L = _lib.load()
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    y = np.ascontiguousarray(y)
    N, T = y.shape
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    theta_ref = np.ascontiguousarray(theta_ref, dtype=np.float64)
    if theta.shape != (N, spec.theta_stride) or theta_ref.shape != theta.shape:
        raise ValueError('theta and theta_ref must be [N][theta_stride]')
    cs = spec.to_c()
    ex = np.ascontiguousarray(extra, dtype=np.float64) if spec.extra else None
    f = np.zeros(N)
    g = np.zeros_like(theta)
    rc = L.tsf_eval_quadratic(ctx.handle, ctypes.byref(cs), N, T, ds_ns.ctypes.data, y.ctypes.data,
                              _lib.y_dtype_code(y), _lib._ptr(ex), theta_ref.ctypes.data, theta.ctypes.data,
                              f.ctypes.data, g.ctypes.data)
    ctx.check(rc)
    return f, g


def design(spec, ds_ns, extra=None, ctx=None):
    """Design matrix X [T][K], scaled time t [T] and the grid info, as the device builds them."""
    ctx = ctx or get_context()
    L = _lib.load()
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    T = len(ds_ns)
    cs = spec.to_c()
    ex = np.ascontiguousarray(extra, dtype=np.float64) if spec.extra else None
    X = np.zeros((T, spec.K))
    t = np.zeros(T)
    grid = np.zeros(1, dtype=_lib.GRID_DTYPE)
    rc = L.tsf_design(ctx.handle, ctypes.byref(cs), T, ds_ns.ctypes.data, _lib._ptr(ex),
                      X.ctypes.data, t.ctypes.data, grid.ctypes.data)
    ctx.check(rc)
    return X, t, grid


def selftest_math(op, a, b=None, ctx=None):
    ctx = ctx or get_context()
    L = _lib.load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.zeros_like(a)
    rc = L.tsf_selftest_math(ctx.handle, int(op), a.size, a.ctypes.data, _lib._ptr(b),
                             out.ctypes.data)
    ctx.check(rc)
    return out


# ---- cross-validation ---------------------------------------------------------------------------

class CVResult(object):
    """What cross_validate returns (include/tsf.h tsf_cross_validate).

    Per series [N]: status (TSF_CV_*), n_folds, n_holdout, n_metric.
    Per fold [F] (series by series, cutoffs ascending): fold_series, cutoff, hist_rows, hold_rows, and `fit`, the
    FitResult of every fold (grid [F]).
    Per holdout row [R] (fold by fold): row_fold, row_index (the row's index in the caller's ds: into [T] for an
    aligned panel, into the ragged panel's rows otherwise), ds, y, yhat, yhat_lower / yhat_upper (None without
    intervals).
    Per metric row [M] (series by series, horizons ascending): metric_series, horizon, mse, rmse, mae, mape,
    coverage (None without intervals)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def fold_offsets(self):
        return np.concatenate([[0], np.cumsum(self.n_folds)]).astype(np.int64)

    @property
    def row_offsets(self):
        return np.concatenate([[0], np.cumsum(self.n_holdout)]).astype(np.int64)

    @property
    def metric_offsets(self):
        return np.concatenate([[0], np.cumsum(self.n_metric)]).astype(np.int64)


def _cv_args(horizon, period, initial, rolling_window):
    a = _lib.TsfCvArgs()
    a.horizon_ns = int(horizon)
    a.period_ns = -1 if period is None else int(period)
    a.initial_ns = -1 if initial is None else int(initial)
    a.rolling_window = float(rolling_window)
    return a


def _cv_panel(ds_ns, y, offsets):
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    y = np.ascontiguousarray(y)
    if offsets is None:
        if y.ndim != 2 or y.shape[1] != ds_ns.shape[0]:
            raise ValueError('aligned panel: y must be [N][T] with T == len(ds)')
        return ds_ns, y, None, y.shape[0], ds_ns.shape[0]
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if y.ndim != 1 or y.shape[0] != ds_ns.shape[0] or offsets[-1] != y.shape[0]:
        raise ValueError('ragged panel: ds / y must be 1-D with offsets[-1] rows')
    return ds_ns, y, offsets, len(offsets) - 1, 0


def cv_plan(ds_ns, horizon, period=None, initial=None, rolling_window=0.1, offsets=None, N=1):
    """tsf_cv_plan (host only, no GPU): fbprophet's cutoffs and row masks per series.  Aligned input: ds_ns [T] shared
    by N series; ragged: offsets [N+1] into ds_ns.  Times in ns; period None = horizon / 2, initial None = 3 * horizon.
    Returns dict: n_folds, status, n_holdout, n_metric [N]; cutoff, hist_rows, hold_rows [F]."""
    L = _lib.load()
    ds_ns = np.ascontiguousarray(ds_ns, dtype=np.int64)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        N, T = len(offsets) - 1, 0
    else:
        T = len(ds_ns)
    a = _cv_args(horizon, period, initial, rolling_window)
    nf, st = np.zeros(N, np.int32), np.zeros(N, np.int32)
    nh, nm = np.zeros(N, np.int64), np.zeros(N, np.int64)
    args = (N, T, _lib._ptr(offsets), ds_ns.ctypes.data, ctypes.byref(a), nf.ctypes.data, st.ctypes.data,
            nh.ctypes.data, nm.ctypes.data)
    if L.tsf_cv_plan(*args, None, None, None) != 0:
        raise ValueError('tsf_cv_plan: bad arguments (horizon > 0, rolling_window in [0, 1], sorted panel)')
    F = int(nf.sum())
    cut, hist, hold = np.zeros(F, np.int64), np.zeros(F, np.int32), np.zeros(F, np.int32)
    if L.tsf_cv_plan(*args, cut.ctypes.data, hist.ctypes.data, hold.ctypes.data) != 0:
        raise ValueError('tsf_cv_plan failed')
    return {'n_folds': nf, 'status': st, 'n_holdout': nh, 'n_metric': nm, 'cutoff': cut, 'hist_rows': hist,
            'hold_rows': hold}


def cross_validate(spec, ds_ns, y, horizon, period=None, initial=None, offsets=None, floor=None, cap=None, extra=None,
                   rolling_window=0.1, intervals=False, uncertainty_samples=1000, interval_width=0.8, seed=0,
                   series_key=None, ctx=None, devices=None):
    """fbprophet's diagnostics.cross_validation + performance_metrics for a whole panel, on the GPU
    (include/tsf.h tsf_cross_validate).  Input as fit_aligned (ds_ns [T], y [N][T], extra [n_extra][T]) or, with
    offsets [N+1], as fit_ragged.  horizon / period / initial: int64 ns (period None = horizon / 2, initial None =
    3 * horizon).  spec: the full-history model's spec (ModelSpec); algorithm=ALGO_AUTO gives fbprophet's optimiser
    rule per fold, with its Newton retry.  series_key [N] keys the interval streams (default: the series index in
    this call).  devices: several GPUs, all folds of a series on one of them.  Returns a CVResult."""
    ds_ns, y, offsets, N, T = _cv_panel(ds_ns, y, offsets)
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    key = None if series_key is None else np.ascontiguousarray(series_key, dtype=np.int64)
    if key is not None and key.shape != (N,):
        raise ValueError('series_key must be [N]')
    devs = None if ctx is not None else resolve_devices(devices)
    kw = dict(rolling_window=rolling_window, intervals=intervals, uncertainty_samples=uncertainty_samples,
              interval_width=interval_width, seed=seed)
    if devs and N >= 2 * MIN_SERIES_PER_DEVICE:
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        lens = np.full(N, T, np.int64) if offsets is None else np.diff(offsets)
        cuts = _cuts(lens, parts)
        key = np.arange(N, dtype=np.int64) if key is None else key       # (the same streams whatever the split)
        ex = None if extra is None else np.asarray(extra)

        def one(c, a, b):
            if offsets is None:
                return cross_validate(spec, ds_ns, y[a:b], horizon, period, initial, None,
                                      None if fl is None else fl[a:b], None if cp is None else cp[a:b], extra,
                                      series_key=key[a:b], ctx=c, **kw)
            r0, r1 = int(offsets[a]), int(offsets[b])
            return cross_validate(spec, ds_ns[r0:r1], y[r0:r1], horizon, period, initial, offsets[a:b + 1] - r0,
                                  None if fl is None else fl[a:b], None if cp is None else cp[a:b],
                                  None if ex is None else ex[:, r0:r1], series_key=key[a:b], ctx=c, **kw)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:]) if b > a]
        parts_res = _run_blocks(one, blocks)
        row_first = [0 if offsets is None else int(offsets[a]) for _, a, _ in blocks]
        return _merge_cv(spec, parts_res, [a for _, a, _ in blocks], intervals, row_first)
    ctx = ctx or get_context()
    L = _lib.load()
    cs = spec.to_c()
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (len(spec.extra), len(ds_ns)):
            raise ValueError('extra must be [n_extra][len(ds)]')
    plan = cv_plan(ds_ns, horizon, period, initial, rolling_window, offsets=offsets, N=N)
    F, R, M = int(plan['n_folds'].sum()), int(plan['n_holdout'].sum()), int(plan['n_metric'].sum())
    fout, farrs = _alloc_out(F, spec.theta_stride, F)
    yhat = np.zeros(R)
    lo = np.zeros(R) if intervals else None
    hi = np.zeros(R) if intervals else None
    hz = np.zeros(M, np.int64)
    mse, rmse, mae, mape = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
    cov = np.zeros(M) if intervals else None
    sst = np.zeros(N, np.int32)
    out = _lib.TsfCvOut(fout, yhat.ctypes.data, _lib._ptr(lo), _lib._ptr(hi), hz.ctypes.data, mse.ctypes.data,
                        rmse.ctypes.data, mae.ctypes.data, mape.ctypes.data, _lib._ptr(cov), sst.ctypes.data)
    a = _cv_args(horizon, period, initial, rolling_window)
    rc = L.tsf_cross_validate(ctx.handle, ctypes.byref(cs), N, T, _lib._ptr(offsets), ds_ns.ctypes.data, y.ctypes.data,
                              _lib.y_dtype_code(y), _lib._ptr(fl), _lib._ptr(cp), _lib._ptr(ex), ctypes.byref(a),
                              _lib._ptr(key), int(uncertainty_samples) if intervals else 0, float(interval_width),
                              int(seed), ctypes.byref(out))
    ctx.check(rc)
    fold_series = np.repeat(np.arange(N, dtype=np.int64), plan['n_folds'])
    # holdout rows: ds / y of the caller's rows [hist, hist + hold) of each fold's series
    start = (np.zeros(N, np.int64) if offsets is None else offsets[:-1])[fold_series] + plan['hist_rows']
    ridx = np.repeat(start - np.concatenate([[0], np.cumsum(plan['hold_rows'])[:-1]]), plan['hold_rows']) + np.arange(R)
    row_fold = np.repeat(np.arange(F, dtype=np.int64), plan['hold_rows'])
    if offsets is None:
        y_rows = y[fold_series[row_fold], ridx].astype(np.float64)
    else:
        y_rows = y[ridx].astype(np.float64)
    return CVResult(spec=spec, status=sst, n_folds=plan['n_folds'], n_holdout=plan['n_holdout'], n_metric=plan['n_metric'],
                    fold_series=fold_series, cutoff=plan['cutoff'], hist_rows=plan['hist_rows'], hold_rows=plan['hold_rows'],
                    fit=FitResult(spec, *farrs), row_fold=row_fold, row_index=ridx, ds=ds_ns[ridx], y=y_rows, yhat=yhat,
                    yhat_lower=lo, yhat_upper=hi,
                    metric_series=np.repeat(np.arange(N, dtype=np.int64), plan['n_metric']), horizon=hz, mse=mse,
                    rmse=rmse, mae=mae, mape=mape, coverage=cov)


def _merge_cv(spec, parts, firsts, intervals, row_first):
    cat = lambda k, p=parts: np.concatenate([getattr(x, k) for x in p])     # noqa: E731
    f_first = np.cumsum([0] + [len(p.cutoff) for p in parts])
    shifted = lambda k, base: np.concatenate([getattr(p, k) + b for p, b in zip(parts, base)])   # noqa: E731
    return CVResult(spec=spec, status=cat('status'), n_folds=cat('n_folds'), n_holdout=cat('n_holdout'),
                    n_metric=cat('n_metric'), fold_series=shifted('fold_series', firsts), cutoff=cat('cutoff'),
                    hist_rows=cat('hist_rows'), hold_rows=cat('hold_rows'),
                    fit=_merge_fits(spec, [p.fit for p in parts], shared_grid=False),
                    row_fold=shifted('row_fold', f_first[:-1]), row_index=shifted('row_index', row_first), ds=cat('ds'), y=cat('y'), yhat=cat('yhat'),
                    yhat_lower=cat('yhat_lower') if intervals else None, yhat_upper=cat('yhat_upper') if intervals else None,
                    metric_series=shifted('metric_series', firsts), horizon=cat('horizon'), mse=cat('mse'),
                    rmse=cat('rmse'), mae=cat('mae'), mape=cat('mape'), coverage=cat('coverage') if intervals else None)


def performance_metrics(cv):
    """fbprophet's performance_metrics frame of a cross_validate result: one row per series and distinct horizon
    (series, horizon [ns], mse, rmse, mae, mape[, coverage]); the rolling window is the one cross_validate was given."""
    import pandas as pd
    d = {'series': cv.metric_series, 'horizon': cv.horizon, 'mse': cv.mse, 'rmse': cv.rmse, 'mae': cv.mae,
         'mape': cv.mape}
    if cv.coverage is not None:
        d['coverage'] = cv.coverage
    return pd.DataFrame(d)


class CVScores(object):
    """What score_cv returns.  quantiles [Q].  Per holdout row [R], in the CVResult's row order: pit, crps [R] and q,
    pinball [Q][R] (None without levels).  Per fold [F], the library's aggregates over the fold's holdout rows:
    fold_n_obs, fold_mean_crps [F], fold_mean_pinball, fold_coverage [F][Q].  Per series [N], over all its holdout rows in
    row order: n_obs (int64), mean_crps [N], mean_pinball, coverage [N][Q]; NaN (n_obs 0) for a series whose
    CVResult.status is not 0."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def cv_fold_keys(cv, series_key=None):
    """The interval stream key of every fold of a CVResult (include/tsf.h, cross-validation):
    (int64)((uint64)key_n * 0x9E3779B97F4A7C15 + (uint64)c) for fold c of series n; key_n = series_key[n] (None: n)."""
    N = len(cv.status)
    key = np.arange(N, dtype=np.int64) if series_key is None else np.ascontiguousarray(series_key, dtype=np.int64)
    if key.shape != (N,):
        raise ValueError('series_key must be [N]')
    F = len(cv.cutoff)
    c = (np.arange(F, dtype=np.int64) - cv.fold_offsets[:-1][cv.fold_series]).astype(np.uint64)
    with np.errstate(over='ignore'):
        return (key[cv.fold_series].view(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + c).view(np.int64)


def cv_fold_futures(cv, extra=None):
    """The holdout rows of a CVResult as one padded batch over its F folds -> (ds [F][Hmax], pad [F][Hmax] bool, row
    [F][Hmax] index into the [R] holdout rows, extra_future [F][n_extra][Hmax] or None): every fold's holdout dates,
    padded to the longest holdout by repeating its last one.  extra: the caller's [n_extra][len(ds)] columns."""
    F = len(cv.cutoff)
    hold = cv.hold_rows.astype(np.int64)
    Hm = int(hold.max()) if F else 0
    first = np.concatenate([[0], np.cumsum(hold)[:-1]]).astype(np.int64) if F else np.zeros(0, np.int64)
    j = np.arange(Hm, dtype=np.int64)[None, :]
    pad = j >= hold[:, None]
    row = first[:, None] + np.minimum(j, hold[:, None] - 1)
    exf = None
    if extra is not None:
        ex = np.asarray(extra, dtype=np.float64)
        exf = np.ascontiguousarray(np.moveaxis(ex[:, cv.row_index[row]], 0, 1))      # [n_extra][F][Hm] -> [F][n_extra][Hm]
    return cv.ds[row], pad, row, exf


def score_cv(cv, quantiles=(), floor=None, cap=None, extra=None, series_key=None, uncertainty_samples=1000, seed=0,
             ctx=None):
    """Every holdout row of a cross_validate result scored against its fold's predictive distribution -> CVScores: one
    score_actuals call over the F folds (fold f's model from cv.fit, its holdout dates padded to the longest holdout by
    repeating the last one, y NaN on the padding, the fold's stream key as in cross_validate).  floor / cap / extra /
    series_key: what cross_validate was given.  With the same uncertainty_samples and seed, the levels (1 - w) / 2 and
    (1 + w) / 2 give cross_validate's yhat_lower / yhat_upper at width w bit for bit."""
    levels = np.array(quantiles, dtype=np.float64).reshape(-1)
    Q = len(levels)
    N, F, R = len(cv.status), len(cv.cutoff), len(cv.y)
    spec = cv.spec
    if spec.extra and extra is None:
        raise ValueError('extra is required: the spec has extra columns')
    fs = cv.fold_series
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    nanv = lambda *shape: np.full(shape, np.nan)      # noqa: E731
    out = dict(quantiles=levels, pit=nanv(R), crps=nanv(R), q=nanv(Q, R) if Q else None,
               pinball=nanv(Q, R) if Q else None, fold_n_obs=np.zeros(F, np.int32), fold_mean_crps=nanv(F),
               fold_mean_pinball=nanv(F, Q) if Q else None, fold_coverage=nanv(F, Q) if Q else None,
               n_obs=np.zeros(N, np.int64), mean_crps=nanv(N), mean_pinball=nanv(N, Q) if Q else None,
               coverage=nanv(N, Q) if Q else None)
    if F == 0 or R == 0:
        return CVScores(**out)
    fut, pad, row, exf = cv_fold_futures(cv, extra if spec.extra else None)
    y_obs = np.where(pad, np.nan, cv.y[row])
    s = score_actuals(spec, cv.fit.theta, cv.fit.y_scale, cv.fit.grid, fut, y_obs, levels,
                      floor=None if fl is None else fl[fs], cap=None if cp is None else cp[fs], extra_future=exf,
                      series_key=cv_fold_keys(cv, series_key), uncertainty_samples=uncertainty_samples, seed=seed, ctx=ctx)
    real = ~pad
    out['pit'], out['crps'] = s.pit[real], s.crps[real]               # (row-major over [F][Hmax]: cv's row order)
    out['fold_n_obs'], out['fold_mean_crps'] = s.n_obs, s.mean_crps
    if Q:
        out['q'] = np.ascontiguousarray(np.moveaxis(s.q, 1, 0)[:, real])
        out['pinball'] = np.ascontiguousarray(np.moveaxis(s.pinball, 1, 0)[:, real])
        out['fold_mean_pinball'], out['fold_coverage'] = s.mean_pinball, s.coverage
    # per series: tsf_score_actuals' per-series rule on the host -- a left-to-right sum from +0.0 over its observed
    # holdout rows (np.cumsum of a 1-D array adds in index order)
    seq = lambda x: np.cumsum(np.concatenate([[0.0], x]))[-1]      # noqa: E731
    ro = cv.row_offsets
    for n in np.flatnonzero(np.asarray(cv.status) == 0):
        rows = np.arange(int(ro[n]), int(ro[n + 1]))
        obs = rows[~np.isnan(cv.y[rows])]
        out['n_obs'][n] = len(obs)
        if not len(obs):
            continue
        cnt = np.float64(len(obs))
        out['mean_crps'][n] = seq(out['crps'][obs]) / cnt
        for i in range(Q):
            out['mean_pinball'][n, i] = seq(out['pinball'][i, obs]) / cnt
            out['coverage'][n, i] = np.float64(np.count_nonzero(cv.y[obs] <= out['q'][i, obs])) / cnt
    return CVScores(**out)


def last_cv_grids(ctx=None):
    """tsf_last_cv_grids (include/tsf_dev.h): (grid tables built, fit launches) of the context's last
    cross_validate call."""
    ctx = ctx or get_context()
    g, n = ctypes.c_int64(), ctypes.c_int32()
    ctx.check(_lib.load().tsf_last_cv_grids(ctx.handle, ctypes.byref(g), ctypes.byref(n)))
    return int(g.value), int(n.value)


# ---- prior-scale tuning ----------------------------------------------------------------------------

TUNE_AXES = ('changepoint_prior_scale', 'seasonality_prior_scale', 'holidays_prior_scale')


def _n_holiday_columns(spec):
    from . import features
    return len(features.holiday_columns(spec.holidays)[0]) if spec.holidays else 0


def tune_candidates(spec, grid):
    """The candidates of a grid over TUNE_AXES (dict axis -> list of scales): itertools.product of the axes in
    TUNE_AXES order, the first varying slowest.  seasonality_prior_scale replaces the prior scale of every seasonality,
    the conditional ones (and so their columns of `extra`) included;
    holidays_prior_scale that of the holiday columns of `extra` (the first len(features.holiday_columns(spec.holidays)
    [0]) entries) -- regressors keep their own scale.  -> (candidates [ModelSpec], params {axis: float64 [C]})."""
    import itertools
    if not isinstance(grid, dict) or not grid:
        raise ValueError('grid must be a non-empty dict over %s' % (TUNE_AXES,))
    unknown = sorted(set(grid) - set(TUNE_AXES))
    if unknown:
        raise ValueError('unknown grid axes %s (tunable: %s)' % (unknown, TUNE_AXES))
    n_hol = _n_holiday_columns(spec)
    if 'seasonality_prior_scale' in grid and not (spec.seasonalities or spec.conditional):
        raise ValueError('grid over seasonality_prior_scale, but the model has no seasonality')
    if 'holidays_prior_scale' in grid and n_hol == 0:
        raise ValueError('grid over holidays_prior_scale, but the model has no holidays')
    axes = [k for k in TUNE_AXES if k in grid]
    values = []
    for k in axes:
        v = np.asarray(grid[k], dtype=np.float64).ravel()
        if v.size == 0:
            raise ValueError('grid axis %s is empty' % k)
        if not (np.isfinite(v).all() and (v > 0).all()):
            raise ValueError('grid axis %s: prior scales must be finite and > 0' % k)
        values.append(v)
    cands, params = [], {k: [] for k in axes}
    for combo in itertools.product(*values):
        # (the original form: the conditional seasonalities among `seasonalities`, lowered again by from_dict with the
        # candidate's scale -- copying spec.extra would lower them twice)
        d = spec.to_dict()
        d['seasonalities'] = [dict(s) for s in d['seasonalities']]
        d['extra'] = [dict(e) for e in d['extra']]
        for e in d['extra'][n_hol:]:          # (a regressor without its own scale would follow holidays_prior_scale)
            e.setdefault('prior_scale', spec.holidays_prior_scale)
        for k, v in zip(axes, combo):
            v = float(v)
            d[k] = v
            params[k].append(v)
            if k == 'seasonality_prior_scale':
                for s in d['seasonalities']:
                    s['prior_scale'] = v
            elif k == 'holidays_prior_scale':
                for e in d['extra'][:n_hol]:
                    e['prior_scale'] = v
        cands.append(ModelSpec.from_dict(d))
    return cands, {k: np.array(v) for k, v in params.items()}


def _effective_scales(spec, cands):
    """{axis: [C]} the scale each candidate gives the axis's columns (the first such column; NaN where it has none)."""
    n_hol = _n_holiday_columns(spec)
    cs = [c.to_c() for c in cands]

    def seas_scale(cand, c):        # (all seasonalities conditional: the first of their columns)
        if c.n_seas:
            return c.seas_prior_scale[0]
        return c.extra_prior_scale[cand.n_user_extra] if cand.conditional else np.nan
    return {'changepoint_prior_scale': np.array([c.changepoint_prior_scale for c in cs]),
            'seasonality_prior_scale': np.array([seas_scale(cand, c) for cand, c in zip(cands, cs)]),
            'holidays_prior_scale': np.array([c.extra_prior_scale[0] if n_hol else np.nan for c in cs])}


class TuneResult(object):
    """What tune returns (include/tsf.h tsf_tune).

    candidates [C] (ModelSpec), params {axis: [C]} (the grid value of each axis per candidate; with explicit candidates
    the scale each gives the axis's columns), metric; score / cand_status [N][C]; best / status [N] (best -1: no
    choice, status the plan's TSF_CV_* or TUNE_NO_SCORE); fit: FitResult of the refit (None without)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def spec_of(self, n):
        """The ModelSpec series n is refitted with: its choice, or the base spec where it has none."""
        b = int(self.best[n])
        return self.candidates[b] if b >= 0 else self.spec

    def frame(self):
        """One row per series: series, candidate (-1: none), status, the scales in effect (TUNE_AXES) and the score of
        the choice (NaN without one)."""
        import pandas as pd
        N = len(self.best)
        ok = self.best >= 0
        eff = _effective_scales(self.spec, list(self.candidates) + [self.spec])
        pick = np.where(ok, self.best, len(self.candidates))
        d = {'series': np.arange(N, dtype=np.int64), 'candidate': self.best.astype(np.int64),
             'status': self.status.astype(np.int64)}
        for k in TUNE_AXES:
            d[k] = eff[k][pick]
        d['metric'] = np.full(N, self.metric, dtype=object)
        d['score'] = np.where(ok, self.score[np.arange(N), np.maximum(self.best, 0)], np.nan)
        return pd.DataFrame(d)


def tune(spec, ds_ns, y, horizon, period=None, initial=None, offsets=None, floor=None, cap=None, extra=None,
         grid=None, candidates=None, metric='rmse', refit=True, ctx=None, devices=None):
    """Prophet's hyperparameter recipe for every series at once (include/tsf.h tsf_tune): cross_validate with each
    candidate's prior scales, score each series by `metric` over all its holdout rows (performance_metrics with
    rolling_window=1), keep the first minimum, and (refit) fit every series on its full history with its choice (the
    base spec where it has none).  Input as cross_validate.  grid: {axis: [scales]} over TUNE_AXES (tune_candidates),
    or candidates: explicit ModelSpecs that differ from spec in their prior scales only.  metric: mse / rmse / mae /
    mape.  devices: several GPUs, split by series.  Returns a TuneResult."""
    if (grid is None) == (candidates is None):
        raise ValueError('give exactly one of grid and candidates')
    if grid is not None:
        cands, params = tune_candidates(spec, grid)
    else:
        cands = list(candidates)
        if not cands:
            raise ValueError('candidates is empty')
        params = _effective_scales(spec, cands)
    if len(cands) > _lib.TUNE_MAX_CAND:
        raise ValueError('at most %d candidates' % _lib.TUNE_MAX_CAND)
    if metric not in _lib.TUNE_METRICS:
        raise ValueError('metric must be one of %s' % sorted(_lib.TUNE_METRICS))
    ds_ns, y, offsets, N, T = _cv_panel(ds_ns, y, offsets)
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    C = len(cands)

    def result(score, cst, best, sst, fit):
        return TuneResult(spec=spec, candidates=cands, params=params, metric=metric, score=score, cand_status=cst,
                          best=best, status=sst, fit=fit)
    devs = None if ctx is not None else resolve_devices(devices)
    if devs and N >= 2 * MIN_SERIES_PER_DEVICE:
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        lens = np.full(N, T, np.int64) if offsets is None else np.diff(offsets)
        cuts = _cuts(lens, parts)
        ex = None if extra is None else np.asarray(extra)

        def one(c, a, b):
            kw = dict(candidates=cands, metric=metric, refit=refit, ctx=c)
            if offsets is None:
                return tune(spec, ds_ns, y[a:b], horizon, period, initial, None, None if fl is None else fl[a:b],
                            None if cp is None else cp[a:b], extra, **kw)
            r0, r1 = int(offsets[a]), int(offsets[b])
            return tune(spec, ds_ns[r0:r1], y[r0:r1], horizon, period, initial, offsets[a:b + 1] - r0,
                        None if fl is None else fl[a:b], None if cp is None else cp[a:b],
                        None if ex is None else ex[:, r0:r1], **kw)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:]) if b > a]
        pr = _run_blocks(one, blocks)
        cat = lambda k: np.concatenate([getattr(p, k) for p in pr])     # noqa: E731
        fit = _merge_fits(spec, [p.fit for p in pr], shared_grid=offsets is None) if refit else None
        return result(cat('score'), cat('cand_status'), cat('best'), cat('status'), fit)
    ctx = ctx or get_context()
    L = _lib.load()
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (len(spec.extra), len(ds_ns)):
            raise ValueError('extra must be [n_extra][len(ds)]')
    base = spec.to_c()
    carr = (_lib.TsfSpec * C)(*[c.to_c() for c in cands])
    score = np.zeros((N, C))
    cst = np.zeros((N, C), np.int32)
    best = np.zeros(N, np.int32)
    sst = np.zeros(N, np.int32)
    fout, farrs = _alloc_out(N, spec.theta_stride, 1 if offsets is None else N) if refit else (_lib.TsfFitOut(), None)
    out = _lib.TsfTuneOut(score.ctypes.data, cst.ctypes.data, best.ctypes.data, sst.ctypes.data, fout)
    a = _cv_args(horizon, period, initial, 1.0)
    rc = L.tsf_tune(ctx.handle, ctypes.byref(base), carr, C, N, T, _lib._ptr(offsets), ds_ns.ctypes.data, y.ctypes.data,
                    _lib.y_dtype_code(y), _lib._ptr(fl), _lib._ptr(cp), _lib._ptr(ex), ctypes.byref(a),
                    _lib.TUNE_METRICS[metric], int(bool(refit)), ctypes.byref(out))
    ctx.check(rc)
    return result(score, cst, best, sst, FitResult(spec, *farrs) if refit else None)


def last_tune_counts(ctx=None):
    """tsf_last_tune_counts (include/tsf_dev.h): (fold panels cut, fit launches) of the context's last tune call."""
    ctx = ctx or get_context()
    e, f = ctypes.c_int32(), ctypes.c_int32()
    ctx.check(_lib.load().tsf_last_tune_counts(ctx.handle, ctypes.byref(e), ctypes.byref(f)))
    return int(e.value), int(f.value)


# ---- model-structure selection (include/tsf.h tsf_select) ---------------------------------------------------

SELECT_AXES = TUNE_AXES + ('seasonality_mode', 'growth', 'changepoint_range', 'n_changepoints')


def select_candidates(spec, grid):
    """The candidates of a grid over SELECT_AXES (dict axis -> list of values): itertools.product of the axes in
    SELECT_AXES order, the first varying slowest.  The prior-scale axes as tune_candidates; seasonality_mode sets the
    mode of every seasonality (the conditional ones included) and of the holiday columns of `extra` -- regressors keep
    theirs; growth, changepoint_range and n_changepoints replace the spec's (growth 'logistic' is allowed here: a
    missing cap is reported by the call).  -> (candidates [ModelSpec], params {axis: array [C]})."""
    import itertools
    if not isinstance(grid, dict) or not grid:
        raise ValueError('grid must be a non-empty dict over %s' % (SELECT_AXES,))
    unknown = sorted(set(grid) - set(SELECT_AXES))
    if unknown:
        raise ValueError('unknown grid axes %s (selectable: %s)' % (unknown, SELECT_AXES))
    n_hol = _n_holiday_columns(spec)
    if 'seasonality_prior_scale' in grid and not (spec.seasonalities or spec.conditional):
        raise ValueError('grid over seasonality_prior_scale, but the model has no seasonality')
    if 'holidays_prior_scale' in grid and n_hol == 0:
        raise ValueError('grid over holidays_prior_scale, but the model has no holidays')
    if 'n_changepoints' in grid and spec.specified_changepoints:
        raise ValueError('grid over n_changepoints, but the changepoint dates are specified')
    axes = [k for k in SELECT_AXES if k in grid]
    values = []
    for k in axes:
        v = list(np.asarray(grid[k]).ravel().tolist())
        if not v:
            raise ValueError('grid axis %s is empty' % k)
        if k in TUNE_AXES and not all(np.isfinite(x) and x > 0 for x in np.asarray(v, dtype=np.float64)):
            raise ValueError('grid axis %s: prior scales must be finite and > 0' % k)
        if k == 'n_changepoints' and not all(float(x) == int(x) and 0 <= int(x) <= _lib.MAX_S for x in v):
            raise ValueError('grid axis n_changepoints: integers in [0, %d]' % _lib.MAX_S)
        values.append(v)
    cands, params = [], {k: [] for k in axes}
    for combo in itertools.product(*values):
        d = spec.to_dict()                      # (the original form, as tune_candidates)
        d['seasonalities'] = [dict(s) for s in d['seasonalities']]
        d['extra'] = [dict(e) for e in d['extra']]
        for e in d['extra'][n_hol:]:            # (a regressor without its own would follow the axes)
            e.setdefault('prior_scale', spec.holidays_prior_scale)
            e.setdefault('mode', spec.seasonality_mode)
        for k, v in zip(axes, combo):
            v = int(v) if k == 'n_changepoints' else (str(v) if k in ('seasonality_mode', 'growth') else float(v))
            d[k] = v
            params[k].append(v)
            if k == 'seasonality_prior_scale':
                for s in d['seasonalities']:
                    s['prior_scale'] = v
            elif k == 'holidays_prior_scale':
                for e in d['extra'][:n_hol]:
                    e['prior_scale'] = v
            elif k == 'seasonality_mode':
                for s in d['seasonalities']:
                    s['mode'] = v
                for e in d['extra'][:n_hol]:
                    e['mode'] = v
        cands.append(ModelSpec.from_dict(d))    # (a bad growth / mode / range is ModelSpec's ValueError)
    return cands, {k: np.array(v) for k, v in params.items()}


def _select_axis_values(cands):
    """{axis: [C]} what each candidate carries for SELECT_AXES, and the names of its seasonalities."""
    d = {k: np.array([getattr(c, k) for c in cands]) for k in SELECT_AXES}
    d['seasonalities'] = np.array([','.join(str(s.get('name')) for s in c.seasonalities + c.conditional) for c in cands],
                                  dtype=object)
    return d


class SelectResult(object):
    """What select_model returns (include/tsf.h tsf_select).

    candidates [C] (ModelSpec), metric; score / cand_status [N][C]; best [N] (-1: the rule made no choice), chosen [N]
    (best, or the fallback: the candidate of the refit), status [N] (the plan's TSF_CV_* or TUNE_NO_SCORE); fit: the
    refit as the library returns it (None without) -- theta rows padded to the widest candidate's stride, grid [C] on an
    aligned panel (aligned = True) or [N]; groups() cuts it into one FitResult per candidate."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def spec_of(self, n):
        """The ModelSpec series n is refitted with."""
        return self.candidates[int(self.chosen[n])]

    def groups(self):
        """[(c, idx, FitResult)] for every candidate c some series was refitted with: idx the series (ascending), the
        FitResult their fits with theta cut to the candidate's stride and the candidate's grid(s) -- what every predict
        entry takes with candidates[c]."""
        if self.fit is None:
            raise ValueError('select_model ran without refit')
        out = []
        f = self.fit
        for c in np.unique(self.chosen):
            c = int(c)
            idx = np.flatnonzero(self.chosen == c)
            sp = self.candidates[c]
            grid = f.grid[c:c + 1] if self.aligned else f.grid[idx]
            out.append((c, idx, FitResult(sp, np.ascontiguousarray(f.theta[idx, :sp.theta_stride]), f.y_scale[idx],
                                          f.fval[idx], f.status[idx], f.n_iter[idx], f.n_eval[idx], grid)))
        return out

    def predict(self, ds_future_ns, floor=None, cap=None, extra_future=None, ctx=None):
        """yhat [N][H]: one predict per group with its candidate, placed by series.  ds_future_ns [H] or [N][H];
        floor / cap [N]; extra_future as predict's ([n_extra][H] shared, [N][n_extra][H] per series).  A series of a
        ragged panel that no fit reached (too few rows: its grid is empty, and predict refuses such a grid) is NaN."""
        N = len(self.chosen)
        fut = np.asarray(ds_future_ns, dtype=np.int64)
        fl, cp = _opt_f64(floor, N, 'floor'), _opt_f64(cap, N, 'cap')
        ex = None if extra_future is None else np.asarray(extra_future, dtype=np.float64)
        yhat = np.full((N, fut.shape[-1]), np.nan)
        for c, idx, f in self.groups():
            ok = np.arange(len(idx)) if self.aligned else np.flatnonzero(f.grid['t_scale_ns'] > 0)
            if ok.size == 0:
                continue
            sel = idx[ok]
            yhat[sel] = predict(f.spec, f.theta[ok], f.y_scale[ok], f.grid if self.aligned else f.grid[ok],
                                fut if fut.ndim == 1 else fut[sel], None if fl is None else fl[sel],
                                None if cp is None else cp[sel], ex if (ex is None or fut.ndim == 1) else ex[sel], ctx=ctx)
        return yhat

    def frame(self):
        """One row per series: series, candidate (the refit's), status, one column per axis of SELECT_AXES (and the
        seasonality names) that varies among the candidates, metric and the score of the choice (NaN without one)."""
        import pandas as pd
        N = len(self.chosen)
        d = {'series': np.arange(N, dtype=np.int64), 'candidate': self.chosen.astype(np.int64),
             'status': self.status.astype(np.int64)}
        for k, v in _select_axis_values(self.candidates).items():
            if len(set(v.tolist())) > 1:
                d[k] = v[self.chosen]
        d['metric'] = np.full(N, self.metric, dtype=object)
        d['score'] = self.score[np.arange(N), self.chosen]
        return pd.DataFrame(d)


def select_model(candidates, ds_ns, y, horizon, period=None, initial=None, offsets=None, floor=None, cap=None, extra=None,
                 metric='rmse', tolerance=0.0, fallback=0, refit=True, ctx=None, devices=None):
    """Choose the model structure per series by cross-validation in one call (include/tsf.h tsf_select): every candidate
    cross-validated as cross_validate(rolling_window=1) scores it, per series the lowest-numbered candidate within
    `tolerance` of the best score (order the candidates from simple to complex), and (refit) every series fitted on its
    full history with its choice -- `fallback` where it has none.  candidates: ModelSpecs that agree in their extra
    columns and optimiser options (select_candidates builds a grid of them).  Input as cross_validate.  devices: several
    GPUs, split by series.  Returns a SelectResult."""
    cands = list(candidates)
    C = len(cands)
    if C > _lib.TUNE_MAX_CAND:
        raise ValueError('at most %d candidates' % _lib.TUNE_MAX_CAND)
    if metric not in _lib.TUNE_METRICS:
        raise ValueError('metric must be one of %s' % sorted(_lib.TUNE_METRICS))
    ds_ns, y, offsets, N, T = _cv_panel(ds_ns, y, offsets)
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    aligned = offsets is None

    def result(score, cst, best, chosen, sst, fit):
        return SelectResult(candidates=cands, metric=metric, tolerance=float(tolerance), score=score, cand_status=cst,
                            best=best, chosen=chosen, status=sst, fit=fit, aligned=aligned)
    devs = None if ctx is not None else resolve_devices(devices)
    if devs and N >= 2 * MIN_SERIES_PER_DEVICE:
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        lens = np.full(N, T, np.int64) if aligned else np.diff(offsets)
        cuts = _cuts(lens, parts)
        ex = None if extra is None else np.asarray(extra)

        def one(c, a, b):
            kw = dict(metric=metric, tolerance=tolerance, fallback=fallback, refit=refit, ctx=c)
            if aligned:
                return select_model(cands, ds_ns, y[a:b], horizon, period, initial, None, None if fl is None else fl[a:b],
                                    None if cp is None else cp[a:b], extra, **kw)
            r0, r1 = int(offsets[a]), int(offsets[b])
            return select_model(cands, ds_ns[r0:r1], y[r0:r1], horizon, period, initial, offsets[a:b + 1] - r0,
                                None if fl is None else fl[a:b], None if cp is None else cp[a:b],
                                None if ex is None else ex[:, r0:r1], **kw)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:]) if b > a]
        pr = _run_blocks(one, blocks)
        cat = lambda k: np.concatenate([getattr(p, k) for p in pr])     # noqa: E731
        fit = None
        if refit:
            fit = _merge_fits(None, [p.fit for p in pr], shared_grid=aligned)
            if aligned:                 # grid[c]: from the first block that refitted a series with candidate c
                fit.grid = fit.grid.copy()
                for c in range(C):
                    for p in pr:
                        if any(p.fit.grid[c:c + 1].tobytes()):
                            fit.grid[c] = p.fit.grid[c]
                            break
        return result(cat('score'), cat('cand_status'), cat('best'), cat('chosen'), cat('status'), fit)
    ctx = ctx or get_context()
    L = _lib.load()
    n_extra = len(cands[0].extra) if cands else 0
    ex = None
    if n_extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (n_extra, len(ds_ns)):
            raise ValueError('extra must be [n_extra][len(ds)]')
    carr = (_lib.TsfSpec * max(C, 1))(*[c.to_c() for c in cands])
    stride_max = max([c.theta_stride for c in cands] + [1])
    if C >= 1 and L.tsf_select_stride(carr, C) != stride_max:
        raise _lib.TsfError('tsf_select_stride disagrees with ModelSpec.theta_stride')
    score = np.zeros((N, max(C, 1)))
    cst = np.zeros((N, max(C, 1)), np.int32)
    best = np.zeros(N, np.int32)
    chosen = np.zeros(N, np.int32)
    sst = np.zeros(N, np.int32)
    fout, farrs = _alloc_out(N, stride_max, C if aligned else N) if refit else (_lib.TsfFitOut(), None)
    out = _lib.TsfSelectOut(score.ctypes.data, cst.ctypes.data, best.ctypes.data, chosen.ctypes.data, sst.ctypes.data, fout)
    a = _cv_args(horizon, period, initial, 1.0)
    rc = L.tsf_select(ctx.handle, carr, C, N, T, _lib._ptr(offsets), ds_ns.ctypes.data, y.ctypes.data,
                      _lib.y_dtype_code(y), _lib._ptr(fl), _lib._ptr(cp), _lib._ptr(ex), ctypes.byref(a),
                      _lib.TUNE_METRICS[metric], float(tolerance), int(fallback), int(bool(refit)), ctypes.byref(out))
    ctx.check(rc)
    return result(score, cst, best, chosen, sst, FitResult(None, *farrs) if refit else None)


# ---- outlier screening: robust residual flags and refit (include/tsf.h) --------------------------------------

class Screen(object):
    """What the screening rule returns: flag (uint8, y's shape: 1 = excluded on input or flagged now), resid (y's shape),
    center / scale / n_new / n_flagged / status [N] (status: _lib.SCREEN_*); fitted (y's shape) where fc.screen made it."""

    def __init__(self, flag, resid, center, scale, n_new, n_flagged, status, fitted=None):
        self.flag, self.resid, self.center, self.scale = flag, resid, center, scale
        self.n_new, self.n_flagged, self.status, self.fitted = n_new, n_flagged, status, fitted


class ScreenedFit(object):
    """fit_screened's result: fit (FitResult, grid [N]: no fit has seen a flagged row), first (the first fit, as
    fit_aligned / fit_ragged return it), screen (Screen, flags cumulative), rounds [N] (rounds that gave new flags)."""

    def __init__(self, fit, first, screen, rounds):
        self.fit, self.first, self.screen, self.rounds = fit, first, screen, rounds


def _screen_args(threshold, max_share, min_rows, passes=1):
    """tsf_screen_args, refused here as the library refuses them (before it is loaded)."""
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError('threshold must be finite and > 0')
    if not 0.0 <= max_share <= 0.5:
        raise ValueError('max_share must be in [0, 0.5]')
    if int(min_rows) != min_rows or min_rows < 2:
        raise ValueError('min_rows must be an integer >= 2')
    if int(passes) != passes or not 1 <= passes <= 8:
        raise ValueError('passes must be an integer in [1, 8]')
    a = _lib.TsfScreenArgs()
    a.threshold, a.max_share, a.min_rows, a.max_passes = float(threshold), float(max_share), int(min_rows), int(passes)
    return a


def _screen_panel(y, offsets, other, what):
    """y (and arrays of y's layout) of a screening call: aligned [N][T], or 1-D with offsets [N+1]."""
    y = np.ascontiguousarray(y)
    if offsets is None:
        if y.ndim != 2:
            raise ValueError('aligned panel: y must be [N][T]')
        N, T = y.shape
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if y.ndim != 1 or offsets.ndim != 1 or len(offsets) < 1 or offsets[-1] != y.shape[0]:
            raise ValueError('ragged panel: y must be 1-D with offsets[-1] rows')
        N, T = len(offsets) - 1, 0
    for name, a in zip(what, other):
        if a is not None and a.shape != y.shape:
            raise ValueError('%s must have the shape of y' % name)
    return y, offsets, N, T


def _alloc_screen(y, N):
    flag = np.zeros(y.shape, np.uint8)
    resid = np.zeros(y.shape)
    center, scale = np.zeros(N), np.zeros(N)
    n_new, n_flagged, status = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    out = _lib.TsfScreenOut(flag.ctypes.data, resid.ctypes.data, center.ctypes.data, scale.ctypes.data,
                            n_new.ctypes.data, n_flagged.ctypes.data, status.ctypes.data)
    return out, (flag, resid, center, scale, n_new, n_flagged, status)


def screen_rows(y, fitted, offsets=None, excluded=None, min_scale=None, threshold=5.0, max_share=0.05, min_rows=10,
                ctx=None):
    """The screening rule (include/tsf.h tsf_screen_rows) on any (y, fitted): per series the median and the MAD of the
    residuals of the rows not excluded, a row flagged where |resid - center| exceeds both threshold * 1.4826 * MAD
    (at least min_scale[n]) and the budget's order statistic, so that at most max_share of a series' rows is ever
    flagged, `excluded` included.  y: [N][T], or 1-D with offsets [N+1] (float64 / float32 / int32); fitted, excluded:
    y's shape.  Returns a Screen."""
    fitted = np.ascontiguousarray(fitted, dtype=np.float64)
    ex = None if excluded is None else np.ascontiguousarray(np.asarray(excluded) != 0, dtype=np.uint8)
    y, offsets, N, T = _screen_panel(y, offsets, (fitted, ex), ('fitted', 'excluded'))
    ms = None if min_scale is None else np.ascontiguousarray(np.broadcast_to(np.asarray(min_scale, np.float64), (N,)))
    code = _lib.y_dtype_code(y)
    a = _screen_args(threshold, max_share, min_rows)
    ctx = ctx or get_context()
    L = _lib.load()
    out, arrs = _alloc_screen(y, N)
    ctx.check(L.tsf_screen_rows(ctx.handle, N, T, _lib._ptr(offsets), y.ctypes.data, code, fitted.ctypes.data,
                                _lib._ptr(ex), _lib._ptr(ms), ctypes.byref(a), ctypes.byref(out)))
    return Screen(*arrs)


def history_future(ds_ns, offsets):
    """A ragged panel's own dates as the padded future panel [N][Tmax] predict reads (rows past a series' last repeat
    its last date), and the row index [N][Tmax] into the panel that made it (for extra columns)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    Tmax = int(lens.max())
    idx = offsets[:-1, None] + np.minimum(np.arange(Tmax)[None, :], np.maximum(lens - 1, 0)[:, None])
    return np.asarray(ds_ns, dtype=np.int64)[idx], idx


def fitted_history(spec, fit, ds_ns, offsets=None, floor=None, cap=None, extra=None, ctx=None):
    """predict on the history's own dates, every row, in y's layout: what fit_screened screens against (aligned:
    shared dates ds [T]; ragged: per-series dates [N][Tmax], padded by the last date)."""
    if offsets is None:
        return predict(spec, fit.theta, fit.y_scale, fit.grid, ds_ns, floor=floor, cap=cap, extra_future=extra, ctx=ctx)
    offsets = np.asarray(offsets, dtype=np.int64)
    fut, idx = history_future(ds_ns, offsets)
    exf = None
    if spec.extra:
        exf = np.ascontiguousarray(np.asarray(extra, dtype=np.float64)[:, idx].transpose(1, 0, 2))
    yh = predict(spec, fit.theta, fit.y_scale, fit.grid, fut, floor=floor, cap=cap, extra_future=exf, ctx=ctx)
    lens = np.diff(offsets)
    return yh[np.arange(fut.shape[1])[None, :] < lens[:, None]]


def screen(spec, fit, ds_ns, y, offsets=None, floor=None, cap=None, extra=None, excluded=None, scale_floor=1e-8,
           threshold=5.0, max_share=0.05, min_rows=10, ctx=None):
    """One screening round of fit_screened by hand: fitted_history of `fit` (a FitResult of this panel), then screen_rows
    with min_scale = scale_floor * fit.y_scale.  Returns a Screen with .fitted."""
    y = np.ascontiguousarray(y)
    fitted = fitted_history(spec, fit, ds_ns, offsets, floor, cap, extra, ctx=ctx)
    s = screen_rows(y, fitted.reshape(y.shape), offsets=offsets, excluded=excluded,
                    min_scale=float(scale_floor) * np.asarray(fit.y_scale, dtype=np.float64), threshold=threshold,
                    max_share=max_share, min_rows=min_rows, ctx=ctx)
    s.fitted = fitted.reshape(y.shape)
    return s


def _merge_screens(parts, aligned):
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])     # noqa: E731
    return Screen(cat('flag'), cat('resid'), cat('center'), cat('scale'), cat('n_new'), cat('n_flagged'), cat('status'))


def fit_screened(spec, ds_ns, y, offsets=None, floor=None, cap=None, extra=None, threshold=5.0, max_share=0.05,
                 min_rows=10, scale_floor=1e-8, passes=1, ctx=None, devices=None):
    """Fit, screen, cut, refit in one call (include/tsf.h tsf_fit_screened): every series fitted on its full history,
    `passes` rounds of (predict on the history, screening rule, the flagged rows cut, the cut series fitted again).
    Input as fit_aligned (ds_ns [T], y [N][T], extra [n_extra][T]) or, with offsets [N+1], as fit_ragged.
    devices: several GPUs, split by series.  Returns a ScreenedFit."""
    ds_ns, y, offsets, N, T = _cv_panel(ds_ns, y, offsets)
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    a = _screen_args(threshold, max_share, min_rows, passes)
    if not (np.isfinite(scale_floor) and scale_floor >= 0):
        raise ValueError('scale_floor must be finite and >= 0')
    kw = dict(threshold=threshold, max_share=max_share, min_rows=min_rows, scale_floor=scale_floor, passes=passes)
    devs = None if ctx is not None else resolve_devices(devices)
    if devs and N >= 2 * MIN_SERIES_PER_DEVICE:
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        lens = np.full(N, T, np.int64) if offsets is None else np.diff(offsets)
        cuts = _cuts(lens, parts)
        ex = None if extra is None else np.asarray(extra)

        def one(c, a, b):
            if offsets is None:
                return fit_screened(spec, ds_ns, y[a:b], None, None if fl is None else fl[a:b],
                                    None if cp is None else cp[a:b], extra, ctx=c, **kw)
            r0, r1 = int(offsets[a]), int(offsets[b])
            return fit_screened(spec, ds_ns[r0:r1], y[r0:r1], offsets[a:b + 1] - r0, None if fl is None else fl[a:b],
                                None if cp is None else cp[a:b], None if ex is None else ex[:, r0:r1], ctx=c, **kw)
        blocks = [(c, int(a), int(b)) for c, a, b in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:]) if b > a]
        pr = _run_blocks(one, blocks)
        return ScreenedFit(_merge_fits(spec, [p.fit for p in pr], shared_grid=False),
                           _merge_fits(spec, [p.first for p in pr], shared_grid=offsets is None),
                           _merge_screens([p.screen for p in pr], offsets is None),
                           np.concatenate([p.rounds for p in pr]))
    ctx = ctx or get_context()
    L = _lib.load()
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (len(spec.extra), len(ds_ns)):
            raise ValueError('extra must be [n_extra][len(ds)]')
    cs = spec.to_c()
    fout, farrs = _alloc_out(N, spec.theta_stride, N)
    first, first_arrs = _alloc_out(N, spec.theta_stride, 1 if offsets is None else N)
    sout, sarrs = _alloc_screen(y, N)
    rounds = np.zeros(N, np.int32)
    out = _lib.TsfFitScreenedOut(fout, ctypes.pointer(first), sout, rounds.ctypes.data)
    rc = L.tsf_fit_screened(ctx.handle, ctypes.byref(cs), N, T, _lib._ptr(offsets), ds_ns.ctypes.data, y.ctypes.data,
                            _lib.y_dtype_code(y), _lib._ptr(fl), _lib._ptr(cp), _lib._ptr(ex), float(scale_floor),
                            ctypes.byref(a), ctypes.byref(out))
    ctx.check(rc)
    return ScreenedFit(FitResult(spec, *farrs), FitResult(spec, *first_arrs), Screen(*sarrs), rounds)


# ---- conformal interval calibration from cross-validation residuals (include/tsf.h) ---------------------------

def calibrated_columns(levels, prefix='yhat_lower_c'):
    """Column names of coverage levels: 0.8 -> 'yhat_lower_c80', 0.975 -> 'yhat_lower_c97.5' ('%s%s' % (prefix,
    format(100 * p, 'g')), the style of quantile_columns).  ValueError for a level that is not strictly inside (0, 1),
    for two levels with the same name and for more than CALIB_MAX_LEVELS levels."""
    lv = [float(p) for p in np.asarray(levels, dtype=np.float64).reshape(-1)]
    if not 1 <= len(lv) <= _lib.CALIB_MAX_LEVELS:
        raise ValueError('between 1 and %d coverage levels (got %d)' % (_lib.CALIB_MAX_LEVELS, len(lv)))
    names = []
    for p in lv:
        if not (np.isfinite(p) and 0.0 < p < 1.0):
            raise ValueError('coverage level %r: must be strictly inside (0, 1)' % (p,))
        name = '%s%s' % (prefix, format(100 * p, 'g'))
        if name in names:
            raise ValueError('coverage levels: two levels are named %s' % name)
        names.append(name)
    return names


def _calib_args(levels, mode, horizon, n_buckets, min_scores):
    """tsf_calib_args, refused here as the library refuses them (before it is loaded)."""
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    calibrated_columns(lv)
    if isinstance(mode, str):
        if mode not in _lib.CALIB_MODES:
            raise ValueError("mode must be 'abs' or 'cqr'")
        mode = _lib.CALIB_MODES[mode]
    if mode not in (_lib.CALIB_ABS, _lib.CALIB_CQR):
        raise ValueError("mode must be 'abs' or 'cqr'")
    if int(horizon) != horizon or horizon <= 0:
        raise ValueError('horizon must be an integer number of ns > 0')
    if int(n_buckets) != n_buckets or not 1 <= n_buckets <= _lib.CALIB_MAX_BUCKETS:
        raise ValueError('n_buckets must be an integer in [1, %d]' % _lib.CALIB_MAX_BUCKETS)
    if int(min_scores) != min_scores or min_scores < 1:
        raise ValueError('min_scores must be an integer >= 1')
    a = _lib.TsfCalibArgs()
    a.mode, a.n_levels, a.horizon_ns, a.n_buckets, a.min_scores = int(mode), len(lv), int(horizon), int(n_buckets), int(min_scores)
    for i, p in enumerate(lv):
        a.levels[i] = float(p)
    return a


class Calibration(object):
    """A calibration table (include/tsf.h tsf_calibrate_rows): q [N][B+1][L] (the conformity-score quantile per series,
    table row -- horizon buckets 0 .. B-1, then the pooled row B -- and level; NaN where fewer than min_scores scores),
    n [N][B+1][L] int32 (the scores behind each), status [N] (_lib.CALIB_*), levels [L] (coverage targets), mode
    (_lib.CALIB_ABS / CALIB_CQR), horizon (ns), n_buckets, min_scores.  cv: the CVResult where fc.calibrate was asked
    for it."""

    def __init__(self, q, n, status, levels, mode, horizon, n_buckets, min_scores, cv=None):
        self.q, self.n, self.status = q, n, status
        self.levels = np.array(levels, dtype=np.float64).reshape(-1)
        self.mode, self.horizon, self.n_buckets, self.min_scores = int(mode), int(horizon), int(n_buckets), int(min_scores)
        self.cv = cv

    def _args(self):
        return _calib_args(self.levels, self.mode, self.horizon, self.n_buckets, self.min_scores)

    @property
    def bucket_width(self):
        return (self.horizon + self.n_buckets - 1) // self.n_buckets

    def apply(self, yhat, ds_future, origin_ns, lower=None, upper=None, want_cell=False, ctx=None):
        """The table applied to a forecast (include/tsf.h tsf_apply_calibration): yhat [N][H], ds_future [H] or [N][H]
        (ns), origin_ns [N] (each model's last history timestamp), lower / upper [N][L][H] (CQR: the model's own bounds at
        each level) -> (lo, hi) [N][L][H], with want_cell also cell int8 [N][L][H] (the bucket used, n_buckets for the
        pooled row, -1 for none).  Rows inside the history use the first bucket and rows beyond the calibrated horizon
        the last one: extrapolations."""
        yhat = np.ascontiguousarray(yhat, dtype=np.float64)
        if yhat.ndim != 2:
            raise ValueError('yhat must be [N][H]')
        N, H = yhat.shape
        L = len(self.levels)
        if self.q.shape != (N, self.n_buckets + 1, L):
            raise ValueError('the table has %d series, yhat %d' % (self.q.shape[0], N))
        ds = np.ascontiguousarray(ds_future, dtype=np.int64)
        shared = ds.ndim == 1
        if ds.shape != ((H,) if shared else (N, H)):
            raise ValueError(_DS_FUTURE_SHAPE)
        origin = np.ascontiguousarray(np.broadcast_to(np.asarray(origin_ns, dtype=np.int64), (N,)))
        lw = up = None
        if self.mode == _lib.CALIB_CQR:
            if lower is None or upper is None:
                raise ValueError('a CQR table needs lower and upper')
            lw = np.ascontiguousarray(lower, dtype=np.float64)
            up = np.ascontiguousarray(upper, dtype=np.float64)
            if lw.shape != (N, L, H) or up.shape != (N, L, H):
                raise ValueError('lower / upper must be [N][L][H]')
        q = np.ascontiguousarray(self.q, dtype=np.float64)
        cnt = np.ascontiguousarray(self.n, dtype=np.int32)
        lo, hi = np.zeros((N, L, H)), np.zeros((N, L, H))
        cell = np.zeros((N, L, H), np.int8) if want_cell else None
        a = self._args()
        ctx = ctx or get_context()
        ctx.check(_lib.load().tsf_apply_calibration(ctx.handle, N, H, yhat.ctypes.data, _lib._ptr(lw), _lib._ptr(up),
                                                    ds.ctypes.data, int(shared), origin.ctypes.data, q.ctypes.data,
                                                    cnt.ctypes.data, ctypes.byref(a), lo.ctypes.data, hi.ctypes.data,
                                                    _lib._ptr(cell)))
        return (lo, hi, cell) if want_cell else (lo, hi)

    def frame(self, keys):
        """One row per series and table row.  keys: a dict (or DataFrame) of [N] series-key columns.  Columns: the keys,
        bucket (0 .. n_buckets, the last the pooled row), horizon_upto (ns: the bucket's largest horizon, the pooled
        row's the whole horizon), then n_c<..> and q_c<..> per level (calibrated_columns); then what from_frame needs
        to rebuild the table: calib_status per series and the settings calib_mode, calib_horizon, calib_min_scores."""
        import pandas as pd
        N, R = self.q.shape[0], self.n_buckets + 1
        cols = {}
        for k in (keys if isinstance(keys, dict) else {c: keys[c] for c in keys.columns}).items():
            v = np.asarray(k[1])
            if v.shape != (N,):
                raise ValueError('key column %s must be [N]' % k[0])
            cols[k[0]] = np.repeat(v, R)
        b = np.tile(np.arange(R, dtype=np.int32), N)
        cols['bucket'] = b
        cols['horizon_upto'] = np.minimum((b.astype(np.int64) + 1) * self.bucket_width, self.horizon)
        cols['horizon_upto'][b == self.n_buckets] = self.horizon
        for i, name in enumerate(calibrated_columns(self.levels, 'n_c')):
            cols[name] = self.n[:, :, i].reshape(-1)
        for i, name in enumerate(calibrated_columns(self.levels, 'q_c')):
            cols[name] = self.q[:, :, i].reshape(-1)
        cols['calib_status'] = np.repeat(self.status, R)
        cols['calib_mode'] = np.full(N * R, self.mode, np.int32)
        cols['calib_horizon'] = np.full(N * R, self.horizon, np.int64)
        cols['calib_min_scores'] = np.full(N * R, self.min_scores, np.int32)
        return pd.DataFrame(cols, columns=list(cols))

    @classmethod
    def from_frame(cls, df):
        """(Calibration, keys DataFrame [N]) of a frame made by .frame: the rows of a series are consecutive, buckets
        ascending; the levels are read back from the q_c<..> column names."""
        names = [c for c in df.columns if c.startswith('q_c')]
        if not names or len(df) == 0:
            raise ValueError('not a calibration frame')
        levels = [float(c[3:]) / 100.0 for c in names]
        for c, want in zip(names, calibrated_columns(levels, 'q_c')):
            if c != want:
                raise ValueError('calibration frame: column %s does not name a level' % c)
        R = int(df['bucket'].max()) + 1
        if len(df) % R or not np.array_equal(df['bucket'].values, np.tile(np.arange(R), len(df) // R)):
            raise ValueError('calibration frame: every series needs its buckets 0 .. %d in order' % (R - 1))
        N, L = len(df) // R, len(names)
        q = np.stack([df[c].values.astype(np.float64).reshape(N, R) for c in names], axis=2)
        n = np.stack([df['n_c' + c[3:]].values.astype(np.int32).reshape(N, R) for c in names], axis=2)
        fixed = ['bucket', 'horizon_upto', 'calib_status', 'calib_mode', 'calib_horizon', 'calib_min_scores']
        kcols = [c for c in df.columns if c not in fixed and not c.startswith('q_c') and not c.startswith('n_c')]
        keys = df.iloc[::R][kcols].reset_index(drop=True)
        cal = cls(np.ascontiguousarray(q), np.ascontiguousarray(n), df['calib_status'].values[::R].astype(np.int32), levels,
                  int(df['calib_mode'].iloc[0]), int(df['calib_horizon'].iloc[0]), R - 1, int(df['calib_min_scores'].iloc[0]))
        return cal, keys


def _alloc_calib(N, B, L):
    q, n, st = np.zeros((N, B + 1, L)), np.zeros((N, B + 1, L), np.int32), np.zeros(N, np.int32)
    return _lib.TsfCalibTable(q.ctypes.data, n.ctypes.data, st.ctypes.data), (q, n, st)


def calibrate_rows(row_offsets, horizon_ns, y, yhat, levels, lower=None, upper=None, mode='abs', horizon=None,
                   n_buckets=10, min_scores=20, ctx=None):
    """The calibration rule alone (include/tsf.h tsf_calibrate_rows) on a ragged set of out-of-sample rows: series n owns
    rows [row_offsets[n], row_offsets[n + 1]) of horizon_ns (int64: ds - cutoff), y, yhat; lower / upper [L][R] under
    'cqr'.  Per series, horizon bucket (n_buckets of them over (0, horizon], plus one pooled row) and level: the
    ceil((m + 1) * level)-th smallest of the m conformity scores |y - yhat| ('abs') or max(lower - y, y - upper) ('cqr'),
    NaN below min_scores.  horizon: ns (required).  Returns a Calibration."""
    if horizon is None:
        raise ValueError('horizon (ns) is required')
    a = _calib_args(levels, mode, horizon, n_buckets, min_scores)
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError('row_offsets must be [N+1]')
    N, R, L = len(off) - 1, int(off[-1]), a.n_levels
    h = np.ascontiguousarray(horizon_ns, dtype=np.int64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    yhat = np.ascontiguousarray(yhat, dtype=np.float64)
    if h.shape != (R,) or y.shape != (R,) or yhat.shape != (R,):
        raise ValueError('horizon_ns, y and yhat must be [row_offsets[-1]]')
    lw = up = None
    if a.mode == _lib.CALIB_CQR:
        if lower is None or upper is None:
            raise ValueError("mode 'cqr' needs lower and upper")
        lw = np.ascontiguousarray(lower, dtype=np.float64).reshape(-1, R) if R else np.zeros((L, 0))
        up = np.ascontiguousarray(upper, dtype=np.float64).reshape(-1, R) if R else np.zeros((L, 0))
        if lw.shape != (L, R) or up.shape != (L, R):
            raise ValueError('lower / upper must be [L][R]')
    ctx = ctx or get_context()
    tab, (q, n, st) = _alloc_calib(N, a.n_buckets, L)
    ctx.check(_lib.load().tsf_calibrate_rows(ctx.handle, N, off.ctypes.data, h.ctypes.data, y.ctypes.data, yhat.ctypes.data,
                                             _lib._ptr(lw), _lib._ptr(up), ctypes.byref(a), ctypes.byref(tab)))
    return Calibration(q, n, st, np.array(a.levels[:L]), a.mode, a.horizon_ns, a.n_buckets, a.min_scores)


def _calib_mask(cal, cv_status):
    """tsf_calibrate's rule for a series whose cross-validation did not end CV_OK: no table."""
    bad = np.asarray(cv_status) != _lib.CV_OK
    cal.q[bad], cal.n[bad], cal.status[bad] = np.nan, 0, _lib.CALIB_NO_SCORES
    return cal


def cv_interval_levels(levels):
    """The tail pairs of coverage levels p as quantile levels: [(1 - p) / 2 ..., (1 + p) / 2 ...] (2 L of them)."""
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    return np.concatenate([(1.0 - lv) / 2.0, (1.0 + lv) / 2.0])


def calibrate_cv(cv, levels, mode='abs', n_buckets=10, min_scores=20, horizon=None, interval_width=None, floor=None,
                 cap=None, extra=None, series_key=None, uncertainty_samples=1000, seed=0, ctx=None):
    """The calibration rule on a cross_validate result -> Calibration: the rows are the CVResult's holdout rows, their
    horizon ds - cutoff.  horizon: the cross-validation's (ns; None: the largest horizon of the result's metric rows).
    'cqr': each level's bounds come from score_cv(cv, quantiles=cv_interval_levels(levels)).q -- floor / cap / extra /
    series_key / uncertainty_samples / seed are score_cv's, what cross_validate was given -- except that ONE level equal
    to interval_width (the width cross_validate was given, with intervals=True) uses the CVResult's own yhat_lower /
    yhat_upper.
    A series whose cv.status is not CV_OK gets no table (CALIB_NO_SCORES), as in fc.calibrate."""
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    if horizon is None:
        if len(cv.horizon) == 0:
            raise ValueError('horizon is required: the CVResult has no metric row to read it from')
        horizon = int(np.max(cv.horizon))
    h = cv.ds - cv.cutoff[cv.row_fold]
    lw = up = None
    m = _lib.CALIB_MODES.get(mode, mode)
    if m == _lib.CALIB_CQR:
        if len(lv) == 1 and cv.yhat_lower is not None and interval_width is not None and lv[0] == float(interval_width):
            lw, up = cv.yhat_lower[None, :], cv.yhat_upper[None, :]
        else:
            s = score_cv(cv, quantiles=cv_interval_levels(lv), floor=floor, cap=cap, extra=extra, series_key=series_key,
                         uncertainty_samples=uncertainty_samples, seed=seed, ctx=ctx)
            lw, up = s.q[:len(lv)], s.q[len(lv):]
    cal = calibrate_rows(cv.row_offsets, h, cv.y, cv.yhat, lv, lower=lw, upper=up, mode=mode, horizon=horizon,
                         n_buckets=n_buckets, min_scores=min_scores, ctx=ctx)
    return _calib_mask(cal, cv.status)


def _merge_calibrations(parts, cv):
    p0 = parts[0]
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])     # noqa: E731
    return Calibration(cat('q'), cat('n'), cat('status'), p0.levels, p0.mode, p0.horizon, p0.n_buckets, p0.min_scores, cv)


def calibrate(spec, ds_ns, y, horizon, levels, mode='abs', n_buckets=10, min_scores=20, period=None, initial=None,
              offsets=None, floor=None, cap=None, extra=None, rolling_window=0.1, uncertainty_samples=1000,
              interval_width=0.8, seed=0, series_key=None, want_cv=False, ctx=None, devices=None):
    """Cross-validation and calibration rule in one call (include/tsf.h tsf_calibrate): input as cross_validate; the rule
    runs on the device's own holdout forecasts and only the table comes back (with want_cv the CVResult too, as
    Calibration.cv: cross_validate's bit for bit).  'abs' runs the folds without intervals; 'cqr' takes ONE level equal
    to interval_width and reads the folds' own yhat_lower / yhat_upper (cross_validate with intervals=True).  devices:
    several GPUs, split by series as cross_validate splits.  Returns a Calibration equal to
    calibrate_cv(cross_validate(...), ...) bit for bit."""
    ds_ns, y, offsets, N, T = _cv_panel(ds_ns, y, offsets)
    a = _calib_args(levels, mode, horizon, n_buckets, min_scores)
    cqr = a.mode == _lib.CALIB_CQR
    if cqr and not (a.n_levels == 1 and a.levels[0] == float(interval_width)):
        raise ValueError("mode 'cqr' in the one call takes one level equal to interval_width (several levels: "
                         "cross_validate, then calibrate_cv)")
    fl = _opt_f64(floor, N, 'floor')
    cp = _opt_f64(cap, N, 'cap')
    key = None if series_key is None else np.ascontiguousarray(series_key, dtype=np.int64)
    if key is not None and key.shape != (N,):
        raise ValueError('series_key must be [N]')
    kw = dict(mode=mode, n_buckets=n_buckets, min_scores=min_scores, period=period, initial=initial,
              rolling_window=rolling_window, uncertainty_samples=uncertainty_samples, interval_width=interval_width,
              seed=seed, want_cv=want_cv)
    devs = None if ctx is not None else resolve_devices(devices)
    if devs and N >= 2 * MIN_SERIES_PER_DEVICE:
        parts = min(len(devs), N // MIN_SERIES_PER_DEVICE)
        lens = np.full(N, T, np.int64) if offsets is None else np.diff(offsets)
        cuts = _cuts(lens, parts)
        key = np.arange(N, dtype=np.int64) if key is None else key       # (the same streams whatever the split)
        ex = None if extra is None else np.asarray(extra)

        def one(c, a_, b_):
            if offsets is None:
                return calibrate(spec, ds_ns, y[a_:b_], horizon, levels, offsets=None, floor=None if fl is None else fl[a_:b_],
                                 cap=None if cp is None else cp[a_:b_], extra=extra, series_key=key[a_:b_], ctx=c, **kw)
            r0, r1 = int(offsets[a_]), int(offsets[b_])
            return calibrate(spec, ds_ns[r0:r1], y[r0:r1], horizon, levels, offsets=offsets[a_:b_ + 1] - r0,
                             floor=None if fl is None else fl[a_:b_], cap=None if cp is None else cp[a_:b_],
                             extra=None if ex is None else ex[:, r0:r1], series_key=key[a_:b_], ctx=c, **kw)
        blocks = [(c, int(a_), int(b_)) for c, a_, b_ in zip(_contexts(devs[:parts]), cuts[:-1], cuts[1:]) if b_ > a_]
        pr = _run_blocks(one, blocks)
        cv = None
        if want_cv:
            row_first = [0 if offsets is None else int(offsets[a_]) for _, a_, _ in blocks]
            cv = _merge_cv(spec, [p.cv for p in pr], [a_ for _, a_, _ in blocks], cqr, row_first)
        return _merge_calibrations(pr, cv)
    ctx = ctx or get_context()
    L = _lib.load()
    cs = spec.to_c()
    ex = None
    if spec.extra:
        ex = np.ascontiguousarray(extra, dtype=np.float64)
        if ex.shape != (len(spec.extra), len(ds_ns)):
            raise ValueError('extra must be [n_extra][len(ds)]')
    tab, (q, n, st) = _alloc_calib(N, a.n_buckets, a.n_levels)
    ca = _cv_args(horizon, period, initial, rolling_window)
    out_p, cv = None, None
    if want_cv:
        plan = cv_plan(ds_ns, horizon, period, initial, rolling_window, offsets=offsets, N=N)
        F, R, M = int(plan['n_folds'].sum()), int(plan['n_holdout'].sum()), int(plan['n_metric'].sum())
        fout, farrs = _alloc_out(F, spec.theta_stride, F)
        yhat = np.zeros(R)
        lo = np.zeros(R) if cqr else None
        hi = np.zeros(R) if cqr else None
        hz = np.zeros(M, np.int64)
        mse, rmse, mae, mape = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
        cov = np.zeros(M) if cqr else None
        sst = np.zeros(N, np.int32)
        out = _lib.TsfCvOut(fout, yhat.ctypes.data, _lib._ptr(lo), _lib._ptr(hi), hz.ctypes.data, mse.ctypes.data,
                            rmse.ctypes.data, mae.ctypes.data, mape.ctypes.data, _lib._ptr(cov), sst.ctypes.data)
        out_p = ctypes.byref(out)
    rc = L.tsf_calibrate(ctx.handle, ctypes.byref(cs), N, T, _lib._ptr(offsets), ds_ns.ctypes.data, y.ctypes.data,
                         _lib.y_dtype_code(y), _lib._ptr(fl), _lib._ptr(cp), _lib._ptr(ex), ctypes.byref(ca),
                         _lib._ptr(key), int(uncertainty_samples) if cqr else 0, float(interval_width), int(seed),
                         ctypes.byref(a), ctypes.byref(tab), out_p)
    ctx.check(rc)
    if want_cv:
        fold_series = np.repeat(np.arange(N, dtype=np.int64), plan['n_folds'])
        start = (np.zeros(N, np.int64) if offsets is None else offsets[:-1])[fold_series] + plan['hist_rows']
        ridx = np.repeat(start - np.concatenate([[0], np.cumsum(plan['hold_rows'])[:-1]]), plan['hold_rows']) + np.arange(R)
        row_fold = np.repeat(np.arange(F, dtype=np.int64), plan['hold_rows'])
        y_rows = (y[fold_series[row_fold], ridx] if offsets is None else y[ridx]).astype(np.float64)
        cv = CVResult(spec=spec, status=sst, n_folds=plan['n_folds'], n_holdout=plan['n_holdout'], n_metric=plan['n_metric'],
                      fold_series=fold_series, cutoff=plan['cutoff'], hist_rows=plan['hist_rows'], hold_rows=plan['hold_rows'],
                      fit=FitResult(spec, *farrs), row_fold=row_fold, row_index=ridx, ds=ds_ns[ridx], y=y_rows, yhat=yhat,
                      yhat_lower=lo, yhat_upper=hi,
                      metric_series=np.repeat(np.arange(N, dtype=np.int64), plan['n_metric']), horizon=hz, mse=mse,
                      rmse=rmse, mae=mae, mape=mape, coverage=cov)
    return Calibration(q, n, st, np.array(a.levels[:a.n_levels]), a.mode, a.horizon_ns, a.n_buckets, a.min_scores, cv)


def model_origin_ns(grid, N=None):
    """Each model's last history timestamp from its grid: start_ns + t_scale_ns ([N]; one shared grid repeats)."""
    g = np.ascontiguousarray(grid, dtype=_lib.GRID_DTYPE)
    o = g['start_ns'].astype(np.int64) + g['t_scale_ns'].astype(np.int64)
    return np.ascontiguousarray(np.broadcast_to(o, (N,))) if N is not None and len(o) == 1 else o


def predict_calibrated(spec, theta, y_scale, grid, ds_future_ns, cal, floor=None, cap=None, extra_future=None,
                       series_key=None, uncertainty_samples=1000, seed=0, want_cell=False, ctx=None):
    """predict, then the calibration table `cal` applied with each model's origin from its grid -> (yhat [N][H], lo, hi
    [N][L][H][, cell]).  An 'abs' table needs the point forecast only; a 'cqr' table first takes the model's own bounds at
    each level's tail pair from predict_quantiles (series_key / uncertainty_samples / seed: its arguments).  yhat is
    predict's bit for bit."""
    N = len(theta)
    lw = up = None
    if cal.mode == _lib.CALIB_CQR:
        L = len(cal.levels)
        pq = predict_quantiles(spec, theta, y_scale, grid, ds_future_ns, cv_interval_levels(cal.levels), floor=floor, cap=cap,
                               extra_future=extra_future, series_key=series_key, uncertainty_samples=uncertainty_samples,
                               seed=seed, ctx=ctx)
        yhat, lw, up = pq.yhat, np.ascontiguousarray(pq.q[:, :L]), np.ascontiguousarray(pq.q[:, L:])
    else:
        yhat = predict(spec, theta, y_scale, grid, ds_future_ns, floor=floor, cap=cap, extra_future=extra_future, ctx=ctx)
    res = cal.apply(yhat, ds_future_ns, model_origin_ns(grid, N), lower=lw, upper=up, want_cell=want_cell, ctx=ctx)
    return (yhat,) + tuple(res)
