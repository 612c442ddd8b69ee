/*
 * tsf.h -- C ABI of libtsf_amd.so: batched per-series Prophet-model MAP fit + predict on
 * MI355X (gfx950).  Plain pointers and sizes, no C++/torch types, no exceptions.
 *
 * What each entry point replaces in the reference (mageky/time-series-spark):
 *
 *   tsf_fit_aligned / tsf_fit_ragged (+ _dev)
 *       `Prophet(growth=..., seasonality_mode=...)` + `model.fit(pdf)` executed once per
 *       (series_id, dim_id) group inside the grouped-map pandas_udf
 *       /root/reference/src/jobs/prophet_modeler.py:56-66 (floor :56-57, cap :59-60,
 *       constructor :65, fit :66), i.e. fbprophet 0.5 setup_dataframe / set_changepoints /
 *       make_all_seasonality_features / *_growth_init and pystan 2.19.1.1
 *       StanModel.optimizing(algorithm='LBFGS' | 'Newton', see tsf_spec.algorithm) on
 *       prophet.stan -- for a whole panel of series in one call.
 *   tsf_predict (+ _dev)
 *       `model.predict(future_df)` + the int cast + floor clamp of
 *       /root/reference/src/jobs/prophet_scorer.py:64-84 (future frame :64-68, predict :70,
 *       astype(int) :73, clamp :76-84).  Only `yhat` is produced: the reference keeps
 *       nothing else (:86).  (tsf_predict_components adds the trend and the components.)
 *   (tests and measurements -- per-evaluation hooks, route switches, kernel timers -- are NOT here: include/tsf_dev.h)
 *
 * Conventions
 *   - Every function returns 0 on success, <0 on API misuse / HIP failure
 *     (tsf_last_error(ctx) gives the text).  Per-series outcomes go to status[] (TSF_ST_*),
 *     mirroring the reference's "RuntimeError -> series dropped" (prophet_modeler.py:81-85)
 *     vs "ValueError propagates" split: the Python layer decides what to raise.
 *   - All buffers are caller-allocated and caller-owned.  `_dev` variants take DEVICE
 *     pointers on the context's GPU plus a hipStream_t (as void*, NULL = default stream) and
 *     are asynchronous; the plain variants take HOST pointers, copy in, run, copy out, sync.
 *   - A tsf_ctx is bound to one GPU and is not re-entrant; use one per GPU / host thread.
 *   - Timestamps are int64 nanoseconds since the Unix epoch (pandas datetime64[ns]), sorted
 *     ascending within a series, rows with NaN y already removed (fbprophet
 *     setup_dataframe does both on the host as well).
 *   - theta layout per series, stride tsf_theta_stride(spec):
 *       [k, m, log(sigma_obs), delta[n_changepoints], beta[K]]
 *     beta in design-column order: seasonalities in spec order, each
 *     [sin1, cos1, sin2, cos2, ...], then the extra (holiday / regressor) columns.
 *     When a series is too short for n_changepoints, S < n_changepoints and the unused
 *     deltas are 0.
 */
#ifndef TSF_H
#define TSF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSF_MAX_SEAS 8
#define TSF_MAX_EXTRA 64
#define TSF_MAX_S 60          /* max changepoints */
#define TSF_MAX_K 64          /* max design columns */
#define TSF_MAX_P 128         /* 3 + S + K */
#define TSF_MAX_T 1048576     /* rows per series (a series is one wavefront's work: 64 chunks of
                                 ceil(T/64) rows); every fit entry point rejects longer input */

enum { TSF_GROWTH_LINEAR = 0, TSF_GROWTH_LOGISTIC = 1 };
enum { TSF_MODE_ADDITIVE = 0, TSF_MODE_MULTIPLICATIVE = 1 };
enum { TSF_Y_F64 = 0, TSF_Y_F32 = 1, TSF_Y_I32 = 2 };
enum { TSF_EVAL_AUTO = 0, TSF_EVAL_RESIDUAL = 1, TSF_EVAL_QUADRATIC = 2 };
/* Which of Stan's optimisers runs the MAP fit.  fbprophet 0.5 chooses
 * `'Newton' if T < 100 else 'LBFGS'` (TSF_ALGO_AUTO: decided per CALL from the longest series of
 * the call -- callers split panels at 100 rows).  Default TSF_ALGO_LBFGS.
 * Newton kernels: one parameter per lane for models of up to 64 parameters (3 + n_changepoints + K) of one
 * column mode -- quadratic-form evaluations, several series per wave, for linear / additive models of up to 28
 * design columns --; two parameters per lane (round 4, one wave and ~140 KB of LDS per series: slow, meant for the
 * handful of series fbprophet retries after a failed L-BFGS fit) up to TSF_MAX_P = 128 and for mixed additive /
 * multiplicative columns.  Every model the library fits has one. */
enum { TSF_ALGO_LBFGS = 0, TSF_ALGO_NEWTON = 1, TSF_ALGO_AUTO = 2 };
enum { TSF_RK_AUTO = 0, TSF_RK_WAVE = 1, TSF_RK_MFMA = 2, TSF_RK_COOP = 3 };
/* What a fit converges to.  TSF_CONVERGE_STAN (default): Stan's optimiser under Stan's termination tests -- what
 * `Prophet.fit` returns (prophet_modeler.py:66): the point where the tests fire, a median 1e-3 .. 1e-2 away from the
 * optimum in forecast, because L-BFGS stalls on the kinks of the Laplace prior on the changepoints.
 * TSF_CONVERGE_MAP: from that point on to the maximum a posteriori estimate of prophet.stan's model itself (an
 * orthant-wise active-set L-BFGS on the same log-posterior, tsf_map_kernels.h): forecasts that are a property of the
 * model, not of a floating-point trajectory.  status then is TSF_ST_MAP_*; n_iter / n_eval count both phases.
 * For linear growth with additive seasonality (<= 64 parameters) the estimate is computed directly, without the Stan-rule
 * fit before it (tsf_map_quad.h: sigma in closed form and an L1-regularised quadratic programme by an active-set method,
 * in turn): n_iter then counts those rounds, n_eval the Cholesky solves + 1, and the call is faster than a Stan-rule fit. */
enum { TSF_CONVERGE_STAN = 0, TSF_CONVERGE_MAP = 1 };
#define TSF_NEWTON_BELOW_T 100

/* per-series status: >= 0 are Stan's optimiser termination codes */
enum {
    TSF_ST_CONTINUE = 0,       /* never returned */
    TSF_ST_ABSX = 10, TSF_ST_ABSF = 20, TSF_ST_RELF = 21, TSF_ST_ABSGRAD = 30,
    TSF_ST_RELGRAD = 31, TSF_ST_MAXIT = 40,
    TSF_ST_CONSTANT = 50,      /* constant y, linear growth: fbprophet skips optimisation */
    TSF_ST_NEWTON_CONVERGED = 60, /* Newton: |lp - last lp| < 1e-8 */
    /* tsf_spec.converge = TSF_CONVERGE_MAP: how the continuation to the maximum a posteriori estimate ended */
    TSF_ST_MAP_KKT = 70,       /* KKT residual (largest one-sided derivative that still descends) <= map_tol */
    TSF_ST_MAP_FTOL = 71,      /* 20 iterations together gained < 1e-13 |f|: the function value has converged */
    TSF_ST_MAP_MAXIT = 72,     /* map_max_iter iterations (the direct solver: 120 rounds or 3 000 solves) */
    TSF_ST_MAP_LS = 73,        /* no lower point along the steepest one-sided descent direction either (rounding level) */
    TSF_ST_NEWTON_FAIL = -4,   /* Newton: log_prob threw inside the finite-difference Hessian */
    TSF_ST_LSFAIL = -1,        /* line search failed (pystan raises RuntimeError) */
    TSF_ST_INIT_NONFINITE = -2,/* log_prob non-finite at the initial point (RuntimeError) */
    TSF_ST_EVAL_LIMIT = -3,    /* > 64*max_iter+1024 evaluations: the line search never settled
                                  (guard; treated like LSFAIL) */
    TSF_ST_TOO_FEW = -10,      /* < 2 rows (fbprophet raises ValueError) */
    TSF_ST_CAP = -11,          /* cap <= floor (fbprophet raises ValueError) */
    TSF_ST_CHANGEPOINT = -12   /* a specified changepoint outside [min ds, max ds] of the series (fbprophet raises
                                  ValueError('Changepoints must fall within training data.')) */
};

/* Model + optimiser settings shared by every series of a call.  Defaults = fbprophet 0.5
 * Prophet.__init__ and stan::services::optimize::lbfgs as pystan 2.19 drives it. */
typedef struct {
    int32_t growth;                         /* TSF_GROWTH_* */
    int32_t n_changepoints;                 /* 25 */
    double changepoint_range;               /* 0.8 */
    double changepoint_prior_scale;         /* tau = 0.05 */
    int32_t n_seas;                         /* Fourier seasonalities */
    int32_t n_extra;                        /* explicit design columns (holidays, regressors) */
    double seas_period[TSF_MAX_SEAS];       /* days: 365.25, 7, 1 */
    double seas_prior_scale[TSF_MAX_SEAS];  /* 10 */
    int32_t seas_order[TSF_MAX_SEAS];       /* 10, 3, 4 */
    int32_t seas_mode[TSF_MAX_SEAS];        /* TSF_MODE_* */
    double extra_prior_scale[TSF_MAX_EXTRA];
    int32_t extra_mode[TSF_MAX_EXTRA];
    int32_t max_iter;                       /* 10000 */
    int32_t history;                        /* 5 */
    double init_alpha;                      /* 1e-3 */
    double tol_obj;                         /* 1e-12 */
    double tol_rel_obj;                     /* 1e4  (x DBL_EPSILON) */
    double tol_grad;                        /* 1e-8 */
    double tol_rel_grad;                    /* 1e7  (x DBL_EPSILON) */
    double tol_param;                       /* 1e-8 */
    /* How the normal likelihood's data term is evaluated (same function, different rounding):
     * TSF_EVAL_RESIDUAL sums residuals over the T rows at every evaluation; TSF_EVAL_QUADRATIC
     * uses SSE(theta) = s0 - 2 c.D + D.(Z^T Z) D around a re-centred reference point -- only
     * possible where the mean is linear in (k, m, delta, beta): linear growth, every column
     * additive (and history == 5).  TSF_EVAL_AUTO picks QUADRATIC where possible; the choice
     * depends on the MODEL only, never on the shape or composition of the panel. */
    int32_t eval_form;                      /* TSF_EVAL_AUTO */
    int32_t recenter_every;                 /* 128: re-centre at least every n accepted iterations */
    double recenter_ratio;                  /* 1.0: ... and when |Z D|^2 > ratio * s0 */
    int32_t algorithm;                      /* TSF_ALGO_LBFGS */
    /* Which kernel runs a RESIDUAL-form L-BFGS fit (same arithmetic, same bits): TSF_RK_WAVE one
     * wavefront per series; TSF_RK_MFMA 16 series per workgroup evaluated together on the matrix
     * cores (aligned panels, one parameter per lane, <= 28 changepoints); TSF_RK_AUTO = WAVE with
     * the cooperative tail: the series still running when the launch has handed out its last series
     * are suspended and finished by one WORKGROUP each (8 waves sharing every evaluation; series of
     * at most 4096 rows) -- and models with more than 64 parameters (two per lane) run on workgroups from
     * their first evaluation, the workgroup kernel being the faster one for them; TSF_RK_COOP = every
     * series on a workgroup from its first evaluation (lowest latency for panels smaller than the GPU). */
    int32_t residual_kernel;                /* TSF_RK_AUTO */
    /* test / tuning hook of the cooperative tail: >= 0 suspends a fit once it has used that many
     * evaluations instead of at the tail of the launch; -1 = the default rule.  Results do not depend
     * on where a fit is suspended. */
    int32_t coop_after;                     /* -1 */
    int32_t converge;                       /* TSF_CONVERGE_STAN */
    int32_t map_max_iter;                   /* 10000: iterations of the continuation (converge = MAP) */
    double map_tol;                         /* 1e-7: its KKT tolerance */
    /* Specified changepoints: see "changepoints at given dates" below. */
    int32_t changepoints_specified;         /* 0 (default): the automatic rule */
    int64_t changepoint_ns[TSF_MAX_S];      /* n_changepoints dates, ns since the epoch, strictly ascending */
} tsf_spec;

/* ---- changepoints at given dates ----------------------------------------------------------------
 * Replaces the `changepoints=[...]` argument of fbprophet's constructor (`Prophet(changepoints=...)`, set_changepoints'
 * `self.specified_changepoints` branch): the trend may change slope at dates the caller knows -- a price change, a
 * migration -- instead of at n_changepoints row timestamps spread over the first changepoint_range of the history.
 * The reference job never passes the argument (prophet_modeler.py:65 uses the default); it is here because users of
 * the model expect it.
 *
 * changepoints_specified = 1: n_changepoints is the number of dates, in [0, TSF_MAX_S], and changepoint_range is
 * ignored, as in fbprophet.  Per grid t_change[j] = (double)(changepoint_ns[j] - start_ns) / (double)t_scale_ns -- the
 * expression that scales a row's timestamp --, S = n_changepoints, and a row belongs to the segments of the dates at or
 * before it; dates may fall between rows.  No dates: the dummy changepoint at t = 0, as for the automatic rule with
 * n_changepoints = 0.  The theta layout does not change.  Every fit, evaluation, prediction, interval and component
 * entry point reads changepoints from the grid alone, so all of them follow.
 *   - A series with a date < min ds or > max ds gets status TSF_ST_CHANGEPOINT: theta is its initial value and no
 *     optimiser runs (as TSF_ST_CAP / TSF_ST_TOO_FEW).  On an aligned panel the one grid decides for every series.  A
 *     date equal to min ds (t_change = 0) or max ds is legal.
 *   - tsf_cross_validate / tsf_tune: fold c of a series fits with the leading dates <= its cutoff -- what fbprophet's
 *     diagnostics.prophet_copy(m, cutoff) keeps --, the deltas of the others are 0; a kept date after the fold's last
 *     history row (irregular timestamps only) makes the fold TSF_ST_CHANGEPOINT and the series TSF_CV_FIT_FAILED.
 *     tsf_tune's candidates must carry base's dates.
 * Deviations, on purpose: dates that are not strictly ascending are API misuse (return < 0 before any launch) where
 * fbprophet sorts them and tolerates duplicates, which give two identical trend columns; TSF_RK_MFMA is rejected
 * with specified dates (its launch plan bounds the changepoint rows per chunk by the automatic spacing).
 * These semantics are restated from recall of fbprophet 0.5; parity with fbprophet itself is unpinned, as everywhere
 * in this library (the tests compare with oracle/fbprophet_restated.py). */

/* What setup derives from one timestamp vector ("grid").  One per call for aligned panels,
 * one per series for ragged panels. */
typedef struct {
    int64_t start_ns;                       /* min ds */
    int64_t t_scale_ns;                     /* max ds - min ds */
    int32_t T;                              /* rows */
    int32_t S;                              /* changepoints actually used */
    int32_t i1;                             /* first row holding max ds */
    int32_t NT;                             /* chunk length ceil(T/64) */
    double t_change[TSF_MAX_S + 4];         /* scaled changepoint times */
} tsf_grid_info;

/* Fit outputs; every pointer caller-allocated (host or device to match the call). */
typedef struct {
    double *theta;          /* [N][tsf_theta_stride(spec)] */
    double *y_scale;        /* [N] */
    double *fval;           /* [N] -log posterior at the returned theta */
    int32_t *status;        /* [N] TSF_ST_* */
    int32_t *n_iter;        /* [N] L-BFGS / Newton iterations */
    int32_t *n_eval;        /* [N] log_prob+gradient evaluations */
    tsf_grid_info *grid;    /* [1] aligned, [N] ragged */
} tsf_fit_out;

typedef struct tsf_ctx tsf_ctx;

int tsf_create(int device_id, tsf_ctx **out);
void tsf_destroy(tsf_ctx *ctx);
const char *tsf_last_error(const tsf_ctx *ctx);
int tsf_device_count(void);

void tsf_spec_default(tsf_spec *spec);
int tsf_spec_size(void);                      /* sizeof(tsf_spec), for binding self-checks */
int tsf_grid_info_size(void);
int tsf_spec_K(const tsf_spec *spec);         /* design columns */
int tsf_theta_stride(const tsf_spec *spec);   /* 3 + n_changepoints + K */

/* ---- fit ------------------------------------------------------------------------------
 * aligned: every series observed on the same T timestamps.  y is [N][T] row-major of
 * y_dtype.  floor / cap: [N] or NULL (NULL = 0; floor is ignored for linear growth exactly
 * as fbprophet ignores the column).  extra: [n_extra][T] or NULL. */
int tsf_fit_aligned(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T,
                    const int64_t *ds, const void *y, int32_t y_dtype, const double *floor,
                    const double *cap, const double *extra, tsf_fit_out *out);
int tsf_fit_aligned_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T,
                        const int64_t *ds, const void *y, int32_t y_dtype,
                        const double *floor, const double *cap, const double *extra,
                        tsf_fit_out *out, void *stream);

/* ragged: series n owns rows [offsets[n], offsets[n+1]) of ds / y / extra
 * (extra: [n_extra][total_rows]). */
int tsf_fit_ragged(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, const int64_t *offsets,
                   const int64_t *ds, const void *y, int32_t y_dtype, const double *floor,
                   const double *cap, const double *extra, tsf_fit_out *out);
int tsf_fit_ragged_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, const int64_t *offsets,
                       int64_t total_rows, int32_t max_T, const int64_t *ds, const void *y,
                       int32_t y_dtype, const double *floor, const double *cap,
                       const double *extra, tsf_fit_out *out, void *stream);

/* ---- predict --------------------------------------------------------------------------
 * yhat[n][h] = trend*(1+multiplicative)+additive in original units (float64).  If
 * yhat_int != NULL also the reference's post-step: (int) truncation toward zero, then
 * values below floor[n] replaced by (int32_t)floor[n] (prophet_scorer.py:73-84).  A truncated
 * value outside int32 saturates to INT32_MIN / INT32_MAX (NaN: INT32_MIN) before the floor
 * clamp; the reference would instead fail the IntegerType cast of its output column there.
 * n_grids = 1 (aligned fit) or N.  ds_future: [H] if shared_future else [N][H].
 * Every grid must satisfy 0 <= S <= min(spec->n_changepoints, TSF_MAX_S) and t_scale_ns > 0,
 * its t_change[0 .. S) ascending: tsf_predict and tsf_predict_intervals reject other grids
 * before any launch; the _dev entries cannot read device-resident grids and require it.
 * extra_future: [n_extra][H] (shared) or [N][n_extra][H]; NULL if n_extra == 0.
 * floor/cap: the values the caller puts in the future frame (prophet_scorer.py:67-68). */
int tsf_predict(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                const int64_t *ds_future, int32_t shared_future, const double *floor,
                const double *cap, const double *extra_future, double *yhat,
                int32_t *yhat_int);
int tsf_predict_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                    const double *theta, const double *y_scale, const tsf_grid_info *grid,
                    int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                    const double *floor, const double *cap, const double *extra_future,
                    double *yhat, int32_t *yhat_int, void *stream);

/* ---- uncertainty intervals ----------------------------------------------------------------
 * yhat_lower / yhat_upper of fbprophet's Prophet.predict_uncertainty -- computed by
 * model.predict(future_df) at /root/reference/src/jobs/prophet_scorer.py:70 and dropped at :86:
 * n_samples simulated futures per series (new trend changepoints ~ Poisson(S (T - 1)) on [1, T] with
 * Laplace(0, mean|delta| + 1e-8) slope changes, observation noise N(0, sigma_obs)), then the
 * (1 -+ interval_width) / 2 percentiles per future row.  fbprophet uses numpy's unseeded global
 * generator; here the draws come from a counter-based generator keyed by (seed, series_key[n],
 * sample, stream), so results are reproducible and independent of how series are batched
 * (series_key NULL: the index of the series in this call).  Also returns the point forecast.
 * Arguments as tsf_predict; n_samples in [2, 4096] (fbprophet: 1000), interval_width in (0, 1)
 * (fbprophet: 0.8). */
int tsf_predict_intervals(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                          const double *theta, const double *y_scale, const tsf_grid_info *grid,
                          int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                          const double *floor, const double *cap, const double *extra_future,
                          const int64_t *series_key, int32_t n_samples, double interval_width,
                          uint64_t seed, double *yhat, double *yhat_lower, double *yhat_upper);
int tsf_predict_intervals_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H,
                              const double *theta, const double *y_scale, const tsf_grid_info *grid,
                              int32_t n_grids, const int64_t *ds_future, int32_t shared_future,
                              const double *floor, const double *cap, const double *extra_future,
                              const int64_t *series_key, int32_t n_samples, double interval_width,
                              uint64_t seed, double *yhat, double *yhat_lower, double *yhat_upper,
                              void *stream);

/* ---- forecast components ------------------------------------------------------------------------
 * The decomposition fbprophet 0.5's Prophet.predict returns beside yhat (predict_trend, predict_seasonal_components,
 * predict_uncertainty): the trend and any set of components -- seasonalities, holidays, regressors, their additive /
 * multiplicative totals -- for a whole panel.  Semantics restated from recall of fbprophet 0.5: parity unpinned (no test
 * compares with the real package; what is pinned is the contract below, against tsf_predict / tsf_predict_intervals).
 * Reference interface replaced: none (the reference keeps yhat alone, prophet_scorer.py:86).
 *
 * Arguments shared with tsf_predict / tsf_predict_intervals mean what they mean there; the same grid check runs first.
 * Component c is a set of design columns: bit j of comp_cols[c] = original column j (the theta layout's beta order:
 * seasonalities in spec order [sin1, cos1, ...], then the extra columns).  comp_scaled[c] = 1 multiplies the component
 * by the series' y_scale (fbprophet does so for additive components; multiplicative ones are relative).  The table
 * (n_comp in [0, TSF_MAX_COMP], every bit below K) is HOST memory in both variants, like spec, and is checked before any
 * launch.
 *
 * Outputs: yhat [N][H], bit-identical to tsf_predict's; trend [N][H] in original units (gtr * y_scale + floor, the value
 * tsf_predict combines with the terms); comp [N][n_comp][H] (NULL if n_comp = 0).
 * Order-of-operations contract: component c is an fma chain over its set columns in ascending original column order
 * starting from 0.0, then multiplied by y_scale if comp_scaled[c]; the design values are the ones tsf_predict uses
 * (the first harmonic from the deterministic sincos, the others by the harmonic recurrence; the caller's extra
 * columns).  So the mask of every additive column with comp_scaled = 1 is tsf_predict's additive term times y_scale,
 * the mask of every multiplicative column (scaled 0) its multiplicative term, and
 *   yhat = trend * (1 + multiplicative_terms) + additive_terms     up to the rounding of that last expression.
 * An empty mask gives 0.0.
 *
 * Intervals: n_samples = 0 computes none (the four interval pointers may be NULL).  Otherwise n_samples in [2, 4096],
 * interval_width in (0, 1) and all four pointers non-NULL: yhat_lower / yhat_upper are tsf_predict_intervals' with the
 * same series_key, seed, width and samples, bit for bit; trend_lower / trend_upper are the same percentiles of the
 * sampled trend of the same draws, before the observation noise (fbprophet's sample_model takes trend and yhat from
 * one trend simulation).  With a MAP fit beta is one point, so a component's own interval is the component itself. */
#define TSF_MAX_COMP 128
int tsf_predict_components(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                           const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                           const int64_t *ds_future, int32_t shared_future, const double *floor, const double *cap,
                           const double *extra_future, int32_t n_comp, const uint64_t *comp_cols,
                           const int32_t *comp_scaled, const int64_t *series_key, int32_t n_samples,
                           double interval_width, uint64_t seed, double *yhat, double *trend, double *comp,
                           double *yhat_lower, double *yhat_upper, double *trend_lower, double *trend_upper);
int tsf_predict_components_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                               const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                               const int64_t *ds_future, int32_t shared_future, const double *floor,
                               const double *cap, const double *extra_future, int32_t n_comp,
                               const uint64_t *comp_cols, const int32_t *comp_scaled, const int64_t *series_key,
                               int32_t n_samples, double interval_width, uint64_t seed, double *yhat, double *trend,
                               double *comp, double *yhat_lower, double *yhat_upper, double *trend_lower,
                               double *trend_upper, void *stream);

/* ---- forecast quantiles, cumulative quantiles, predictive samples ----------------------------------
 * The predictive distribution behind tsf_predict_intervals' one symmetric pair: any set of quantiles of the sampled yhat
 * per future row, the same quantiles of each sample's running sum over the future rows ("P90 of the total of the next 14
 * days": quantiles of sums are not sums of quantiles), the quantiles of the sampled trend, and the raw draws themselves
 * (fbprophet 0.5's Prophet.predictive_samples: {'yhat', 'trend'}, each (H, n_samples) per series).  Semantics restated
 * from recall of fbprophet 0.5: parity unpinned (no test compares with the real package; what is pinned is the contract
 * below, against tsf_predict / tsf_predict_intervals / tsf_predict_components).
 * Reference interface replaced: none (the reference keeps yhat alone, prophet_scorer.py:86).
 *
 * Arguments shared with tsf_predict_intervals mean what they mean there; the same grid check runs first.  n_samples in
 * [2, 4096].  quantiles [n_q] and the tsf_quantile_out struct are HOST memory in both variants, like spec; the pointers
 * inside the struct are host pointers in the host variant and device pointers in _dev.  n_q in [0, TSF_MAX_QUANT], every
 * level finite and in [0, 1] (0: the minimum, 1: the maximum); their order and duplicates are the caller's business.
 * n_q = 0 is legal only where a sample output is wanted; a call that wants none of q / cum_q / trend_q / samples /
 * trend_samples is refused.  Every refusal returns < 0 with a message, before any launch; the context stays usable.
 *
 * Contract:
 *   The draws are tsf_predict_intervals' draws: the same generator, keys (seed, series_key[n], sample, stream) and
 *   counters.  Sample s of a series depends neither on n_samples, nor on the batch, nor on which outputs are requested.
 *   A quantile at level p is taken over the ascending sorted values v[0 .. n_samples): with
 *     pos = p * (double)(n_samples - 1), lo = floor(pos), hi = min(lo + 1, n_samples - 1)
 *   it is v[lo] + (v[hi] - v[lo]) * (pos - lo), the expression and rounding of tsf_predict_intervals.  So the levels
 *   (1 - w) / 2 and (1 + w) / 2, formed in double exactly so, give tsf_predict_intervals' yhat_lower / yhat_upper at
 *   width w bit for bit, and trend_q gives tsf_predict_components' trend_lower / trend_upper the same way.
 *   The running sum of sample s is c[s][0] = sample[s][0], c[s][h] = c[s][h-1] + sample[s][h]: plain double adds in the
 *   row order the caller gave (it does not restart where unsorted futures restart the trend sweep).  cum_q[n][i][h] is
 *   the quantile of c[.][h]; cum_q[n][i][0] == q[n][i][0] bit for bit.
 *   No int truncation or floor clamp is applied (tsf_predict_intervals applies none either).
 *
 * Scratch: series are processed in chunks whose sample buffers (yhat; the running sums if cum_q; the trend if trend_q or
 * trend_samples) stay within 512 MB; results do not depend on the chunking.  Requested raw samples are copied out of the
 * scratch chunk by chunk in stream order: the host variant never holds N * H * n_samples values on the device. */
#define TSF_MAX_QUANT 64
typedef struct {
    double *yhat;           /* [N][H]        required: tsf_predict's, bit for bit */
    double *q;              /* [N][n_q][H]   per-row quantiles of the sampled yhat; NULL: not wanted */
    double *cum_q;          /* [N][n_q][H]   quantiles of each sample's running sum over rows 0..h; NULL: not wanted */
    double *trend_q;        /* [N][n_q][H]   per-row quantiles of the sampled trend (before noise); NULL: not wanted */
    double *samples;        /* [N][H][n_samples] raw yhat draws, sample s at index s; NULL: not wanted */
    double *trend_samples;  /* [N][H][n_samples] raw trend draws; NULL: not wanted */
} tsf_quantile_out;
int tsf_predict_quantiles(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                          const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                          const int64_t *ds_future, int32_t shared_future, const double *floor, const double *cap,
                          const double *extra_future, const int64_t *series_key, int32_t n_samples, uint64_t seed,
                          int32_t n_q, const double *quantiles, tsf_quantile_out *out);
int tsf_predict_quantiles_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                              const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                              const int64_t *ds_future, int32_t shared_future, const double *floor,
                              const double *cap, const double *extra_future, const int64_t *series_key,
                              int32_t n_samples, uint64_t seed, int32_t n_q, const double *quantiles,
                              tsf_quantile_out *out, void *stream);

/* ---- scoring observed values against the predictive distribution (PIT, CRPS, pinball) ----------------
 * The other half of tsf_predict_quantiles: given fitted models and the values observed on the forecast rows, how good
 * is the predictive distribution, and how surprising is each observation under it?  Per row, from the same draws and
 * the same single sort per row: the probability integral transform (PIT: uniform on [0, 1] over many rows where the
 * distribution is calibrated; a value in a far tail flags an anomaly), the sample CRPS (a proper score in the units of
 * y: lower is better), the quantiles at any set of levels and their pinball losses.  Per series: the means over the
 * observed rows, the empirical coverage of every level (the share of observed rows with y <= q: near the level where
 * the quantile is calibrated) and the row count.  Only [N][H]-sized answers leave the device; doing the same from
 * tsf_predict_quantiles' raw samples needs N * H * n_samples values on the host.
 * Reference interface replaced: none (neither the reference nor fbprophet has such a function); parity unpinned (what
 * is pinned is the contract below, against tsf_predict_quantiles' draws and quantiles).
 * Timing: tools/bench_scores.py; DESIGN.md 5g.
 *
 * Arguments shared with tsf_predict_quantiles mean what they mean there; the same grid check runs first, then its
 * checks of n_samples ([2, 4096]), n_q ([0, TSF_MAX_QUANT]) and the levels.  quantiles [n_q] and the tsf_score_out
 * struct are HOST memory in both variants; y_obs and the pointers inside the struct are host pointers in the host
 * variant and device pointers in _dev.  y_obs [N][H]: the observed value of every forecast row, NaN = not observed.
 *
 * Contract:
 *   The draws are tsf_predict_quantiles' draws (same generator, keys and counters); v[0 .. n_samples) below is a row's
 *   draws sorted ascending and y its observed value.
 *   q[n][i][h] is tsf_predict_quantiles' expression at level p = quantiles[i] (same pos, lo, hi, same three
 *   roundings): bit for bit its q.  pinball[n][i][h]: with e = y - q, e >= 0 ? p * e : (p - 1.0) * e.
 *   pit = ((double)lt + 0.5 * (double)eq) / (double)n_samples, lt = #{v < y}, eq = #{v == y} (exact counts): the
 *   mid-distribution transform, in steps of 0.5 / n_samples; 0 below every draw, 1 above every draw.
 *   crps is the sample CRPS mean_i |v[i] - y| - (1/2) mean_{i,j} |v[i] - v[j]|, regrouped over the sorted row into
 *   non-negative terms so that nothing cancels:
 *     d = v[i] - y;  w = (double)(2 * i - (n_samples - 1)) / (double)n_samples;  c[i] = fabs(d) - w * d
 *   (plain operations: multiply, round, subtract; |w| < 1 so c[i] >= 0), c[i] = +0.0 for n_samples <= i < NSP (NSP:
 *   n_samples rounded up to a power of two, at least 2), then the fixed tree
 *     for (s = NSP / 2; s >= 1; s /= 2) c[i] = c[i] + c[i + s] for every i < s
 *   and crps = c[0] / (double)n_samples.  With the exact value x of the sample CRPS of the same draws,
 *     |crps - x| <= 2^-53 * (4 * mean_i |v[i] - y| + (log2(NSP) + 2) * x).
 *   A row whose y is NaN gets NaN in pit, crps and pinball; its q is still written.
 *   Per series, over its rows in the caller's row order with plain double adds from +0.0: n_obs = the number of rows
 *   with a non-NaN y; mean_crps and mean_pinball[n][i] = the sum over the observed rows / (double)n_obs;
 *   coverage[n][i] = (double)#{observed rows with y <= q[n][i][h]} / (double)n_obs.  n_obs = 0: NaN means and coverage.
 *   No floating-point atomics.  Every output depends neither on how the call is cut into scratch chunks (512 MB, one
 *   sample buffer), nor on what else is in the batch, nor on which other outputs are requested.  Per-row arrays the
 *   requested aggregates need and the caller did not ask for live in the context's scratch.
 *   Behaviour for non-finite draws is unspecified (as for the quantiles).
 *
 * Refusals (< 0 with a message, before any launch; the context stays usable): a NULL out, out->yhat or y_obs;
 * n_samples outside [2, 4096]; a bad n_q or level; n_q = 0 with q, pinball, mean_pinball or coverage requested; a call
 * that wants nothing beyond yhat; in the host variant an infinite y_obs value (the _dev variant cannot look: there it
 * is the caller's business).  N == 0 is a legal no-op.
 *
 * Totals over several rows (running totals, weeks, months) and roll-ups are scored by tsf_predict_windows and
 * tsf_rollup_windows ("totals over row windows", below).
 * Out of scope: a split over several GPUs (the call is per context, like tsf_predict_quantiles). */
typedef struct {
    double *yhat;           /* [N][H]        required: tsf_predict's, bit for bit */
    double *pit;            /* [N][H]        NULL: not wanted (all below likewise) */
    double *crps;           /* [N][H] */
    double *q;              /* [N][n_q][H]   tsf_predict_quantiles' q, bit for bit */
    double *pinball;        /* [N][n_q][H] */
    int32_t *n_obs;         /* [N] */
    double *mean_crps;      /* [N] */
    double *mean_pinball;   /* [N][n_q] */
    double *coverage;       /* [N][n_q] */
} tsf_score_out;
int tsf_score_out_size(void);       /* sizeof(tsf_score_out): the self-check of a binding */
int tsf_score_actuals(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                      const double *y_scale, const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future,
                      int32_t shared_future, const double *floor, const double *cap, const double *extra_future,
                      const int64_t *series_key, int32_t n_samples, uint64_t seed,
                      const double *y_obs /* [N][H], NaN = not observed */, int32_t n_q, const double *quantiles,
                      tsf_score_out *out);
int tsf_score_actuals_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                          const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                          const int64_t *ds_future, int32_t shared_future, const double *floor, const double *cap,
                          const double *extra_future, const int64_t *series_key, int32_t n_samples, uint64_t seed,
                          const double *y_obs, int32_t n_q, const double *quantiles, tsf_score_out *out, void *stream);

/* ---- group roll-ups: predictive quantiles of sums over series ---------------------------------------
 * The predictive distribution of a TOTAL over several series -- P90 of a series_id over its dim_ids, of a region, of the
 * whole panel -- and of its running sum over the future rows.  The point forecast of a total is a sum of yhat columns;
 * its quantiles are not sums of quantiles, so the draws of the members are summed sample by sample on the device and
 * the sums are sorted.  A group's members need not share a tsf_spec nor fit one call, so a roll-up is an accumulator
 * that lives across calls: create, add (once per spec, as often as needed), read quantiles (any time), free.
 * Reference interface replaced: none (neither the reference nor fbprophet has such a function); parity unpinned (what is
 * pinned is the contract below, against tsf_predict_quantiles' draws).  Host pointers only, like tsf_cross_validate.
 * Timing: tools/bench_rollup.py; the first MI355X run is in DESIGN.md 5f.
 *
 * Meaning: by default the members are taken as independent given their fits (each series is fitted alone and draws
 * from its own stream); where the members' errors are positively correlated in reality, such a roll-up's spread is too
 * narrow.  The remedy is opt-in: tsf_residual_corr estimates each group's residual correlation from the fits' own history
 * and tsf_rollup_set_noise_corr makes the adds draw the members' observation noise with it ("correlated group roll-ups"
 * below, with its limits).  A handle without a correlation set is what it always was, bit for bit.
 *
 * Rows: every member is forecast on the roll-up's own ds_future[H], one shared calendar; row h of a group is the sum
 * over its members at row index h.  extra_future is [n_extra][H] with shared_extra set, else [N][n_extra][H].  A
 * member's forecast is tsf_predict's with shared_future = 1 where the spec has no extra column or shared_extra is
 * set, and with shared_future = 0 and the calendar repeated per series otherwise.
 *
 * Draws: tsf_predict_quantiles' draws for the same (seed, series_key[n], sample); sample s of a member depends on
 * nothing else.  series_key is required: the "index in this call" default would give series 0 of two add calls the
 * same stream and a perfectly correlated sum.  Keys that are distinct across calls are the caller's business.
 *
 * Accumulation: acc[g][h][s] ([G][H][n_samples]), ysum[g][h] and count[g] belong to the handle and start at +0.0 / 0.
 * An add performs acc = acc + sample and ysum = ysum + yhat (tsf_predict's float64 value: no int truncation, no floor
 * clamp), plain double adds, the members of a group one at a time in ascending order of their index in that call; add
 * calls apply in call order.  The result depends neither on how a call is cut into scratch chunks (512 MB, one sample
 * buffer) nor on what else the call contains.  No floating-point atomics.
 *
 * Quantiles: q[g][i][h] is tsf_predict_quantiles' expression (same pos / lo / hi, same rounding) over the ascending
 * sort of acc[g][h][0 .. n_samples); cum_q[g][i][h] the same over c[g][h][s], c[g][0][s] = acc[g][0][s],
 * c[g][h][s] = c[g][h-1][s] + acc[g][h][s], so cum_q[.][.][0] == q[.][.][0] bit for bit.  tsf_rollup_quantiles does
 * not modify the accumulators: it may be called repeatedly and between adds.  A group nobody was added to has count 0
 * and 0.0 everywhere.  n_q and the levels as in tsf_predict_quantiles; n_q = 0 is legal only with samples.
 *
 * Refusals (< 0 with a message in the context's tsf_last_error, before any launch; the accumulators are untouched and
 * the context stays usable) -- create: G < 1, H < 1, n_samples outside [2, 4096], NULL ds_future; add: a group value
 * outside [0, G), NULL series_key, tsf_predict's grid checks, n_extra > 0 with NULL extra_future, logistic growth
 * without cap, n_grids not 1 or N; quantiles: a bad n_q or level, an output set that wants none of q / cum_q / samples.
 * N == 0 is a legal no-op.  A failed device allocation in create returns < 0 and leaves nothing behind.  A HIP failure
 * in the middle of an add (or of tsf_rollup_set_totals, below) poisons the handle: every later call on it returns < 0. */
typedef struct tsf_rollup tsf_rollup;
int tsf_rollup_create(tsf_ctx *ctx, int64_t G, int32_t H, const int64_t *ds_future /* [H] */, int32_t n_samples,
                      uint64_t seed, tsf_rollup **out);
int tsf_rollup_add(tsf_rollup *r, const tsf_spec *spec, int64_t N, const double *theta, const double *y_scale,
                   const tsf_grid_info *grid, int32_t n_grids, const double *floor, const double *cap,
                   const double *extra_future, int32_t shared_extra, const int64_t *series_key /* [N], required */,
                   const int64_t *group /* [N], each in [0, G) */);
typedef struct {
    double *yhat;           /* [G][H]        required: the sum of the members' yhat */
    int64_t *count;         /* [G]           members added so far; NULL: not wanted */
    double *q;              /* [G][n_q][H]   per-row quantiles of the summed draws; NULL: not wanted */
    double *cum_q;          /* [G][n_q][H]   quantiles of each summed sample's running sum over rows 0..h; NULL: not wanted */
    double *samples;        /* [G][H][n_samples] the summed draws themselves; NULL: not wanted */
} tsf_rollup_out;
int tsf_rollup_quantiles(tsf_rollup *r, int32_t n_q, const double *quantiles, tsf_rollup_out *out);
void tsf_rollup_free(tsf_rollup *r);        /* before tsf_destroy of its context */

/* ---- reconciliation: member forecasts and directly fitted totals made coherent -----------------------
 * A roll-up's total is bottom-up: the sum of its members' draws.  Whoever forecasts such a hierarchy usually fits the
 * total directly as well (the sum of twenty noisy histories has a far better signal than any one of them), and then the
 * direct forecast of the total and the sum of the member forecasts disagree, and the members do not use what the total
 * knows.  Reconciliation projects the incoherent pair (total, members) onto the coherent subspace by weighted least
 * squares, sample by sample, so that the reconciled quantiles are quantiles of coherent draws -- on the device, where
 * the draws already are (doing it by hand moves N * H * n_samples * 8 bytes to the host).
 * Reference interface replaced: none (neither the reference nor fbprophet has such a function: none of this is
 * Prophet's); parity unpinned (what is pinned is the contract below, against tsf_predict_quantiles' draws and
 * tsf_rollup_quantiles' accumulators).  Host pointers only, like tsf_rollup_*.
 * Timing: tools/bench_reconcile.py; DESIGN.md 5j.
 *
 * Method (two-level hierarchy, diagonal weights: the MinT / WLS solution with a diagonal covariance, applied to joint
 * samples).  Group g has members i with draws x_i[h][s] and one directly fitted total with draws t_g[h][s]; w_i > 0 and
 * v_g > 0 are the caller's estimates of the forecast error variance of each base forecast; W_g = sum of w_i over the
 * group.  Minimising (t - sum b_i)^2 / v + sum (x_i - b_i)^2 / w_i gives, with d_g[h][s] = t_g[h][s] - acc[g][h][s]
 * (the incoherence of sample s; acc is the roll-up's sum of member draws),
 *   lambda_i = w_i / (v_g + W_g),  mu_g = W_g / (v_g + W_g),
 *   reconciled member x_i + lambda_i * d_g,  reconciled total acc_g + mu_g * d_g.
 * sum_i lambda_i = mu_g, so the reconciled members sum to the reconciled total (to rounding).  The total's stream and
 * the members' streams are independent, so where the weights equal the true variances the reconciled member has variance
 * w_i - w_i^2 / (v_g + W_g): never wider than before.  The independence caveat of the roll-ups applies unchanged:
 * members (and the total) are taken as independent given their fits; where their errors are positively correlated in
 * reality, the spreads are too narrow.
 *
 * tsf_reconcile_shares (host only: no context, no device) turns weights into shares.  group [N] in [0, G); w [N] (NULL:
 * all 1.0); v [G] (NaN: the group has no total).  W_g is summed from +0.0 in ascending member index by plain double
 * adds; share[i] = w_i / (v_g + W_g) and share_total[g] = W_g / (v_g + W_g), each one add and one divide.  A group whose
 * v is NaN, or which has no member, gets +0.0 in both.  Returns -1 for a group value outside [0, G) and for a weight
 * or v that is not finite and positive (NaN v excepted).  Weight policies ('ols': all 1; 'struct': members 1, the total
 * its member count; residual variances; cross-validation mse) are the caller's, on top of this.
 *
 * tsf_rollup_set_totals forecasts Gt directly fitted total series on the roll-up's calendar exactly as tsf_rollup_add
 * forecasts members (same arguments, checks, refusals and draws: (seed, series_key[n], sample)) and adds them to a second
 * accumulator: top[G][H][n_samples] = +0.0 + draw, ytop[G][H] = +0.0 + yhat, series n into group[n].  The two buffers
 * are allocated by the first call and not before: a roll-up that never reconciles costs what it did.  It may be called
 * once per spec bucket; a group that has a total already, or that appears twice in one call, is refused before any
 * launch.  Keys distinct from each other and from the members' keys are the caller's business: a total that shares a
 * key with a member shares its stream, and the independence above is gone.  A HIP failure in the middle poisons the
 * handle, as for add.
 *
 * tsf_rollup_reconcile is the second pass over the members: called after every add and set_totals, with the same
 * members, keys (and the handle's seed and n_samples), so the draws are the ones that were added.  Arguments as in
 * tsf_rollup_add, then share [N] (finite, in [0, 1]), the levels as in tsf_predict_quantiles and the outputs.
 * Contract, in plain double operations (no fused multiply-add):
 *   d = top[g][h][s] - acc[g][h][s] where group g has a total, +0.0 where it has none;
 *   sample' = sample + share[n] * d                         (a subtract, a multiply, an add)
 *   yhat'   = yhat + share[n] * (ytop[g][h] - ysum[g][h])   (the same three; +0.0 in place of the difference without a total)
 *   q is tsf_predict_quantiles' expression over the ascending sort of sample'; cum_q the same over the running sums
 *   c[0] = sample'[0], c[h] = c[h-1] + sample'[h] along the rows.
 * So share = 0 everywhere gives tsf_predict_quantiles' yhat, q, cum_q and samples bit for bit (for every value the
 * draws produce: -0.0 would become +0.0), and a group without a total leaves its members untouched.  The call modifies
 * neither accumulator, may be repeated, and poisons nothing.  The result depends neither on how the call is cut into
 * scratch chunks (512 MB; one sample buffer, two with cum_q) nor on what else is in the call, nor on which outputs are
 * requested.  No floating-point atomics.  Members that were not added (or other keys) are not detected: d is then not
 * their incoherence, and that is the caller's business.
 *
 * tsf_rollup_reconciled_totals reads the totals: per cell acc + share_total[g] * (top - acc) (the same three operations,
 * +0.0 for the difference without a total), yhat the same from ysum and ytop; the outputs are tsf_rollup_quantiles'
 * outputs over that quantity (count: the members added).  share_total [G], finite and in [0, 1].  Groups are processed
 * in ranges through the context's scratch; neither accumulator is modified.
 *
 * Refusals (< 0 with a message, before any launch; the accumulators are untouched and the handle and the context stay
 * usable): tsf_rollup_add's for set_totals and reconcile; a second total for a group; reconcile or reconciled_totals
 * before any set_totals (not silent zeros); a share outside [0, 1] or NaN; a bad n_q or level; an output set that
 * wants none of q / cum_q / samples.  N == 0 (Gt == 0) is a legal no-op.
 *
 * Hierarchies deeper than two levels: "tree reconciliation", below.
 * Out of scope: non-diagonal covariance (MinT-shrink); per-row weights; the job
 * configuration of the modeler and the scorer; _dev variants; more than one GPU. */
int tsf_reconcile_shares(int64_t N, const int64_t *group, const double *w /* [N], NULL = all 1.0 */, int64_t G,
                         const double *v /* [G]; NaN = the group has no total */, double *share /* [N] lambda */,
                         double *share_total /* [G] mu */);
int tsf_rollup_set_totals(tsf_rollup *r, const tsf_spec *spec, int64_t Gt, const double *theta, const double *y_scale,
                          const tsf_grid_info *grid, int32_t n_grids, const double *floor, const double *cap,
                          const double *extra_future, int32_t shared_extra, const int64_t *series_key /* [Gt], required */,
                          const int64_t *group /* [Gt], the group each total series belongs to */);
typedef struct {
    double *yhat;           /* [N][H]        required: the reconciled point forecast */
    double *q;              /* [N][n_q][H]   per-row quantiles of the reconciled draws; NULL: not wanted */
    double *cum_q;          /* [N][n_q][H]   quantiles of each reconciled sample's running sum over rows 0..h; NULL: not wanted */
    double *samples;        /* [N][H][n_samples] the reconciled draws themselves; NULL: not wanted */
} tsf_reconcile_out;
int tsf_reconcile_out_size(void);   /* sizeof(tsf_reconcile_out): the self-check of a binding */
int tsf_rollup_reconcile(tsf_rollup *r, const tsf_spec *spec, int64_t N, const double *theta, const double *y_scale,
                         const tsf_grid_info *grid, int32_t n_grids, const double *floor, const double *cap,
                         const double *extra_future, int32_t shared_extra, const int64_t *series_key /* [N], required */,
                         const int64_t *group /* [N] */, const double *share /* [N] */, int32_t n_q,
                         const double *quantiles, tsf_reconcile_out *out);
int tsf_rollup_reconciled_totals(tsf_rollup *r, const double *share_total /* [G] */, int32_t n_q, const double *quantiles,
                                 tsf_rollup_out *out);

/* ---- tree reconciliation: hierarchies deeper than two levels ---------------------------------------------
 * The reconciliation above stops at members and one total per group.  Real hierarchies go on: (series, dim) -> series
 * -> region -> everything, each level with directly fitted totals of its own.  For a tree with diagonal weights the
 * weighted least squares projection onto the coherent subspace is one sweep up and one sweep down over the sample
 * buffers the roll-up already holds -- streaming kernels, nothing dense, nothing through the host.
 * Reference interface replaced: none (none of this is Prophet's); parity unpinned (what is pinned is the contract
 * below, against tsf_predict_quantiles' draws and the roll-up's accumulators).  Host pointers only, like tsf_rollup_*.
 * Timing: tools/bench_tree.py; DESIGN.md 5p.
 *
 * Levels.  Level 0: the members.  Level 1: the roll-up's G groups.  Levels 2 .. L (L - 1 = n_upper <=
 * TSF_TREE_MAX_LEVELS): n_nodes[k] nodes at level k + 2; every node below the top level has one parent in the level
 * above; the top level may hold several nodes (a forest).  Arrays "over the nodes" are flat, level 1 first:
 * [G + n_nodes[0] + ... + n_nodes[n_upper - 1]] = [M].  `parent` is flat over the nodes below the top: parent[g] of
 * group g in [0, n_nodes[0]), then the parents of the level-2 nodes in [0, n_nodes[1]), and so on: [M - n_nodes[n_upper - 1]].
 *
 * Problem.  Members have variances w_i; a node n of level >= 1 may have a directly fitted total t_n with variance v_n.
 * Minimise sum_i (x_i - b_i)^2 / w_i + sum_n (t_n - c_n)^2 / v_n, c_n the sum of the b_i below node n.
 *
 * tsf_reconcile_tree_shares (host only: no context, no device).  group [N] in [0, G); w [N] (NULL: all 1.0); v [M]
 * (NaN: the node has no total).  In plain double operations, every sum from +0.0 in ascending index:
 *   level 1:  E_g = W_g = sum of w_i over the group;  share[i] = w_i / W_g
 *   any level, v_n not NaN and E_n > 0:  mu_n = E_n / (v_n + E_n),  e_n = (E_n * v_n) / (v_n + E_n)
 *   otherwise:                           mu_n = +0.0,               e_n = E_n
 *   the level above:  E_p = sum of e_c over the children c of p;  kappa_c = e_c / E_p, +0.0 where E_p == 0
 *   the top level:    kappa = +0.0 (it has no parent)
 * e_n is the variance left in node n after its own total and everything below it are blended in; kappa_c is child c's
 * share of what its parent moves by.  A node with no member below it has E = 0, so mu = e = kappa = +0.0, and a total
 * given for it is ignored (as tsf_reconcile_shares treats a group without members).  Returns -1 for a group or parent
 * out of range, a weight or v that is not finite and positive (NaN v excepted), n_upper outside
 * [0, TSF_TREE_MAX_LEVELS], n_nodes < 1, G < 1.  Weight policies are the caller's, on top of this.
 *
 * tsf_rollup_set_tree declares levels 2 .. L above the handle's groups (n_upper >= 1) and allocates what the solve
 * keeps: per group cell one double (delta), per node cell of an upper level two (the bottom-up sum A and c).  A roll-up
 * that never calls it costs what it did.  Refused: a second call; a handle with a noise correlation; a parent out of
 * range; n_nodes[k] * H or G * H >= 2^31.
 *
 * tsf_rollup_set_node_totals forecasts the directly fitted totals of nodes of one level in [2, L] exactly as
 * tsf_rollup_set_totals does for level 1 (which stays the entry for level 1): tsf_rollup_add's arguments, checks and
 * draws ((seed, series_key[n], sample)), series n into node[n] of that level; t = +0.0 + draw, yt = +0.0 + yhat.  The
 * level's buffer is allocated by the first call for it.  At most one total per node over all calls; a node that
 * appears twice in one call is refused before any launch.  Keys distinct from every other key of the hierarchy are the
 * caller's business.  A HIP failure in the middle poisons the handle, as for add.
 *
 * tsf_rollup_solve_tree runs the two sweeps with mu [M] and kappa [M] (each finite and in [0, 1]).  Per cell
 * (node, row, sample), in plain double operations (no fused multiply-add), one writer per cell, no atomics:
 *   up, level 1:   A = acc
 *   up, above:     A_p = sum of m_c over the children c of p, from +0.0 in ascending child index
 *   every level:   m_n = A_n + mu_n * (t_n - A_n) where node n was given a total (set_totals / set_node_totals),
 *                  m_n = A_n where it was not (whatever mu_n says)
 *   down, top:     c_n = m_n
 *   down, below:   c_n = m_n + kappa_n * (c_p - A_p), p the parent of n
 *   kept:          delta_g = c_g - acc_g per group cell; c_n per cell of the levels above
 * The point forecast goes through the same recursion on ysum / ytop / the node totals' yhat.  Neither accumulator is
 * modified.  A later tsf_rollup_add, tsf_rollup_set_totals or tsf_rollup_set_node_totals invalidates the solve: the two
 * reads below are refused until it has run again.  It may be repeated with other shares.
 *
 * tsf_rollup_reconcile_tree is the members' second pass: tsf_rollup_reconcile's arguments, rules and outputs with
 *   sample' = sample + share[n] * delta[g][h][s],  yhat' = yhat + share[n] * ydelta[g][h]    (a multiply, an add)
 * and share [N] from tsf_reconcile_tree_shares.  The draws are the ones that were added (same keys, the handle's seed);
 * the result depends neither on the scratch chunks nor on what else is in the call nor on the outputs requested.
 * Without any total anywhere every delta is +0.0 and the call returns tsf_predict_quantiles' outputs bit for bit.
 * With one upper level and no upper totals the solution is the two-level one above in exact arithmetic, not in bits
 * (that one multiplies w_i / (v + W) by (t - acc) in one step).
 *
 * tsf_rollup_tree_totals reads the reconciled nodes node0 .. node0 + n_nodes of one level in [1, L]: at level 1 the
 * cells acc + delta (one add), above it c itself; yhat the same from the point forecasts; the outputs are
 * tsf_rollup_quantiles' outputs over those cells, sized by n_nodes (count: the members added below each node).  Nodes
 * are processed in ranges through the context's scratch; nothing the handle holds is modified.
 *
 * Refusals (< 0 with a message, before any launch; the handle and the context stay usable): any of these before
 * set_tree (shares excepted); a level outside its range; a node out of range or given a total twice; reconcile_tree or
 * tree_totals before solve_tree or after a later add / set_totals / set_node_totals; a share, mu or kappa outside
 * [0, 1] or NaN; tsf_rollup_add's refusals for set_node_totals and reconcile_tree; a bad n_q or level of a quantile; an
 * output set that wants none of q / cum_q / samples; every entry on a handle with a noise correlation.  N == 0,
 * Gt == 0 and n_nodes == 0 are legal no-ops.
 *
 * Limits: diagonal weights (no MinT-shrink); one weight per node, not per row; roll-ups with a noise correlation are
 * not reconciled; one calendar, as with any roll-up; windows of the reconciled draws, the job configuration of the
 * modeler and the scorer, _dev variants and more than one GPU are out of scope. */
#define TSF_TREE_MAX_LEVELS 4
int tsf_reconcile_tree_shares(int64_t N, const int64_t *group, const double *w /* [N], NULL = all 1.0 */, int64_t G,
                              int32_t n_upper, const int64_t *n_nodes /* [n_upper] */, const int64_t *parent,
                              const double *v /* [M]; NaN = the node has no total */, double *share /* [N] */,
                              double *mu /* [M] */, double *e /* [M] */, double *kappa /* [M] */);
int tsf_rollup_set_tree(tsf_rollup *r, int32_t n_upper, const int64_t *n_nodes /* [n_upper] */, const int64_t *parent);
int tsf_rollup_set_node_totals(tsf_rollup *r, int32_t level, const tsf_spec *spec, int64_t Gt, const double *theta,
                               const double *y_scale, const tsf_grid_info *grid, int32_t n_grids, const double *floor,
                               const double *cap, const double *extra_future, int32_t shared_extra,
                               const int64_t *series_key /* [Gt], required */,
                               const int64_t *node /* [Gt], the node of `level` each total series belongs to */);
int tsf_rollup_solve_tree(tsf_rollup *r, const double *mu /* [M] */, const double *kappa /* [M] */);
int tsf_rollup_reconcile_tree(tsf_rollup *r, const tsf_spec *spec, int64_t N, const double *theta, const double *y_scale,
                              const tsf_grid_info *grid, int32_t n_grids, const double *floor, const double *cap,
                              const double *extra_future, int32_t shared_extra, const int64_t *series_key /* [N], required */,
                              const int64_t *group /* [N] */, const double *share /* [N] */, int32_t n_q,
                              const double *quantiles, tsf_reconcile_out *out);
int tsf_rollup_tree_totals(tsf_rollup *r, int32_t level, int64_t node0, int64_t n_nodes, int32_t n_q,
                           const double *quantiles, tsf_rollup_out *out);

/* ---- temporal reconciliation: daily forecasts and directly fitted period totals made coherent ---------------
 * The reconciliations above work across series.  This one works along time, inside one series: the H rows of a forecast
 * are the members, the forecast of a second model fitted on the period totals of the same history (its weekly or monthly
 * sums) is the total, and each row window [win_start[k], win_end[k]) is a group.  The sum of seven noisy days has a
 * better signal than any one of them, so the period model sees level and yearly pattern better; the daily model alone
 * knows the pattern inside the period.  Without this a caller who fits both has two answers for "next week's total".
 * The method is "reconciliation"'s projection (weighted least squares, diagonal weights, two levels), applied to each
 * sample's path on the device: the reconciled rows of a window sum to the reconciled period total, and the quantiles of
 * both are quantiles of coherent draws.
 * Reference interface replaced: none (neither the reference nor fbprophet has such a function); parity unpinned (what is
 * pinned is the contract below, against tsf_predict, tsf_predict_quantiles and tsf_predict_windows).  Host pointers only.
 * Timing: tools/bench_temporal.py; DESIGN.md 5q.
 *
 * tsf_temporal_shares (host only: no context, no device) is tsf_reconcile_shares' rule per window.  w [N][H] (NULL: all
 * 1.0) and v [N][K] are the caller's estimates of the error variance of every row's forecast and of every period
 * forecast; a NaN v marks a window that is not reconciled for that series.  Per series and window
 *   W = the sum of w[n][h] over the window's rows, from +0.0 by plain double adds in ascending row order,
 *   share[n][h] = w[n][h] / (v[n][k] + W),   share_total[n][k] = W / (v[n][k] + W)       (each one add and one divide).
 * A window with a NaN v gets +0.0 in its share cells and NaN in share_total; a row in no window gets share +0.0.
 * Returns -1 for K outside [1, TSF_MAX_WINDOWS], a window that is not 0 <= win_start < win_end <= H, two windows that
 * share a row, and a w or v that is not finite and positive (NaN v excepted).
 *
 * tsf_predict_temporal.  The first block of arguments is the daily model and means what it means in
 * tsf_predict_quantiles; the second block is the period model on its K rows ds_period (one row per window, in the order
 * of the windows), with a spec, grids, floor, cap, extra columns and keys of its own.  noise_ar, noise_ar_p [N]: each
 * model's AR(1) coefficients, phi in [0, 1), or NULL for independent noise.  They are arguments of this call: a pending
 * tsf_set_noise_ar setting is neither taken nor cleared.  share [N][H] and share_total [N][K] as tsf_temporal_shares
 * writes them.  The tsf_temporal_out struct, the levels, the windows and the shares are host memory.
 *
 * Contract, in plain double operations (no fused multiply-add).  x[h][s] are the daily draws: tsf_predict_quantiles'
 * samples for (spec, series_key[n], seed, n_samples) with tsf_set_noise_ar(noise_ar) where it is given; t[k][s] are the
 * period model's draws, the same statement for (spec_p, period_key[n], noise_ar_p) on the K rows ds_period; y and yp are
 * tsf_predict's point forecasts of the two models.  Window k = [a, b) is active for series n where share_total[n][k] is
 * not NaN.
 *   sum      = x[a][s];  sum = sum + x[h][s] for h = a + 1 .. b - 1           (tsf_predict_windows' window sum)
 *   d        = t[k][s] - sum where the window is active, +0.0 where it is not
 *   x'[h][s] = x[h][s] + share[n][h] * d        for the rows of the window; a row in no window is left as it is
 *   win'[k][s] = sum + share_total[n][k] * d    (the NaN of an inactive window read as +0.0: win' = sum)
 *   ysum = y[a]; ysum = ysum + y[h] ...;  dy = yp[k] - ysum (+0.0 where inactive)
 *   yhat'[h] = y[h] + share[n][h] * dy,   total[k] = ysum + share_total[n][k] * dy
 *   q is tsf_predict_quantiles' expression over the ascending sort of x'[h][.]; cum_q the same over the running sums
 *   c[0] = x'[0], c[h] = c[h-1] + x'[h]; win_q the same over win'[k][.].
 * So with every share +0.0 and every share_total +0.0 or NaN, yhat, q, cum_q and samples are tsf_predict_quantiles' bit
 * for bit and total and win_q are tsf_predict_windows' (for every value the draws produce: -0.0 would become +0.0).
 * The sum of share[n][h] over a window equals share_total[n][k] (to rounding), so the reconciled rows of an active window
 * sum to its reconciled total up to rounding.  The two streams are independent where the keys differ, so with weights
 * equal to the true variances a reconciled total has variance v W / (v + W) and a reconciled row w - w^2 / (v + W).
 * The result depends neither on how the call is cut into scratch chunks (512 MB: the daily sample buffer, a second one
 * with cum_q, and the period buffer), nor on which outputs are wanted, nor on what other series are in the call.  No
 * floating-point atomics.  Behaviour for non-finite draws is unspecified.
 *
 * Refusals (< 0 with a message, before any launch; the context stays usable): everything tsf_predict_windows refuses
 * for its model, its windows (against H) and its levels, and the same for the period model (against K rows); two
 * windows that share a row (tsf_predict_windows allows them; here a row would get two corrections); a NULL share or
 * share_total, a share outside [0, 1] or NaN, a share_total outside [0, 1] and not NaN; a NULL series_key or
 * period_key; a phi outside [0, 1); K outside [1, TSF_MAX_WINDOWS]; a NULL out or out->yhat; an output set that wants
 * nothing but yhat and total; n_q = 0 with q, cum_q or win_q wanted.  N == 0 is a legal no-op.
 * Not detected, the caller's business: a period_key equal to a series_key (the two streams are then shared and the
 * independence above is gone); a ds_period that does not describe the windows.
 *
 * Out of scope: more than two temporal levels (weeks do not nest in months); overlapping windows; cross-temporal
 * reconciliation (a roll-up whose members are temporally reconciled); non-diagonal weights; estimating the weights (w
 * and v are the caller's variances); the job configurations; _dev variants; more than one GPU. */
int tsf_temporal_shares(int64_t N, int32_t H, int32_t K, const int32_t *win_start, const int32_t *win_end /* [K] */,
                        const double *w /* [N][H], NULL = all 1.0 */, const double *v /* [N][K]; NaN = not reconciled */,
                        double *share /* [N][H] */, double *share_total /* [N][K] */);
typedef struct {
    double *yhat;           /* [N][H]        required: the reconciled point forecast */
    double *q;              /* [N][n_q][H]   per-row quantiles of the reconciled draws; NULL: not wanted (all below likewise) */
    double *cum_q;          /* [N][n_q][H]   quantiles of each reconciled sample's running sum over rows 0..h */
    double *total;          /* [N][K]        the reconciled point forecast of every window's total */
    double *win_q;          /* [N][n_q][K]   quantiles of the reconciled window totals */
    double *samples;        /* [N][H][n_samples] the reconciled draws */
    double *win_samples;    /* [N][K][n_samples] the reconciled window totals of every sample */
} tsf_temporal_out;
int tsf_temporal_out_size(void);    /* sizeof(tsf_temporal_out): the self-check of a binding */
int tsf_predict_temporal(tsf_ctx *ctx,
                         const tsf_spec *spec, int64_t N, int32_t H, const double *theta, const double *y_scale,
                         const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future /* [H] or [N][H] */,
                         int32_t shared_future, const double *floor, const double *cap, const double *extra_future,
                         const int64_t *series_key /* [N], required */, const double *noise_ar /* [N] phi or NULL */,
                         const tsf_spec *spec_p, int32_t K, const double *theta_p, const double *y_scale_p,
                         const tsf_grid_info *grid_p, int32_t n_grids_p, const int64_t *ds_period /* [K] or [N][K] */,
                         int32_t shared_period, const double *floor_p, const double *cap_p, const double *extra_period,
                         const int64_t *period_key /* [N], required */, const double *noise_ar_p /* [N] phi or NULL */,
                         int32_t n_samples, uint64_t seed, const int32_t *win_start, const int32_t *win_end /* [K] */,
                         const double *share /* [N][H] */, const double *share_total /* [N][K] */, int32_t n_q,
                         const double *quantiles, tsf_temporal_out *out);

/* ---- correlated group roll-ups: a shared noise factor per group ----------------------------------------
 * The members of a total share weather, promotions and outages, so their forecast errors move together, and the P90
 * of a total of m independent members is too narrow by a factor that grows like sqrt(1 + (m - 1) rho): more than 3 x at
 * m = 100 and rho = 0.1.  Two pieces, both opt-in: an estimator of each group's residual correlation from the fits' own
 * history, and an add route that draws the members' observation noise with that correlation.  Reference interface
 * replaced: none (neither the reference nor fbprophet has such a function); parity unpinned (what is pinned is the
 * contract below: the estimator bit for bit against a numpy restatement, tests/corr_ref.py, and the add against the
 * independent add plus the restated factor term).  Timing: tools/bench_rollup_corr.py; DESIGN.md 5l.
 *
 * Limits, stated plainly.  One factor with equal loading per group: every pair of members of a group gets the same
 * rho.  Contemporaneous correlation only: the factor is independent from row to row.  rho is estimated in sample, on
 * the residuals of the fits' own history.  Only the observation noise is correlated: the sampled trend changes of the
 * members stay independent.  A negative estimate is clipped to 0.  A series rolled up under two groupings (two handles)
 * gets two unrelated factors.  Reconciling correlated draws is out of scope (see the refusals).
 *
 * tsf_residual_corr.  Aligned panels only (co-movement is row by row): y [N][T] in y_dtype; fitted [N][T] double --
 * tsf_predict of each fit on its own history dates, as tsf_fit_screened forms it; group [N], each value in [0, G), or -1
 * for a series that takes no part; args (NULL: the defaults) {rho_max = 0.95, min_rows = 8}.  Outputs per group: rho,
 * status (required), rho_raw, n_pairs, n_used (NULL: not wanted); per series: scale (NULL: not wanted).  Host pointers
 * in the host variant; in _dev y, fitted and every output are device pointers, while group, args and the tsf_corr_out
 * struct itself are HOST memory (the members' lists are built on the host), and the call synchronises the stream before
 * it returns.
 * Contract, in plain double operations with one rounding each (no fused multiply-add, no atomics; a group's result
 * depends on nothing else in the batch):
 *   Per series i: row t is present where r = (double)y - fitted is finite; n_i = the present rows, ss_i = sum of r * r
 *   over them.  n_i < min_rows or ss_i == 0: the series is unused and scale[i] = NaN.  Otherwise
 *   scale[i] = sqrt(ss_i / (double)n_i) and e_it = r_it / scale[i].
 *   Per group g and row t: over the used members present at t, in ascending series index, u = u + e, q = q + e * e,
 *   k += 1 (from +0.0, +0.0, 0); c_t = u * u - q (the sum of e_i e_j over the ordered pairs) and p_t = k (k - 1), an int64.
 *   Per group: A = sum of c_t, P = sum of p_t (an integer: exact), rho_raw = A / (double)P,
 *   rho = fmin(fmax(rho_raw, 0), rho_max), n_pairs = P / 2, n_used = the used members.  P == 0 (a singleton, an empty
 *   group, members that never overlap): rho_raw = NaN, rho = +0.0, status TSF_CORR_NO_PAIRS; otherwise TSF_CORR_OK.
 *   The two sums over t (ss_i, A): 64 partials from +0.0, partial l adds rows l, l + 64, ... in ascending order (an absent
 *   row adds +0.0); the partials are combined by the xor butterfly v[l] = v[l] + v[l ^ d] for d = 1, 2, 4, 8, 16, 32.
 * Refusals (< 0 with a message, before any launch; the context stays usable): a NULL out, out->rho or out->status; NULL
 *   y, fitted or group with N > 0; a group value outside [-1, G); rho_max outside [0, 1]; min_rows < 2; a bad y_dtype;
 *   T < 1; G < 1.  N == 0 is a legal no-op that reports every group TSF_CORR_NO_PAIRS.
 *
 * tsf_rollup_set_noise_corr.  rho [G], each finite and in [0, 1]; group_key [G] (NULL: the group index), the key of each
 * group's factor stream.  Legal only on a handle nothing has been added to.  It stores a_g = sqrt(1 - rho_g) - 1 and
 * b_g = sqrt(rho_g), formed on the host in double (IEEE sqrt), and the keys.  From then on tsf_rollup_add (same
 * signature, checks, chunking and ownership: one accumulator cell, its members added in list order by plain double adds)
 * adds, for a member i of a group with rho_g > 0, at row index h and sample s,
 *   v = v + (x_i + ((a_g * z_i + b_g * w) * sn_i)),    sn_i = exp(theta_i[2]) * y_scale_i  (the library's deterministic exp)
 * where x_i is the member's draw (tsf_predict_quantiles' sample), z_i the standard normal the draw's noise was made from
 * -- Box-Muller sqrt(-2 log u1) cos(2 pi u2) on the stream keyed (seed, series_key[i], s, stream 1) at counters 2h,
 * 2h + 1 -- regenerated, not stored, and w the same expression on the group's stream keyed (seed, group_key[g], s,
 * stream 2) at the same counters, formed once per cell.  The member's noise becomes
 * (sqrt(1 - rho) z_i + sqrt(rho) w) sigma y_scale: its own marginal law is unchanged, any two members of a group have
 * noise correlation rho at the same row and sample, and different rows, samples and groups stay independent.  A group
 * with rho_g == 0 takes the independent expression v = v + x_i exactly, so its bits are those of a handle without a
 * correlation; ysum and count are carried as always.  The result still depends neither on the chunking nor on what else
 * a call contains.  tsf_rollup_quantiles and tsf_rollup_windows read the accumulators and need nothing new.
 * Refusals (< 0 with a message; the accumulators are untouched and the handle and the context stay usable):
 *   set_noise_corr after any add or set_totals, on a poisoned handle, with a NULL rho, or with a rho that is not finite
 *   or outside [0, 1]; tsf_rollup_set_totals, tsf_rollup_reconcile and tsf_rollup_reconciled_totals on a handle with a
 *   correlation set.
 * Out of scope: ragged panels; several factors or unequal loadings; correlated trend changes; lagged correlation; the
 * job configurations (the scorer has models and no history). */
enum { TSF_CORR_OK = 0, TSF_CORR_NO_PAIRS = -50 };
typedef struct {
    double rho_max;         /* the estimate is clipped to [0, rho_max]; default 0.95 */
    int32_t min_rows;       /* a series with fewer present rows is unused; default 8 */
    int32_t reserved_;      /* 0 */
} tsf_corr_args;
typedef struct {
    double *rho;            /* [G] required: the clipped estimate, what tsf_rollup_set_noise_corr takes */
    double *rho_raw;        /* [G] the estimate before clipping (NaN without pairs); NULL: not wanted */
    int64_t *n_pairs;       /* [G] member pairs summed over the rows; NULL: not wanted */
    int32_t *n_used;        /* [G] the group's used members; NULL: not wanted */
    int32_t *status;        /* [G] required: TSF_CORR_* */
    double *scale;          /* [N] each series' residual root mean square (NaN: unused); NULL: not wanted */
} tsf_corr_out;
int tsf_corr_args_size(void);       /* sizeof(tsf_corr_args), sizeof(tsf_corr_out): the self-checks of a binding */
int tsf_corr_out_size(void);
int tsf_residual_corr(tsf_ctx *ctx, int64_t N, int32_t T, const void *y, int32_t y_dtype, const double *fitted,
                      const int64_t *group /* [N], each in [-1, G) */, int64_t G, const tsf_corr_args *args /* NULL = defaults */,
                      tsf_corr_out *out);
int tsf_residual_corr_dev(tsf_ctx *ctx, int64_t N, int32_t T, const void *y, int32_t y_dtype, const double *fitted,
                          const int64_t *group, int64_t G, const tsf_corr_args *args, tsf_corr_out *out, void *stream);
int tsf_rollup_set_noise_corr(tsf_rollup *r, const double *rho /* [G] */, const int64_t *group_key /* [G], NULL = g */);

/* ---- serially correlated observation noise: AR(1) per series ---------------------------------------
 * The observation noise of the draws is independent from row to row; the residuals of a real fit are not (a promotion,
 * a cold spell, an outage lasts several rows), and with lag-one autocorrelation phi the spread of a total over n rows
 * is too narrow by a factor that tends to sqrt((1 + phi) / (1 - phi)): 2.0 at phi = 0.6, 1.36 at phi = 0.3.  This is the
 * time-direction twin of the correlated roll-ups above.  Two pieces, both opt-in: an estimator of each series' residual
 * autocorrelation from the fit's own history, and a one-shot context setting that makes the next drawing entry chain the
 * noise of each sample's rows.  Reference interface replaced: none (neither the reference nor fbprophet has such a
 * function); parity unpinned (what is pinned is the contract below: the estimator bit for bit against a numpy
 * restatement, tests/ar_ref.py, and the chain against the independent draw's own normals).  Timing:
 * tools/bench_noise_ar.py; DESIGN.md 5o.  Without a setting every entry is what it always was, bit for bit.
 *
 * Limits, stated plainly.  Lag one ROW, not one unit of time: a Friday-to-Monday pair counts as lag one, rows are taken
 * as equally spaced (in the history for the estimate, in the future for the draw).  phi is estimated in sample, on
 * residuals that a flexible fit shrinks and may push negative.  A negative estimate is clipped to 0 (phi_raw is there
 * for the caller who wants it).  Uncentred: the residuals' mean is taken as 0.  The estimator is biased towards 0 by a
 * term of order phi / T: with A = sum r_t r_{t-1} / np, B = ss / n and a Gaussian AR(1) of unit variance,
 * Cov(A, B) ~ 4 phi / (T (1 - phi^2)) and Var(B) ~ 2 (1 + phi^2) / (T (1 - phi^2)), so the ratio's second-order
 * expansion E[A / B] ~ phi - Cov(A, B) + phi Var(B) gives E[phi_raw] ~ phi - 2 phi / T; what the fit's own parameters
 * remove from the residuals comes on top and is not derived here.  Only the observation noise is chained: the sampled
 * trend changes are what they were.  One phi per series: no higher lags, no seasonal lag.
 *
 * tsf_residual_autocorr.  Panel: aligned (offsets NULL: y, fitted are [N][T]) or ragged (T ignored; series n owns rows
 * offsets[n] .. offsets[n + 1], as tsf_screen_rows takes them).  y in y_dtype; fitted double -- tsf_predict of each fit
 * on its own history dates; args (NULL: the defaults) {phi_max = 0.95, min_pairs = 8}.  Outputs per series: phi, status
 * (required), phi_raw, n_pairs, scale (NULL: not wanted).  Host pointers in the host variant; in _dev y, fitted and
 * every output are device pointers, while offsets, args and the tsf_ar_out struct itself are HOST memory, and the call
 * synchronises the stream before it returns.
 * Contract, in plain double operations with one rounding each (no fused multiply-add, no atomics; a series' result
 * depends on nothing else in the batch):
 *   Row t of a series is present where r_t = (double)y_t - fitted_t is finite; n = the present rows, ss = sum of
 *   r_t * r_t over them.  A pair is a row t >= 1 of the series with t and t - 1 both present; np = the pairs,
 *   C = sum of r_t * r_{t-1} over them.
 *   phi_raw = (C / (double)np) / (ss / (double)n),  phi = fmin(fmax(phi_raw, 0), phi_max),
 *   scale = sqrt(ss / (double)n), n_pairs = np.
 *   np < min_pairs or ss == 0: phi_raw = NaN, phi = +0.0, status TSF_AR_NO_PAIRS; otherwise TSF_AR_OK.  scale is NaN
 *   only where n == 0 or ss == 0.
 *   The two sums (ss, C): 64 partials from +0.0, partial l adds rows (for C: pairs, by their row t) l, l + 64, ... of the
 *   series in ascending order (an absent row or pair adds +0.0); the partials are combined by the xor butterfly
 *   v[l] = v[l] + v[l ^ d] for d = 1, 2, 4, 8, 16, 32.
 * Refusals (< 0 with a message, before any launch; the context stays usable): a NULL out, out->phi or out->status; NULL
 *   y or fitted with N > 0; a bad y_dtype; phi_max outside [0, 1); min_pairs < 1; T < 1 on an aligned call; offsets
 *   that do not start at 0 or decrease.  N == 0 is a legal no-op.
 *
 * tsf_set_noise_ar.  phi: HOST [n], each finite with |phi| < 1 (a negative value is legal here: the estimator never
 * returns one, a caller may); NULL or n == 0 clears.  The setting is consumed by the NEXT drawing entry on this context
 * and is gone afterwards whatever that call returns.  It stores c = sqrt(1 - phi * phi) beside each phi, formed on the
 * host in double (IEEE sqrt).  The entries that take it, with their _dev forms: tsf_predict_intervals,
 * tsf_predict_quantiles, tsf_score_actuals, tsf_predict_windows, and tsf_rollup_add on a handle without a noise
 * correlation; phi[i] belongs to series i of that call, and a call with N != n fails with a message (it is never
 * silently ignored: this is a statistical setting, not a scheduling hint).  The pairs cross to the device from host
 * memory, so a _dev entry that takes a setting synchronises its stream once, before its first launch.  In such a call
 * the standard normal z_h that the draw of series i, sample s, row h makes from its noise stream (counters 2h, 2h + 1:
 * untouched) is replaced by e_h:
 *   e_0 = z_0;   e_h = phi * e_{h-1} + c * z_h   (two products and one add, each rounded),
 * in the caller's row order, never restarted -- not where unsorted future rows restart the trend sweep either, the rule
 * of the running sum -- and the sample is trend * (1 + mult) + add + (e_h * sigma) * y_scale as always.  A series with
 * phi == 0 takes the independent expression exactly (a select, not 0 * e + 1 * z), so its bits are those of a call
 * without a setting.  The start is stationary, so each row's marginal law is unchanged (per-row quantiles and intervals
 * keep their law), rows i, j of one sample correlate phi^|i - j|, and samples, series and the sampled trend stay
 * independent; sample s still depends on nothing but (seed, series key, s, phi).  Every consumer of the draws inherits
 * the chain: the running sums, the window totals, the scores, the roll-up's accumulators.
 * Every other entry that draws refuses (< 0 with a message, before any launch) while a setting is pending, and clears
 * it: tsf_predict_components, tsf_cross_validate and tsf_calibrate, tsf_rollup_set_totals, tsf_rollup_reconcile, and
 * tsf_rollup_add on a handle with tsf_rollup_set_noise_corr (that route regenerates z from the counters and would
 * disagree with the chain).  Entries that do not draw (fits, tsf_predict, the roll-up's reads) leave the setting alone.
 * The jobs: the modeler writes each series' phi beside its models and the scorer draws with it (model.noise, io.noise,
 * forecast.noise: "the noise state of a fitted panel" below).  Out of scope: the model blob. */
enum { TSF_AR_OK = 0, TSF_AR_NO_PAIRS = -51 };
typedef struct {
    double phi_max;         /* the estimate is clipped to [0, phi_max]; default 0.95; in [0, 1) */
    int32_t min_pairs;      /* a series with fewer pairs gets phi = 0 and TSF_AR_NO_PAIRS; default 8 */
    int32_t reserved_;      /* 0 */
} tsf_ar_args;
typedef struct {
    double *phi;            /* [N] required: the clipped estimate, what tsf_set_noise_ar takes */
    double *phi_raw;        /* [N] the estimate before clipping (NaN without pairs); NULL: not wanted */
    int64_t *n_pairs;       /* [N] the pairs of the series; NULL: not wanted */
    double *scale;          /* [N] the residual root mean square; NULL: not wanted */
    int32_t *status;        /* [N] required: TSF_AR_* */
} tsf_ar_out;
int tsf_ar_args_size(void);         /* sizeof(tsf_ar_args), sizeof(tsf_ar_out): the self-checks of a binding */
int tsf_ar_out_size(void);
int tsf_residual_autocorr(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets /* NULL = aligned [N][T] */, const void *y,
                          int32_t y_dtype, const double *fitted, const tsf_ar_args *args /* NULL = defaults */,
                          tsf_ar_out *out);
int tsf_residual_autocorr_dev(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets /* host */, const void *y,
                              int32_t y_dtype, const double *fitted, const tsf_ar_args *args, tsf_ar_out *out, void *stream);
int tsf_set_noise_ar(tsf_ctx *ctx, const double *phi /* host [n] */, int64_t n);

/* ---- serially correlated observation noise: the conditioned start ------------------------------------
 * The chain above starts every sample at the stationary law, e_0 = z_0: right for a forecast that begins far from the
 * data.  A forecast that begins at the row behind the history does not: the fit has just seen the last residual.  If the
 * last present row stood r above the fit (y units) and the residuals are an AR(1) with autocorrelation phi and marginal
 * deviation sigma y_scale, then the noise of the row `steps` rows behind it has mean phi^steps r and variance
 * (1 - phi^(2 steps)) sigma^2 y_scale^2, and the rows after it follow the same recursion as always.  With p0 = phi^steps:
 * the noise of future row h has mean m_h = p0 phi^h r and variance (1 - (p0 phi^h)^2) sigma^2 y_scale^2, rows i <= j have
 * noise covariance phi^(j - i) times row i's variance, and as h grows everything tends to the stationary chain.  The
 * point forecast gains the correction of a regression with AR(1) errors (yhat + m_h: it removes the share p0^2 of the
 * first row's squared error, 36 % at phi = 0.6 and steps = 1), the near rows' intervals narrow by sqrt(1 - p0^2), and
 * totals, running sums, roll-ups and scores inherit both, being functions of the same draws.  Three pieces, all opt-in;
 * reference interface replaced: none; parity unpinned (pinned: the contract below, restated in numpy in
 * tests/ar_start_ref.py).  Timing: tools/bench_noise_ar_start.py; DESIGN.md 5s.  Without the new setting every entry is
 * what it was, bit for bit -- the stationary chain included.
 *
 * tsf_residual_last.  The panel arguments of tsf_residual_autocorr (aligned, or ragged by offsets; y in y_dtype, fitted
 * double).  Outputs per series, all three required: last_resid = r_t = (double)y_t - fitted_t of the last present
 * (finite) row t; last_gap (int32) = the rows of the series behind that row, 0 where the final row is present; status
 * TSF_AR_OK, or TSF_AR_NO_ROW for a series without a present row (an empty one too), whose last_resid is +0.0 and whose
 * last_gap is its row count.  Host pointers in the host variant; in _dev y, fitted and the three outputs are device
 * pointers, offsets and the tsf_ar_last_out struct itself are HOST memory, and the call synchronises the stream before
 * it returns.  One launch, one wave per series, which reads the series from its end in blocks of 64 rows and stops at the
 * first block with a present row.  Refusals: those of tsf_residual_autocorr (but for its args), a NULL last_resid,
 * last_gap or status, and a ragged series of more than 2^31 - 1 rows; N == 0 is a legal no-op.
 * tsf_residual_autocorr_last (host pointers only) is both calls on one copy of the panel: the copy-in of y and fitted is
 * most of either, and a caller of the conditioned start wants both.  Its outputs are those of the two entries, bit for
 * bit, and its refusals the union of theirs.
 *
 * tsf_set_noise_ar_start.  resid: HOST [n], y units, each finite; steps: HOST [n], each >= 1: last_gap plus the number
 * of rows from the end of the history to the first future row (normally the next row: 1) -- lag one ROW, as above.  Legal
 * only while a tsf_set_noise_ar setting for the same n is pending: without one, or with another n, it is refused (< 0,
 * a message) and the pending setting is cleared; a bad resid or steps is refused likewise and clears it too (a
 * statistical setting is never half applied).  NULL resid or steps, or n == 0, clears the start only.  A later
 * tsf_set_noise_ar clears the start.  Both settings are consumed together by the next drawing entry, under the one-shot
 * rule above.  It stores per series, formed on the host in plain double operations with one rounding each (no fused
 * multiply-add):
 *   p0 = phi multiplied by itself steps - 1 more times (the loop stops at the first zero, whose sign it keeps);
 *   c0 = sqrt(1 - p0 * p0);   m0 = resid * p0
 * in an array [n][3] of its own beside the (phi, c) pairs, which are what they were.
 *
 * tsf_noise_ar_mean (host only, no context, nothing launched; < 0 for a bad argument: n < 0, H < 0, a NULL array that is
 * needed, |phi| >= 1 or not finite, a non-finite resid, steps < 1).  The conditional mean in y units, [n][H]:
 *   mean[i][0] = m0 = resid[i] * p0;   mean[i][h] = phi[i] * mean[i][h - 1]   (one product each).
 *
 * The conditioned draw.  In a call that holds both settings, series i is drawn with m_h = tsf_noise_ar_mean's values and
 * z_h the same counter-based normals as always (counters 2h, 2h + 1 of the noise stream, untouched):
 *   e_0 = c0 * z_0;   e_h = phi * e_(h-1) + c * z_h   (the expression above);
 *   sample = trend * (1 + mult) + (add + m_h) + (e_h * sigma) * y_scale;   yhat' = yhat + m_h   (one add).
 * The mean travels in the additive piece: a kernel of its own (ar_start_shift_kernel, one thread per series and row) runs
 * behind the point forecast's kernel and in front of the sample kernel; it forms m_h by the recursion above and adds it to
 * the chunk's additive term (add * y_scale, already rounded: `add` above) and to yhat, one add each.  The order of the adds in
 * a sample is therefore (trend * (1 + mult) + (add + m_h)) + noise.  The sample kernel's third instance differs from the
 * chained one in e_0 alone.  A series with phi == 0 takes the independent expression exactly (a select), and neither its
 * additive term nor its yhat is touched, whatever resid is.  The sampled trend and trend_out are unchanged; ysum of a
 * roll-up accumulates the shifted yhat.  Sample s depends on nothing but (seed, series key, s, phi, resid, steps).
 * The entries that take the start are exactly those that take tsf_set_noise_ar; those that refuse a pending setting
 * refuse as before and clear both.
 *
 * Limits.  tsf_predict_temporal takes its phi as arguments, not through the setting, and keeps the stationary start (its
 * signature is published).  No conditioning inside tsf_cross_validate, tsf_calibrate, tsf_tune and tsf_select: the folds
 * would need each fold's fitted history; none on roll-ups with a noise correlation; no higher lags; the chain
 * runs on rows, not on the calendar; the model blob is untouched (the state travels in a table of its own: "the noise
 * state of a fitted panel" below); no devices= split; no
 * existing signature or struct changes (tsf_ar_out is what it was). */
enum { TSF_AR_NO_ROW = -52 };       /* beside TSF_AR_OK: a series without a present row */
typedef struct {
    double *last_resid;     /* [N] required: the last present row's residual, y units (+0.0 without one) */
    int32_t *last_gap;      /* [N] required: the rows of the series behind that row */
    int32_t *status;        /* [N] required: TSF_AR_OK or TSF_AR_NO_ROW */
} tsf_ar_last_out;
int tsf_ar_last_out_size(void);     /* sizeof(tsf_ar_last_out): the self-check of a binding */
int tsf_residual_last(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets /* NULL = aligned [N][T] */, const void *y,
                      int32_t y_dtype, const double *fitted, tsf_ar_last_out *out);
int tsf_residual_last_dev(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets /* host */, const void *y,
                          int32_t y_dtype, const double *fitted, tsf_ar_last_out *out, void *stream);
/* tsf_residual_autocorr and tsf_residual_last on one copy of the panel (host pointers): both results, each bit for bit */
int tsf_residual_autocorr_last(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y, int32_t y_dtype,
                               const double *fitted, const tsf_ar_args *args, tsf_ar_out *out, tsf_ar_last_out *last);
int tsf_set_noise_ar_start(tsf_ctx *ctx, const double *resid /* host [n], y units */, const int32_t *steps /* host [n], >= 1 */,
                           int64_t n);
int tsf_noise_ar_mean(int64_t n, const double *phi, const double *resid, const int32_t *steps, int32_t H,
                      double *mean /* [n][H] */);

/* ---- serially correlated observation noise: the noise state of a fitted panel --------------------------
 * What the conditioned start needs from a history -- phi, the last present row's residual and the rows behind it -- are
 * five numbers per series, and the modeler holds the history at the moment it fits.  By hand they cost a forecast of the
 * whole history ([rows] fitted values to the host and back) for the two estimator entries above to read.
 * tsf_noise_state forms them in one launch from the panel and its fit, with no buffer of fitted values at any point;
 * tsf_predict_conditioned is the corrected point forecast with the reference's integer column, for the caller who has the
 * numbers and no history (the scorer job: DESIGN.md 5u).  Both opt-in; reference interface replaced: none; parity unpinned
 * (pinned: the contract below, against tsf_predict, tsf_residual_autocorr, tsf_residual_last and tsf_noise_ar_mean).
 * Timing: tools/bench_noise_state.py.
 *
 * tsf_noise_state.  The panel arguments of tsf_fit_aligned (offsets NULL: ds [T], y [N][T], extra [n_extra][T]) or
 * tsf_fit_ragged (offsets [N + 1], T ignored: ds, y [total_rows], extra [n_extra][total_rows]), floor / cap [N] or NULL as
 * there; a fit of that panel (theta [N][tsf_theta_stride(spec)], y_scale [N], grid [n_grids], n_grids = 1 or N, status
 * [N]); excluded (uint8 in y's layout, 1 = the row is absent, as if y were NaN there) or NULL; args (NULL: the defaults
 * of tsf_ar_args).  Outputs per series: every field of tsf_ar_out and of tsf_ar_last_out -- phi, status, last_resid,
 * last_gap, last_status required; phi_raw, n_pairs, scale NULL where not wanted -- and last_ds_ns (NULL: not wanted): the
 * date of the series' final row, present or not, INT64_MIN for an empty series.
 * Contract: each output is bit for bit what tsf_predict on the series' own dates (with the same floor, cap and explicit
 * columns), then tsf_residual_autocorr, then tsf_residual_last give, for every model tsf_predict takes; a series' result
 * depends on nothing else in the batch.  A series whose fit status is negative has no fitted values (its grid may be the
 * degenerate one of a series of fewer than two rows, which tsf_predict refuses): phi = +0.0, phi_raw and scale NaN,
 * n_pairs 0, TSF_AR_NO_PAIRS, TSF_AR_NO_ROW, last_resid +0.0, last_gap = its row count.
 * One launch (noise_state_kernel), one wave per series: lane l takes rows l, l + 64, ...; per row the fitted value by
 * predict_kernel's per-series-date arithmetic, the residual, and the residual into ar_series_kernel's sums (the left
 * neighbour by shuffle, a carry across 64-row steps).
 * Host pointers in the host variant.  In _dev ds, y, floor, cap, extra, theta, y_scale, grid, status, excluded and every
 * output are device pointers; spec, offsets, args and the tsf_noise_state_out struct itself are HOST memory, and the call
 * synchronises the stream before it returns.
 * Refusals (< 0 with a message, before any launch; the context stays usable): those of tsf_residual_autocorr and
 * tsf_residual_last on the panel (N outside [0, 2^31 - 1], a NULL required output, a bad y_dtype or args, T < 1 aligned,
 * offsets that do not start at 0 or decrease, a series of more than 2^31 - 1 rows); with N > 0 those of tsf_predict (a
 * bad spec, NULL ds, y, theta, y_scale, grid or status, n_grids other than 1 or N, NULL extra with n_extra > 0, logistic
 * growth without cap, and -- host variant -- a grid of a series with status >= 0 that tsf_predict refuses) and -- host
 * variant -- an excluded value other than 0 / 1.  N == 0 is a legal no-op.
 *
 * tsf_predict_conditioned.  tsf_predict's arguments, then phi, resid, steps: HOST [N] in both variants, checked as
 * tsf_set_noise_ar and tsf_set_noise_ar_start check them (phi finite with |phi| < 1, resid finite, steps >= 1).
 *   yhat = tsf_predict's, plus tsf_noise_ar_mean's row values for the series with phi != 0 (one add per cell): the bits of
 *   the yhat a drawing entry returns under the same conditioned start.
 *   yhat_int (NULL: not wanted) = the reference's post-step on that corrected yhat: truncate toward zero, saturate to
 *   int32, clamp to floor -- the expression of tsf_predict, one device function both kernels call.
 *   A series with phi == 0 gets tsf_predict's two outputs bit for bit.
 * predict_kernel, then conditioned_shift_kernel (one thread per series and row) on the same stream.  It reads no pending
 * tsf_set_noise_ar setting and leaves one alone.  _dev: the forecast's arrays and both outputs are device pointers, and
 * the call synchronises the stream before it returns (the (phi, m0) pairs cross from host memory). */
typedef struct {
    double *phi;            /* [N] required: tsf_ar_out's fields */
    double *phi_raw;        /* [N] or NULL */
    int64_t *n_pairs;       /* [N] or NULL */
    double *scale;          /* [N] or NULL */
    int32_t *status;        /* [N] required: TSF_AR_OK or TSF_AR_NO_PAIRS */
    double *last_resid;     /* [N] required: tsf_ar_last_out's fields */
    int32_t *last_gap;      /* [N] required */
    int32_t *last_status;   /* [N] required: TSF_AR_OK or TSF_AR_NO_ROW */
    int64_t *last_ds_ns;    /* [N] or NULL: the date of the final row, INT64_MIN for an empty series */
} tsf_noise_state_out;
int tsf_noise_state_out_size(void); /* sizeof(tsf_noise_state_out): the self-check of a binding */
int tsf_noise_state(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets /* NULL = aligned */,
                    const int64_t *ds, const void *y, int32_t y_dtype, const double *floor, const double *cap,
                    const double *extra, const double *theta, const double *y_scale, const tsf_grid_info *grid,
                    int32_t n_grids, const int32_t *status, const uint8_t *excluded /* NULL = none */,
                    const tsf_ar_args *args /* NULL = defaults */, tsf_noise_state_out *out);
int tsf_noise_state_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets /* host */,
                        const int64_t *ds, const void *y, int32_t y_dtype, const double *floor, const double *cap,
                        const double *extra, const double *theta, const double *y_scale, const tsf_grid_info *grid,
                        int32_t n_grids, const int32_t *status, const uint8_t *excluded, const tsf_ar_args *args,
                        tsf_noise_state_out *out, void *stream);
int tsf_predict_conditioned(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                            const double *y_scale, const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future,
                            int32_t shared_future, const double *floor, const double *cap, const double *extra_future,
                            const double *phi /* host [N] */, const double *resid /* host [N] */,
                            const int32_t *steps /* host [N] */, double *yhat, int32_t *yhat_int);
int tsf_predict_conditioned_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                                const double *y_scale, const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future,
                                int32_t shared_future, const double *floor, const double *cap, const double *extra_future,
                                const double *phi, const double *resid, const int32_t *steps, double *yhat,
                                int32_t *yhat_int, void *stream);

/* ---- conditional seasonalities ---------------------------------------------------------------------
 * Replaces the `condition_name=` argument of fbprophet 0.5's `Prophet.add_seasonality(name, period, fourier_order,
 * prior_scale, mode, condition_name)`: a seasonality that applies only on the rows where a boolean column of the frame
 * is true -- a weekly pattern that differs in and out of season, a daily pattern that differs on weekdays and
 * weekends.  fbprophet builds the seasonality's Fourier columns and sets them to 0 on the rows where the column is
 * false (make_all_seasonality_features: `features[~df[condition_name]] = 0`).  The reference job never adds one
 * (prophet_modeler.py:65 takes the constructor's defaults); it is here because users of the model expect it.
 *
 * Here a conditional seasonality is LOWERED to explicit design columns: 2 * order entries of tsf_spec's extra columns
 * per seasonality (prior scale and mode per column), whose values this entry builds from the timestamps and the
 * condition rows.  No fit, predict or sampling kernel knows about conditions: every entry point that takes `extra` /
 * `extra_future` follows.  For seasonality s (period p, order m, condition row c) the entry writes 2 * m columns
 * [sin 1, cos 1, sin 2, cos 2, ...], seasonalities in the order of the struct, column j of the whole at
 * cols + j * col_stride:
 *   - row i with cond[c][i] != 0: the value the fit's own tables hold for an unconditional seasonality of that period
 *     and order at timestamp ds[i] -- bit for bit (the same statements: the first harmonic from the library's sincos
 *     at 2 pi t / p, t in days since the epoch, the others by the recurrence u[h+1] = 2 cos u[h] - u[h-1]);
 *   - row i with cond[c][i] == 0: +0.0.
 * A value is a function of (ds[i], p, harmonic, cond[c][i]) alone: not of the panel's first timestamp, of `rows` or of
 * where the row stands, so the columns of a sub-range of rows are the sub-range of the columns (cross-validation folds,
 * future rows).  cols may point INTO the caller's extra block -- col_stride is its row length -- beside the holiday and
 * regressor columns; nothing but the rows [0, rows) of the sum of 2 * order columns is written.
 *   - cs is host memory in both variants (as tsf_spec); ds / cond / cols are host pointers in the plain variant, device
 *     pointers in _dev, which is asynchronous on `stream`.
 *   - rows = 0 is a legal no-op.
 *   - API misuse (return < 0, text through tsf_last_error, before any launch; the context stays usable): col_stride <
 *     rows; n outside [1, TSF_MAX_SEAS]; a period that is not finite and > 0; an order < 1, or orders whose columns
 *     exceed TSF_MAX_EXTRA; a condition index outside [0, n_cond).
 * Deviation, on purpose: fbprophet keeps a conditional seasonality's columns among the seasonal columns, in the order
 * the seasonalities were added; here they stand among the extra columns, behind the holidays and the caller's
 * regressors.  The posterior is the same function of the same columns; the optimiser's trajectory -- and with it the
 * last bits of a Stan-rule fit -- depends on the column order, as it does for every fit of this library.  A model with
 * such columns has explicit columns, so its fits leave the lattice tables and the in-register harmonic expansion, as a
 * model with holidays does.
 * These semantics are restated from recall of fbprophet 0.5; parity with fbprophet itself is unpinned, as everywhere
 * in this library. */
typedef struct {
    int32_t n;                          /* conditional seasonalities, 1 .. TSF_MAX_SEAS */
    double  period[TSF_MAX_SEAS];       /* days, finite, > 0 */
    int32_t order[TSF_MAX_SEAS];        /* >= 1; sum of 2*order <= TSF_MAX_EXTRA */
    int32_t cond[TSF_MAX_SEAS];         /* index of its condition row, in [0, n_cond) */
} tsf_cond_seas;
int tsf_cond_columns(tsf_ctx *ctx, const tsf_cond_seas *cs, int64_t rows, const int64_t *ds,
                     int32_t n_cond, const uint8_t *cond /* [n_cond][rows], non-zero = true */,
                     double *cols /* [sum 2*order][col_stride] */, int64_t col_stride);
int tsf_cond_columns_dev(tsf_ctx *ctx, const tsf_cond_seas *cs, int64_t rows, const int64_t *ds,
                         int32_t n_cond, const uint8_t *cond, double *cols, int64_t col_stride, void *stream);

/* ---- totals over row windows: quantiles and scores of calendar-period totals ----------------------------
 * "P10 / P50 / P90 of next week's total, of each calendar month, of every rolling 7-row block", for a series and for
 * a roll-up's group total, and how an observed total scores against it.  cum_q answers this only for windows that start
 * at row 0; a later window cannot be had by differencing two of its quantiles (quantiles of sums are not sums or
 * differences of quantiles), and summing tsf_predict_quantiles' raw samples on the host moves N * H * n_samples values.
 * Here every sample's rows are summed over each window [win_start[k], win_end[k]) on the device, on the way into the
 * per-row kernels' sort, and only [N][K]-sized answers leave it.  No second sample buffer is taken (cum_q takes one).
 * Which rows make a week or a month is the caller's business: the library sees row indices (the Python layer's
 * period_windows forms them from a calendar).
 * Reference interface replaced: none (neither the reference nor fbprophet has such a function); parity unpinned (what
 * is pinned is the contract below, against tsf_predict_quantiles, tsf_score_actuals and tsf_rollup_quantiles).
 * Timing: tools/bench_windows.py; DESIGN.md 5k.
 *
 * tsf_predict_windows: the arguments up to seed are tsf_predict_quantiles' and mean what they mean there (the same
 * grid check runs first, N > 0, n_samples in [2, 4096]); n_q, the levels and their checks are its as well.
 * K in [1, TSF_MAX_WINDOWS]; win_start, win_end [K] with 0 <= win_start[k] < win_end[k] <= H: row indices, end
 * exclusive.  Windows may overlap, repeat and come in any order.  y_win [N][K]: the observed total of every window,
 * NaN = not observed (the caller decides what a window with a missing row is worth; the Python layer's window_totals
 * makes it NaN); NULL where nothing is scored.  quantiles, win_start, win_end and the tsf_window_out struct are HOST
 * memory in both variants (the windows are checked before anything is launched); y_win and the pointers inside the
 * struct are host pointers in the host variant and device pointers in _dev.
 *
 * Contract:
 *   The draws are tsf_predict_quantiles' draws (same generator, keys and counters; the chunking budget counts one
 *   sample buffer).  The window sum of sample s is
 *     c = sample[s][a];  c = c + sample[s][h] for h = a + 1 .. b - 1      (a = win_start[k], b = win_end[k])
 *   plain double adds in the row order the caller gave: the running sum of tsf_predict_quantiles started at row a.
 *   v[0 .. n_samples) below is a window's sums sorted ascending, y its y_win.
 *   q[n][i][k] is tsf_predict_quantiles' expression at level quantiles[i] over v (same pos, lo, hi, same roundings);
 *   pit, crps [n][k] and pinball [n][i][k] are tsf_score_actuals' expressions over v and y, operation for operation
 *   (the mid-distribution PIT from exact counts; the CRPS regrouped to non-negative terms and summed by the fixed
 *   halving tree, with tsf_score_actuals' error bound; NaN where y is NaN, q still written).
 *   n_obs, mean_crps, mean_pinball and coverage are tsf_score_actuals' per-series rule with the windows in the place
 *   of the rows: over the windows in the order given, plain double adds from +0.0, NaN where n_obs = 0.  A window
 *   given twice counts twice.
 *   yhat is tsf_predict's, bit for bit.  total[n][k] = yhat[n][a] + ... + yhat[n][b - 1], added one row at a time in
 *   row order from the first row's value: the sum of the point forecasts, not the mean of the draws.
 *   Identities (bit for bit): with the windows [h, h + 1) for every h, q is tsf_predict_quantiles' q, total is yhat,
 *   and pit / crps / pinball and the per-series means are tsf_score_actuals' on y_obs = y_win; with the windows
 *   [0, h + 1) for every h, q is tsf_predict_quantiles' cum_q.
 *   No floating-point atomics.  Every output depends neither on how the call is cut into scratch chunks, nor on what
 *   else is in the batch, nor on the other windows of the call, nor on which other outputs are requested.  Per-window
 *   arrays the requested aggregates need and the caller did not ask for live in the context's scratch.
 *   Behaviour for non-finite draws is unspecified (as for the quantiles).
 *
 * tsf_rollup_windows: the same over the handle's accumulators acc[g][h][s], a group in the place of a series (N = G,
 * y_win [G][K]); yhat is the handle's ysum and total its window sums.  With the windows [h, h + 1) q is
 * tsf_rollup_quantiles' q and with [0, h + 1) its cum_q, bit for bit.  Like tsf_rollup_quantiles it may be called at
 * any time, between adds as well, and does not modify the handle; a group nobody was added to gives 0.0 in yhat,
 * total and q.  Host pointers only.
 *
 * Refusals (< 0 with a message, before any launch; the context and the handle stay usable): a NULL out; an output set
 * that wants nothing; K outside [1, TSF_MAX_WINDOWS]; NULL win_start or win_end; a window with win_start < 0,
 * win_start >= win_end or win_end > H; n_samples outside [2, 4096]; a bad n_q or level; n_q = 0 with q, pinball,
 * mean_pinball or coverage requested; a score output (pit, crps, pinball, n_obs, mean_crps, mean_pinball, coverage)
 * with a NULL y_win; in the host-pointer entries an infinite y_win value (the _dev variant cannot look: there it is
 * the caller's business); tsf_predict_quantiles' refusals of the forecast's inputs; a poisoned roll-up.
 *
 * Out of scope: windows of the trend draws; windows of the reconciled draws (tsf_rollup_reconcile /
 * _reconciled_totals); windows over cross-validation folds; a roll-up `periods` key in the job configuration;
 * per-series calendars in the Python layer's period_windows (row windows themselves work on any rows, per-series and
 * unsorted ones included: the sum follows the caller's row order). */
#define TSF_MAX_WINDOWS 4096
typedef struct {
    double *yhat;           /* [N][H]        tsf_predict's, bit for bit; NULL: not wanted (all below likewise) */
    double *total;          /* [N][K]        the sum of yhat over each window's rows */
    double *q;              /* [N][n_q][K]   quantiles of the window sums of the draws */
    double *pit;            /* [N][K] */
    double *crps;           /* [N][K] */
    double *pinball;        /* [N][n_q][K] */
    int32_t *n_obs;         /* [N]           windows with a non-NaN y_win */
    double *mean_crps;      /* [N] */
    double *mean_pinball;   /* [N][n_q] */
    double *coverage;       /* [N][n_q] */
} tsf_window_out;
int tsf_window_out_size(void);      /* sizeof(tsf_window_out): the self-check of a binding */
int tsf_predict_windows(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                        const double *y_scale, const tsf_grid_info *grid, int32_t n_grids, const int64_t *ds_future,
                        int32_t shared_future, const double *floor, const double *cap, const double *extra_future,
                        const int64_t *series_key, int32_t n_samples, uint64_t seed, int32_t K,
                        const int32_t *win_start /* [K] */, const int32_t *win_end /* [K], exclusive */,
                        const double *y_win /* [N][K] or NULL, NaN = not observed */, int32_t n_q,
                        const double *quantiles, tsf_window_out *out);
int tsf_predict_windows_dev(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t H, const double *theta,
                            const double *y_scale, const tsf_grid_info *grid, int32_t n_grids,
                            const int64_t *ds_future, int32_t shared_future, const double *floor, const double *cap,
                            const double *extra_future, const int64_t *series_key, int32_t n_samples, uint64_t seed,
                            int32_t K, const int32_t *win_start, const int32_t *win_end, const double *y_win,
                            int32_t n_q, const double *quantiles, tsf_window_out *out, void *stream);
int tsf_rollup_windows(tsf_rollup *r, int32_t K, const int32_t *win_start, const int32_t *win_end,
                       const double *y_win /* [G][K] or NULL */, int32_t n_q, const double *quantiles,
                       tsf_window_out *out);

/* ---- cross-validation ---------------------------------------------------------------------
 * fbprophet 0.5 diagnostics.cross_validation + performance_metrics for a whole panel: every series is refitted at
 * several cutoffs and each fold's forecast is scored against the rows held out after its cutoff.  The semantics are
 * restated from recall of fbprophet 0.5's diagnostics.py; parity with the real package is not pinned by any test.
 *
 * Cutoffs, per series (generate_cutoffs; times int64 ns):
 *   the first is max(ds) - horizon (before min(ds): status TSF_CV_LESS_THAN_HORIZON); step back by period while the
 *   last cutoff is >= min(ds) + initial; where (cutoff, cutoff + horizon] holds no row, jump to (the last ds <= cutoff)
 *   - horizon; drop the last cutoff appended (none left: TSF_CV_NO_CUTOFF); ascending order.
 * Fold c of a series fits rows ds <= cutoff_c (fewer than 2: TSF_CV_TOO_FEW, the series gets no fold at all) with the
 * call's tsf_spec -- prophet_copy keeps the seasonalities of the full-history model; its scales and changepoints come
 * from the shorter history -- and predicts the rows in (cutoff_c, cutoff_c + horizon] with their own extra columns and
 * the series' floor / cap.  Since ds is sorted, those are rows [hist_rows, hist_rows + hold_rows) of the series.
 *
 * Optimiser: spec->algorithm = TSF_ALGO_AUTO is fbprophet's rule PER FOLD -- Newton for a fold history of fewer than
 * TSF_NEWTON_BELOW_T rows, L-BFGS otherwise, and Newton once more for a fold whose L-BFGS fit ended in TSF_ST_LSFAIL,
 * TSF_ST_INIT_NONFINITE or TSF_ST_EVAL_LIMIT (models of at most TSF_MAX_P parameters; wider models stay on L-BFGS).
 * TSF_ALGO_LBFGS / TSF_ALGO_NEWTON run every fold on that optimiser and retry nothing.  A fold's fit outputs are those
 * of tsf_fit_ragged on the explicitly cut prefix panel, bit for bit.
 *
 * Intervals (n_samples > 0): tsf_predict_intervals with series_key of fold c of series n =
 *   (int64_t)((uint64_t)key_n * 0x9E3779B97F4A7C15 + (uint64_t)c),   key_n = series_key[n] (NULL: n)
 * -- independent of how series are batched; passing that key to tsf_predict_intervals reproduces the fold's interval.
 *
 * Metrics, per series over all its holdout rows (n of them), horizon = ds - cutoff:
 *   w = clamp((int64_t)(rolling_window * n), 1, n); rows are grouped by distinct horizon into sums and counts, and
 *   every distinct horizon h whose cumulative count (horizons ascending) reaches w gets one metric row: the mean over
 *   the w rows of the window ending with h's group, the leftmost group of the window weighted partially (Prophet's
 *   rolling_mean_by_h).  mse, rmse = sqrt(windowed mse), mae, mape (NaN for the whole series if min |y| < 1e-8),
 *   coverage (fraction of rows with lower <= y <= upper; only with intervals).
 *   DELIBERATE DEVIATION: fbprophet 0.5 itself takes a row-wise rolling mean of w rows after an unstable sort by
 *   horizon, so on an aligned panel (C rows at every horizon) its result depends on how those ties happen to be
 *   ordered; the grouped form here does not.  The metric row count depends on the timestamps only (tsf_cv_plan).
 *
 * tsf_cv_plan (host only, no tsf_ctx, no device): aligned input (offsets NULL, ds [T], T >= 1) or ragged (T = 0,
 * offsets [N+1], ds [offsets[N]]).  Fills per series n_folds / status (TSF_CV_*) / n_holdout (holdout rows over all
 * folds) / n_metric (metric rows); cutoff / hist_rows / hold_rows are per fold, series by series (fold c of series n
 * at index sum(n_folds[0 .. n)) + c), and may be NULL -- call once without them to size them.  Returns 0, -1 bad
 * arguments.  args->period_ns <= 0 = horizon / 2, args->initial_ns < 0 = 3 * horizon (fbprophet's defaults);
 * horizon_ns > 0, rolling_window in [0, 1] (performance_metrics' default 0.1).
 *
 * tsf_cross_validate: the whole cross-validation on this context's GPU; input as tsf_fit_aligned (T > 0, offsets
 * NULL, y [N][T], extra [n_extra][T]) or tsf_fit_ragged (T = 0, offsets [N+1]); floor / cap [N] as there.  Outputs
 * (host pointers, sized from tsf_cv_plan: F = sum n_folds, R = sum n_holdout, M = sum n_metric):
 *   fit                 every member [F] (grid [F]), folds in plan order
 *   yhat                [R] holdout rows fold by fold; yhat_lower / yhat_upper [R] with intervals, else unused
 *   horizon_ns .. mape  [M] metric rows series by series, horizons ascending; coverage [M] with intervals
 *   series_status       [N] TSF_CV_* of the plan, or TSF_CV_FIT_FAILED if a fold's final fit status is < 0 (its
 *                       metric rows are then NaN)
 * Pending cost hints (tsf_set_cost_hints) are discarded.  Returns 0, < 0 as every entry point.
 * Reference interface replaced: none (the reference's jobs never cross-validate). */
enum {
    TSF_CV_OK = 0,
    TSF_CV_LESS_THAN_HORIZON = -20,   /* max(ds) - horizon < min(ds) ("Less data than horizon.") */
    TSF_CV_NO_CUTOFF = -21,           /* no cutoff after the initial window */
    TSF_CV_TOO_FEW = -22,             /* fewer than 2 rows before a cutoff */
    TSF_CV_FIT_FAILED = -23           /* a fold's fit failed (status < 0): Prophet would raise */
};
typedef struct {
    int64_t horizon_ns;
    int64_t period_ns;          /* <= 0: horizon / 2 */
    int64_t initial_ns;         /* < 0: 3 * horizon */
    double rolling_window;      /* 0.1 */
} tsf_cv_args;
typedef struct {
    tsf_fit_out fit;
    double *yhat, *yhat_lower, *yhat_upper;
    int64_t *horizon_ns;
    double *mse, *rmse, *mae, *mape, *coverage;
    int32_t *series_status;
} tsf_cv_out;
int tsf_cv_plan(int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds, const tsf_cv_args *args,
                int32_t *n_folds, int32_t *status, int64_t *n_holdout, int64_t *n_metric, int64_t *cutoff,
                int32_t *hist_rows, int32_t *hold_rows);
int tsf_cross_validate(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets,
                       const int64_t *ds, const void *y, int32_t y_dtype, const double *floor, const double *cap,
                       const double *extra, const tsf_cv_args *args, const int64_t *series_key, int32_t n_samples,
                       double interval_width, uint64_t seed, tsf_cv_out *out);

/* ---- prior-scale tuning by cross-validation ------------------------------------------------------
 * The documented Prophet recipe for choosing hyperparameters -- cross_validation for every combination of a grid of
 * prior scales, performance_metrics(..., rolling_window=1), keep the argmin -- for every series of a panel at once.
 * fbprophet 0.5 has no tuner of its own; parity with the real package is not pinned.
 *
 * Candidates: cand[0 .. C) are tsf_specs structurally identical to base; only changepoint_prior_scale,
 *   seas_prior_scale[0 .. n_seas) and extra_prior_scale[0 .. n_extra) may differ (every other field -- growth,
 *   changepoints, columns, modes, optimiser options, converge -- must be equal; the call rejects anything else before
 *   any launch).  So every candidate has one theta layout, one set of grids, one predict spec: the predict, interval
 *   and cross-validation kernels read no prior scale.  1 <= C <= TSF_TUNE_MAX_CAND; every prior scale of base and of
 *   the candidates finite and > 0.
 * Score: score[n][c] = the cross-validation metric of series n under candidate c over all its holdout rows -- the single
 *   metric row tsf_cross_validate returns with rolling_window = 1 (w = n rows), bit for bit.  metric: TSF_TUNE_MSE ..
 *   TSF_TUNE_MAPE.  Cutoffs from cv->horizon_ns / period_ns / initial_ns exactly as there; cv->rolling_window is
 *   ignored; no intervals.  The folds' optimiser (including algorithm = TSF_ALGO_AUTO's rule and Newton retry per fold)
 *   is tsf_cross_validate's, with the candidate's spec.
 * cand_status[n][c]: TSF_CV_* as tsf_cross_validate's series_status under candidate c: the plan's status (then a NaN
 *   score), TSF_CV_FIT_FAILED (a fold's fit failed: NaN score), or TSF_CV_OK.
 * Choice: best[n] = the lowest c among the candidates with a finite score that attain the minimum (np.nanargmin's
 *   first minimum).  series_status[n]: the plan's status where it is not TSF_CV_OK (best -1); TSF_TUNE_NO_SCORE where
 *   no candidate has a finite score (e.g. mape with min |y| < 1e-8, or every candidate's fold fit failed; best -1);
 *   else TSF_CV_OK.
 * Refit (refit = 1): each series fitted on its full history with cand[best[n]], or with base where best[n] = -1; out->fit
 *   as tsf_fit_aligned (aligned input: grid [1]) or tsf_fit_ragged (ragged: grid [N]) would return it for that series.
 *   algorithm = TSF_ALGO_AUTO applies fbprophet's rule PER SERIES as cross-validation applies it per fold: Newton below
 *   TSF_NEWTON_BELOW_T rows, L-BFGS otherwise, Newton once more after TSF_ST_LSFAIL / TSF_ST_INIT_NONFINITE /
 *   TSF_ST_EVAL_LIMIT (models of at most TSF_MAX_P parameters).  refit = 0: out->fit is not touched.
 * Input as tsf_cross_validate (host pointers; T > 0 aligned, T = 0 with offsets [N+1] ragged).  Outputs (host):
 *   score / cand_status [N][C], best / series_status [N], fit (refit = 1) [N].  Pending cost hints are discarded.
 * Work shared by the candidates: the panel crosses to the device once, the plan, the holdout panel, the fold panel of
 * each optimiser group (cv_expand_kernel) and its calendar classes are made once; per candidate one fit launch per
 * optimiser group (plus its own Newton retry group), one predict over every fold and one metrics pass.
 * Reference interface replaced: none. */
#define TSF_TUNE_MAX_CAND 256
enum { TSF_TUNE_MSE = 0, TSF_TUNE_RMSE = 1, TSF_TUNE_MAE = 2, TSF_TUNE_MAPE = 3 };
enum { TSF_TUNE_NO_SCORE = -24 };     /* series_status: no candidate has a finite score */
typedef struct {
    double *score;              /* [N][C] */
    int32_t *cand_status;       /* [N][C] */
    int32_t *best;              /* [N] */
    int32_t *series_status;     /* [N] */
    tsf_fit_out fit;            /* refit: [N], grid [1] aligned / [N] ragged */
} tsf_tune_out;
int tsf_tune(tsf_ctx *ctx, const tsf_spec *base, const tsf_spec *cand, int32_t C, int64_t N, int32_t T,
             const int64_t *offsets, const int64_t *ds, const void *y, int32_t y_dtype, const double *floor,
             const double *cap, const double *extra, const tsf_cv_args *cv, int32_t metric, int32_t refit,
             tsf_tune_out *out);

/* ---- model-structure selection by cross-validation ---------------------------------------------
 * tsf_tune's recipe over candidates that differ in STRUCTURE: Prophet's documented hyperparameter search lists
 * seasonality_mode among the parameters to tune and changepoint_range as worth trying, and a panel raises the same
 * question for growth, the number of changepoints and the seasonality set.  One call scores every candidate for every
 * series, chooses per series, and refits each series with its choice.  tsf_tune and its contract are unchanged.
 *
 * Candidates: cand[0 .. C), 1 <= C <= TSF_TUNE_MAX_CAND; there is no base spec.  They may differ in growth,
 *   n_changepoints, changepoint_range, changepoints_specified and the dates, the whole seasonality set (n_seas, periods,
 *   orders, modes, prior scales), extra_mode, extra_prior_scale and changepoint_prior_scale.  They must agree in n_extra
 *   (the call has one `extra` array, and its columns are every candidate's) and in every optimiser field (max_iter,
 *   history, init_alpha, tol_*, eval_form, recenter_*, algorithm, residual_kernel, coop_after, converge, map_max_iter,
 *   map_tol).  A logistic candidate without cap is refused, as is a prior scale that is not finite and > 0 and any spec
 *   a fit call would refuse.  Every refusal happens before any launch and leaves the context usable.
 * Score: score[n][c] / cand_status[n][c] = what tsf_cross_validate returns for cand[c] with rolling_window = 1 on the
 *   same panel, floor, cap, extra and cutoffs -- the single metric row and the series status, bit for bit (NaN where the
 *   series has no metric row).  metric: TSF_TUNE_MSE .. TSF_TUNE_MAPE; cv->rolling_window is ignored; no intervals.  The
 *   plan reads no spec field and is made once; a candidate with specified changepoints keeps per fold the leading
 *   dates <= the cutoff, its own table.
 * Choice: m = the least finite score of the row; best[n] = the lowest c with a finite score and
 *   score[n][c] <= m * (1.0 + tolerance) -- one add, one multiply, no fused multiply-add.  tolerance finite and >= 0;
 *   tolerance = 0 is tsf_tune's first-minimum rule exactly.  Order the candidates from simple to complex and the choice
 *   is the simplest one within the tolerance of the best: a model does not win on selection noise.  series_status[n]
 *   as tsf_tune's: the plan's status where it is not TSF_CV_OK (best -1), TSF_TUNE_NO_SCORE where no candidate has a
 *   finite score (best -1), else TSF_CV_OK.  chosen[n] = best[n], or `fallback` (in [0, C)) where best[n] is -1: the
 *   candidate the refit uses.
 * Refit (refit = 1): every series fitted on its whole history with cand[chosen[n]], the optimiser rule applied per
 *   series as in tsf_tune's refit.  The series' row of every fit output is what tsf_fit_aligned / tsf_fit_ragged gives
 *   for that series with that spec, bit for bit.  theta rows have stride_max = tsf_select_stride(cand, C) doubles: the
 *   first tsf_theta_stride(&cand[chosen[n]]) are the fit's, the rest +0.0.  grid, aligned panel: [C], grid[c] candidate
 *   c's grid where at least one series with rows was refitted with it, all zero bytes otherwise; ragged panel: [N].  A
 *   series without rows is left as tsf_tune's refit leaves it (status TSF_ST_TOO_FEW, everything else zero).
 *   refit = 0: out->fit is not touched.
 * Work shared by the candidates: the panel crosses to the device once; the holdout rows and the metric tables are made
 *   once; the fold panel of each optimiser group is cut once per distinct grouping of the folds (with equal algorithm
 *   the grouping differs only between candidates Newton takes, at most TSF_MAX_P parameters, and those it does not;
 *   candidates with specified changepoints share a panel where they carry the same dates); the fold fit
 *   outputs are allocated once at stride_max and read at each candidate's own stride.  tsf_last_tune_counts reports
 *   the call's fold panels and fit launches, as for tsf_tune.
 * Input as tsf_tune (host pointers).  Outputs (host): score / cand_status [N][C], best / chosen / series_status [N],
 *   fit (refit = 1).  Pending cost hints are discarded.  tsf_select_stride returns -1 for cand NULL, C < 1 or an n_seas
 *   out of range.  Timing: tools/bench_select.py; DESIGN.md 5r.
 * Reference interface replaced: none. */
typedef struct {
    double *score;            /* [N][C] */
    int32_t *cand_status;     /* [N][C] */
    int32_t *best;            /* [N]  the rule's choice, -1: none */
    int32_t *chosen;          /* [N]  best, or `fallback` where best is -1: the candidate the refit uses */
    int32_t *series_status;   /* [N]  as tsf_tune's */
    tsf_fit_out fit;          /* refit = 1: theta [N][stride_max], the others [N]; grid [C] aligned / [N] ragged */
} tsf_select_out;
int tsf_select_out_size(void);
int tsf_select_stride(const tsf_spec *cand, int32_t C);   /* stride_max = max over c of tsf_theta_stride(&cand[c]) */
int tsf_select(tsf_ctx *ctx, const tsf_spec *cand, int32_t C, int64_t N, int32_t T, const int64_t *offsets,
               const int64_t *ds, const void *y, int32_t y_dtype, const double *floor, const double *cap,
               const double *extra, const tsf_cv_args *cv, int32_t metric, double tolerance, int32_t fallback,
               int32_t refit, tsf_select_out *out);

/* ---- outlier screening: robust residual flags and refit ------------------------------------------------
 * One bad row -- a double-counted day, an outage, a unit mix-up -- bends the trend and the seasonality of its whole
 * series, and Prophet's documented remedy is to remove the rows and fit again.  tsf_screen_rows is that decision for
 * every series of a panel at once, as a pure function of (y, fitted, excluded) per series; tsf_fit_screened is the whole
 * remedy in one call: fit, screen, cut, fit again.  Everything here is opt-in: no other entry point changes.
 * Reference interface replaced: none (neither the reference nor fbprophet has such a function); parity unpinned (what is
 * pinned is the contract below, bit for bit against a numpy restatement, and tsf_fit_screened against the composition of
 * the public calls).  Timing: tools/bench_screen.py; DESIGN.md 5h.
 *
 * tsf_screen_rows.  Panel: aligned (offsets NULL: y, fitted, excluded, flag, resid are [N][T]) or ragged (T ignored;
 * series n owns rows [offsets[n], offsets[n + 1]) of each).  y in y_dtype; fitted double; excluded uint8 (non-zero = the
 * row was removed earlier and takes no part) or NULL; min_scale [N] (a floor under the robust scale) or NULL = 0.
 * Host pointers in the host variant; device pointers in _dev (args and the tsf_screen_out struct itself are HOST memory
 * in both; _dev on a ragged panel reads offsets back and synchronises the stream).
 *
 * Contract per series.  m0 = its row count; L = its rows with excluded == 0, m = |L|; x = m0 - m.  In plain double
 * operations, one rounding each:
 *   r_i = (double)y_i - fitted_i for every row;  a = {r_i : i in L} sorted ascending;
 *   center = 0.5 * (a[(m-1)/2] + a[m/2]);  d_i = fabs(r_i - center);  b = {d_i : i in L} sorted ascending;
 *   mad = 0.5 * (b[(m-1)/2] + b[m/2]);  scale = fmax(1.4826 * mad, min_scale[n]);
 *   B = (int64)floor(max_share * (double)m0) - x  (the budget: at most a share max_share of the series' rows is ever
 *   flagged, earlier exclusions included);  B <= 0: no new flag;  otherwise
 *   cut = fmax(threshold * scale, b[m-1-B]),  and row i of L is flagged iff d_i > cut.
 *   The comparison is strict, so at most B rows are flagged and ties at the budget's boundary flag nothing.  Sorting
 *   moves values and rounds nothing: every output is a function of the series' multiset of residuals alone.
 *   flag_i = (excluded_i != 0) | new_i;  resid_i = r_i (every row);  n_new = the new flags, n_flagged = all flags.
 *   status[n]: TSF_SCREEN_OK, or -- each of these leaves flag = excluded, n_new = 0, center = scale = NaN (resid is
 *   still written), the first that applies -- TSF_SCREEN_TOO_LONG (m0 > TSF_SCREEN_MAX_ROWS), TSF_SCREEN_TOO_FEW
 *   (m < min_rows), TSF_SCREEN_NONFINITE (a non-finite r_i on a row of L: a NaN in fitted flags nothing).
 *   No atomics; a series' results depend neither on the rest of the batch nor on how the call is cut into launches.
 * Refusals (< 0 with a message, before any launch; the context stays usable): a NULL out, out->flag, out->status, y or
 *   fitted; threshold not finite or not > 0; max_share outside [0, 0.5]; min_rows < 2; max_passes outside [1, 8] (read by
 *   tsf_fit_screened only, checked by both); a bad y_dtype; a bad panel.  N == 0 is a legal no-op.
 *
 * tsf_fit_screened.  Input as tsf_cross_validate (host pointers; T > 0 aligned, T = 0 with offsets [N+1] ragged); the
 * panel crosses to the device once.
 *   Round 0: every series fitted on its full history as tsf_tune's refit fits base: with algorithm TSF_ALGO_LBFGS /
 *   TSF_ALGO_NEWTON tsf_fit_aligned / tsf_fit_ragged bit for bit, with TSF_ALGO_AUTO fbprophet's rule PER SERIES with
 *   the Newton retry (see tsf_tune).  out->first, where given, receives it (grid [1] aligned / [N] ragged).
 *   Round p = 1 .. max_passes: fitted = tsf_predict of each series' current fit on its own history dates, every row,
 *   the excluded ones too (aligned: shared_future = 1 over ds [T]; ragged: shared_future = 0 over [N][Tmax], Tmax = the
 *   longest series, rows past a series' last repeating its last date); tsf_screen_rows with excluded = the flags so far
 *   and min_scale[n] = scale_floor_rel * y_scale[n] of the current fit (fitted is NaN for a series whose current fit
 *   failed: it is reported TSF_SCREEN_NONFINITE or TSF_SCREEN_TOO_FEW); the series with n_new > 0 are cut
 *   (screen_compact_kernel: the rows without a flag, in order) into ragged panels and fitted again, the optimiser by the
 *   same rule on the KEPT row count.  A series with n_new == 0 is finished and is not screened again; the loop ends when
 *   no series has new flags or after max_passes rounds, the last round's flagged series fitted again too: no final fit
 *   has seen a flagged row.
 *   out->fit [N], grid [N] always: a never-flagged series has its first fit bit for bit (aligned: a copy of the one
 *   grid); a flagged series has what tsf_fit_ragged returns on the explicitly cut panel, bit for bit, a failed refit's
 *   status included.  out->screen: flag and n_flagged cumulative; resid, center, scale, status, n_new those of the last
 *   round in which the series was screened.  rounds[n] = the rounds that gave series n new flags.
 *   Pending cost hints are discarded.  scale_floor_rel finite and >= 0. */
#define TSF_SCREEN_MAX_ROWS 16384
enum { TSF_SCREEN_OK = 0, TSF_SCREEN_TOO_FEW = -30, TSF_SCREEN_TOO_LONG = -31, TSF_SCREEN_NONFINITE = -32 };
typedef struct {
    double threshold, max_share;
    int32_t min_rows, max_passes;
} tsf_screen_args;
typedef struct {
    uint8_t *flag;          /* [rows]  required: 1 = excluded on input or flagged now */
    double *resid;          /* [rows]  NULL: not wanted (all below but status likewise) */
    double *center, *scale; /* [N] */
    int32_t *n_new, *n_flagged;     /* [N] */
    int32_t *status;        /* [N]     required */
} tsf_screen_out;
typedef struct {
    tsf_fit_out fit;        /* [N], grid [N] always */
    tsf_fit_out *first;     /* NULL: not wanted; the first fit, grid [1] aligned / [N] ragged */
    tsf_screen_out screen;
    int32_t *rounds;        /* [N] or NULL */
} tsf_fit_screened_out;
int tsf_screen_args_size(void);     /* sizeof(tsf_screen_args), sizeof(tsf_screen_out): the self-checks of a binding */
int tsf_screen_out_size(void);
int tsf_fit_screened_out_size(void);
int tsf_screen_rows(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets /* NULL = aligned [N][T] */, const void *y,
                    int32_t y_dtype, const double *fitted, const uint8_t *excluded, const double *min_scale,
                    const tsf_screen_args *args, tsf_screen_out *out);
int tsf_screen_rows_dev(tsf_ctx *ctx, int64_t N, int32_t T, const int64_t *offsets, const void *y, int32_t y_dtype,
                        const double *fitted, const uint8_t *excluded, const double *min_scale,
                        const tsf_screen_args *args, tsf_screen_out *out, void *stream);
int tsf_fit_screened(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds,
                     const void *y, int32_t y_dtype, const double *floor, const double *cap, const double *extra,
                     double scale_floor_rel, const tsf_screen_args *args, tsf_fit_screened_out *out);

/* ---- conformal interval calibration from cross-validation residuals ------------------------------------
 * Prophet's intervals carry trend and observation noise only, so on real panels the coverage tsf_cross_validate reports
 * comes back off interval_width.  Split-conformal calibration is the standard remedy: per series and per horizon bucket,
 * the finite-sample-corrected empirical quantile of a conformity score over the cross-validation's out-of-sample rows,
 * by which the forecast's interval is then widened or narrowed.  tsf_calibrate_rows is that rule for a whole panel at
 * once, as a pure function of each series' multiset of (bucket, score); tsf_apply_calibration applies a table to a
 * forecast; tsf_calibrate is cross-validation and rule in one call.  Everything here is opt-in: no other entry point
 * changes.  Reference interface replaced: none (neither the reference nor fbprophet has such a function); parity
 * unpinned (what is pinned is the contract below, bit for bit against a numpy restatement, and tsf_calibrate against the
 * composition of the public calls).  Timing: tools/bench_calibrate.py; DESIGN.md 5i.
 * Coverage after calibration is MARGINAL (over series' rows, not conditional on a date) and rests on the folds' errors
 * being exchangeable with the forecast's own: DESIGN.md 5i.
 *
 * tsf_calibrate_rows.  A ragged set of holdout rows: series n owns rows [row_off[n], row_off[n + 1]) of horizon_ns
 * (int64: ds - cutoff), y, yhat (double) [R], R = row_off[N]; lower / upper [L][R] (level l's bounds at l * R; read under
 * TSF_CALIB_CQR only, NULL otherwise).  Host pointers in the host variant; device pointers in _dev (args and the
 * tsf_calib_table struct itself are HOST memory in both; _dev reads row_off back and synchronises the stream).
 * tsf_calib_args: mode; n_levels L in [1, TSF_CALIB_MAX_LEVELS]; levels[l] strictly inside (0, 1), the coverage
 * targets; horizon_ns > 0; n_buckets B in [1, TSF_CALIB_MAX_BUCKETS]; min_scores >= 1.
 *
 * Contract per series.  Integer arithmetic is int64; every double operation is rounded once, in the order written.
 *   w = (horizon_ns + B - 1) / B.  A row with horizon h is eligible iff 0 < h <= horizon_ns; its bucket is
 *   min(B - 1, (h - 1) / w).  Its score at level l:
 *     TSF_CALIB_ABS: s = fabs(y - yhat), the same for every l; the row is live iff it is eligible and s is finite.
 *     TSF_CALIB_CQR: s = fmax(lower_l - y, y - upper_l); live iff eligible and y, lower_l, upper_l are all finite (the
 *       three operands are tested, not s: fmax drops a NaN).
 *   Cell (b, l), b < B, holds the live scores of bucket b; cell (B, l) all live scores of the series (the pooled cell).
 *   With m its count and a its scores ascending:  n[n][b][l] = m;  m < min_scores: q[n][b][l] = NaN;  otherwise
 *     k = (int64)ceil((double)(m + 1) * levels[l]),  q[n][b][l] = a[min(k, m) - 1] + 0.0
 *   (a product that rounds just above an integer takes the next rank: conservative; k > m takes the maximum; the + 0.0
 *   returns a zero as +0.0 whichever zero the sort left at the rank).  Sorting moves values and rounds nothing: the
 *   table depends on the series' multiset of (bucket, score) only -- not on the row order, the rest of the batch or how
 *   the call is cut into launches.  No atomics.
 *   status[n]: TSF_CALIB_TOO_LONG (more than TSF_CALIB_MAX_ROWS rows: every q NaN, every n 0); TSF_CALIB_NO_SCORES (the
 *   pooled cell of every level has m < min_scores); TSF_CALIB_OK otherwise.
 * Refusals (< 0 with a message, before any launch; the context stays usable): a NULL row_off, horizon_ns, y, yhat,
 *   args, table, table->q, table->n or table->status; a mode other than the two; n_levels, a level, n_buckets,
 *   min_scores or horizon_ns outside the ranges above; TSF_CALIB_CQR without lower and upper; row_off not ascending from
 *   0.  N == 0 is a legal no-op.
 *
 * tsf_apply_calibration.  yhat [N][H]; lower / upper [N][L][H] (read under TSF_CALIB_CQR only, NULL otherwise);
 * ds_future [H] (shared_future = 1) or [N][H] as in tsf_predict; origin_ns [N], the model's last history timestamp
 * (grid.start_ns + grid.t_scale_ns); q / n [N][B+1][L] and the tsf_calib_args that made them.  Per element (n, l, i):
 *   h = ds - origin;  b = h <= 0 ? 0 : min(B - 1, (h - 1) / w).  A row inside the history takes the first bucket and a
 *   row beyond the calibrated horizon the last one: both are EXTRAPOLATIONS of the table, no score was observed there.
 *   The cell used is b if n[b][l] >= min_scores, else the pooled cell B if n[B][l] >= min_scores, else none.
 *   ABS: lo = yhat - q, hi = yhat + q.  CQR: lo = fmin(lower_l - q, yhat), hi = fmax(upper_l + q, yhat) (a negative q
 *   narrows the interval, down to yhat at most).  No cell, or yhat not finite: lo = hi = NaN.
 * Outputs lo, hi [N][L][H]; cell int8 [N][L][H] (b, B or -1) or NULL.  _dev: device pointers (args in HOST memory).
 *
 * tsf_calibrate.  Input as tsf_cross_validate plus the tsf_calib_args; calib->horizon_ns must equal the
 * cross-validation's horizon.  The call runs tsf_cross_validate's own steps, forms each holdout row's horizon and
 * observed value on the device, and runs the rule on the device's yhat [R] with row_off = the series' holdout rows: the
 * table equals tsf_cross_validate followed by tsf_calibrate_rows on its outputs bit for bit, except that a series whose
 * series_status is not TSF_CV_OK gets no table (q NaN, n 0, TSF_CALIB_NO_SCORES).  cv_out, where not NULL, receives
 * what tsf_cross_validate returns, bit for bit.  TSF_CALIB_ABS needs no intervals (n_samples may be 0); TSF_CALIB_CQR is
 * accepted only with n_levels == 1, n_samples > 0 and levels[0] == interval_width, and reads the folds' own yhat_lower /
 * yhat_upper.  Only the [N]-sized table crosses back to the host where cv_out is NULL. */
#define TSF_CALIB_MAX_ROWS 16384
#define TSF_CALIB_MAX_LEVELS 16
#define TSF_CALIB_MAX_BUCKETS 64
enum { TSF_CALIB_ABS = 0, TSF_CALIB_CQR = 1 };
enum { TSF_CALIB_OK = 0, TSF_CALIB_NO_SCORES = -40, TSF_CALIB_TOO_LONG = -41 };
typedef struct {
    int32_t mode, n_levels;
    double levels[TSF_CALIB_MAX_LEVELS];
    int64_t horizon_ns;
    int32_t n_buckets, min_scores;
} tsf_calib_args;
typedef struct {
    double *q;              /* [N][B+1][L] required */
    int32_t *n;             /* [N][B+1][L] required */
    int32_t *status;        /* [N]         required */
} tsf_calib_table;
int tsf_calib_args_size(void);      /* sizeof(tsf_calib_args), sizeof(tsf_calib_table): the self-checks of a binding */
int tsf_calib_table_size(void);
int tsf_calibrate_rows(tsf_ctx *ctx, int64_t N, const int64_t *row_off, const int64_t *horizon_ns, const double *y,
                       const double *yhat, const double *lower, const double *upper, const tsf_calib_args *args,
                       tsf_calib_table *table);
int tsf_calibrate_rows_dev(tsf_ctx *ctx, int64_t N, const int64_t *row_off, const int64_t *horizon_ns, const double *y,
                           const double *yhat, const double *lower, const double *upper, const tsf_calib_args *args,
                           tsf_calib_table *table, void *stream);
int tsf_apply_calibration(tsf_ctx *ctx, int64_t N, int32_t H, const double *yhat, const double *lower, const double *upper,
                          const int64_t *ds_future, int32_t shared_future, const int64_t *origin_ns, const double *q,
                          const int32_t *n, const tsf_calib_args *args, double *lo, double *hi, int8_t *cell);
int tsf_apply_calibration_dev(tsf_ctx *ctx, int64_t N, int32_t H, const double *yhat, const double *lower,
                              const double *upper, const int64_t *ds_future, int32_t shared_future, const int64_t *origin_ns,
                              const double *q, const int32_t *n, const tsf_calib_args *args, double *lo, double *hi,
                              int8_t *cell, void *stream);
int tsf_calibrate(tsf_ctx *ctx, const tsf_spec *spec, int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds,
                  const void *y, int32_t y_dtype, const double *floor, const double *cap, const double *extra,
                  const tsf_cv_args *args, const int64_t *series_key, int32_t n_samples, double interval_width,
                  uint64_t seed, const tsf_calib_args *calib, tsf_calib_table *table, tsf_cv_out *cv_out);

/* ---- scheduling hints ---------------------------------------------------------------------
 * A launch ends with its longest fits (cfg2: 1 582 evaluations against a mean of 454), and nothing
 * cheap about a series predicts how long its fit takes -- except an earlier fit of the same
 * series: a job that re-fits its panel regularly (the reference's modeler is such a job) can hand
 * the evaluation counts of the previous run (tsf_fit_out.n_eval) to the next one.
 * tsf_set_cost_hints: cost[i] = expected relative cost of series i of the NEXT fit call on this
 * context (any fit entry point): consumed by it if it has exactly n series, discarded otherwise.  The work queue of that call hands the
 * series out in order of decreasing cost (ties: by index).  Results do not depend on the order
 * (every series is fitted by itself); only the launch time does: the BASELINE cfg2 panel with the
 * counts of its own previous fit takes 7.1-7.6 ms instead of 9.4.
 * cost: HOST pointer, copied by the call; NULL or n == 0 clears.  The hints are used once.
 * Reference interface replaced: none (Spark's scheduler knows nothing about a group's cost). */
int tsf_set_cost_hints(tsf_ctx *ctx, const int32_t *cost, int64_t n);

/* ---- host-side panel packing (no device work, no tsf_ctx) ---------------------------------
 * Regroups a long table (one row per observation) into the contiguous per-series runs
 * tsf_fit_ragged takes.  Replaces the row movement of
 *   df.groupby('series_id','dim_id').apply(...)   /root/reference/src/jobs/prophet_modeler.py:139-141
 * (Spark shuffle + one Arrow->pandas frame per group) and fbprophet's per-group
 * `history = df[df['y'].notnull()]`, sort by ds (Prophet.fit / setup_dataframe).
 * Order contract: series ascending by (series_id, dim_id); inside a series ascending ds with
 * ties in input order; rows whose y is NaN dropped; series left with no row dropped.
 *
 *   tsf_pack_rows   builds the plan.  The four input arrays are only read and must stay alive
 *                   until tsf_pack_fetch returns.  n_threads <= 0: one per core (max 32).
 *                   *identity = 1 when the input already is in packed order with no NaN
 *                   (then ds/y need not be copied at all).
 *   tsf_pack_fetch  fills caller-allocated outputs (any may be NULL): keys [n_series],
 *                   offsets [n_series+1], ds_out / y_out [n_rows], and per series
 *                   span = last ds - first ds, min_dt = smallest positive spacing (-1 if none),
 *                   y_max -- the inputs of fbprophet's set_auto_seasonalities and of
 *                   cap = max(y) * cap_multiplier (prophet_modeler.py:59-60).  span and every spacing are
 *                   differences of ascending int64 values, taken exactly and SATURATED at INT64_MAX (a series
 *                   that holds NaT = INT64_MIN beside a real date spans more than int64 holds; any series
 *                   without NaT and under 292 years long is unaffected).  y_max is the first of the largest
 *                   values.  ds_out may be the ds array given to tsf_pack_rows (in place).
 *   tsf_pack_flags  what tsf_pack_fetch's pass over the packed rows saw (valid after it): *aligned = 1 when every
 *                   series is observed on the first series' timestamp vector (one shared calendar: the panel can go
 *                   to tsf_fit_aligned as [n_series][T] without another look at ds); *has_inf = 1 when a y is
 *                   infinite (fbprophet raises "Found infinity in column y."); *integral = 1 when every y is an
 *                   integer that fits int32 -- the quantity column of the reference's schema
 *                   (prophet_modeler.py:16), which may then cross to the device as TSF_Y_I32; *has_nat = 1 when a ds
 *                   is INT64_MIN, pandas' NaT (fbprophet raises "Found NaN in column ds.").
 *   tsf_pack_rows_typed  the same plan for columns in the caller's own types: keys of key_bytes = 4 (the reference's
 *                   int32 series_id / dim_id, prophet_modeler.py:13-14) or 8, y of y_dtype TSF_Y_* (int32 = the
 *                   reference's quantity: no NaN possible).  A table already in packed order is then used in place, in
 *                   those types (tsf_pack_fetch writes ds_out / y_out -- always int64 / float64 -- only when asked).
 * Returns 0, -1 bad arguments, -2 out of memory, -3 other failure. */
typedef struct tsf_pack tsf_pack;
int tsf_pack_rows(int64_t n, const int64_t *series_id, const int64_t *dim_id, const int64_t *ds,
                  const double *y, int32_t n_threads, tsf_pack **out, int64_t *n_rows,
                  int64_t *n_series, int32_t *identity);
int tsf_pack_fetch(tsf_pack *p, int64_t *key_series_id, int64_t *key_dim_id, int64_t *offsets,
                   int64_t *ds_out, double *y_out, int64_t *span, int64_t *min_dt, double *y_max);
int tsf_pack_rows_typed(int64_t n, const void *series_id, const void *dim_id, int32_t key_bytes, const int64_t *ds,
                        const void *y, int32_t y_dtype, int32_t n_threads, tsf_pack **out, int64_t *n_rows,
                        int64_t *n_series, int32_t *identity);
int tsf_pack_flags(const tsf_pack *p, int32_t *aligned, int32_t *has_inf, int32_t *integral, int32_t *has_nat);
void tsf_pack_free(tsf_pack *p);

/* ---- model blobs (host side) ------------------------------------------------------------------
 * The `model` column of the fit UDF's output -- pickle.dumps(model) per series in the reference
 * (/root/reference/src/jobs/prophet_modeler.py:72-75) -- for a whole fitted batch at once: blob n is written at
 * out + n * stride, stride = prefix_len + 64 + 8 * (n_theta + n_tchange): the prefix (magic, version, the constructor
 * arguments: shared by the batch, built by the caller), then the little-endian record
 *   f64 y_scale | i64 start_ns, t_scale_ns, last_ds_ns | i32 T, S, i1, NT, status, n_iter, n_theta, n_tchange |
 *   f64 theta[n_theta] | f64 t_change[n_tchange]
 * theta [N][n_theta], y_scale / status / n_iter [N] and grid [n_grids] (1 or N) are a fit's outputs (tsf_fit_out);
 * last_ds [N] is the last history date of each series, null-y rows included (where make_future_dataframe starts,
 * prophet_scorer.py:64-66).  One contiguous buffer with equal strides is an Arrow binary column as it stands: the model
 * parquet (prophet_modeler.py:118-125) is written from it without a Python object per series.
 * Returns 0, -1 bad arguments, -2 out of memory. */
int tsf_model_blobs(int64_t N, const void *prefix, int32_t prefix_len, int32_t n_theta, const double *theta,
                    const double *y_scale, const tsf_grid_info *grid, int32_t n_grids, const int64_t *last_ds,
                    const int32_t *status, const int32_t *n_iter, int32_t n_tchange, void *out, int32_t n_threads);

/* ---- model-input reader (host side, no device work, no tsf_ctx) ---------------------------
 * Replaces ProphetModeler.read_input_dataframe's
 *   spark.read.csv(path, header=False, schema=MODEL_INPUT_SCHEMA)
 *   /root/reference/src/jobs/prophet_modeler.py:102-116 (schema :12-17)
 * for header-less CSV files, parsed in parallel straight into the columns tsf_pack_rows takes.
 *   layout      one letter per column of the FILES: 's' series_id, 'd' dim_id, 't' start_time,
 *               'q' quantity, 'x' ignored.  Hive-partitioned input (series_id=751/...csv) has
 *               layout "dtq" and the partition value in series_id[file].
 *   start_time  yyyy-MM-dd[( |T)HH:mm[:ss[.fffffffff]]][Z], taken as naive wall time
 *   quantity    integer (the reference's schema) or decimal; an empty field is a null and
 *               comes out as NaN (the packer drops it as fbprophet drops y.isnull() rows)
 *   rows come out in file order, files in the order given.
 *   The fine print (what tests/csv_ref.py restates):
 *   lines       end at '\n'; an unterminated last line counts.  Trailing '\r' and ' ' are cut off a line first; a
 *               line then empty is BLANK: skipped, not malformed, but it counts in line numbers.
 *   fields      split at ',' (quotes do not protect a comma); the layout's last column takes the rest of the line, so
 *               a line with MORE fields than the layout fails in that column unless it is 'x'.  Every converted
 *               field is first trimmed: blanks and tabs at both ends, '\r' at the end, then ONE pair of double
 *               quotes around what is left (nothing inside the quotes is trimmed again, except for quantity).
 *   integers    (series_id, dim_id) an optional '+' or '-' and 1 to 18 digits: a lone sign, an empty field and 19
 *               digits or more do not convert.
 *   start_time  exactly the pattern above: 4-digit year, 2-digit month / day / hour / minute / second, the fraction
 *               only after seconds, at least one digit; digits after the ninth are dropped (truncation).  The date
 *               must exist (proleptic Gregorian; Feb 29 in leap years only), hour <= 23 (no hour 24), minute and
 *               second <= 59.  A timestamp that int64 nanoseconds cannot hold -- outside
 *               1677-09-21T00:12:43.145224193 .. 2262-04-11T23:47:16.854775807; INT64_MIN is pandas' NaT and is
 *               never produced -- DOES NOT CONVERT (round 13: it used to wrap into a valid-looking value; pandas
 *               raises OutOfBoundsDatetime there; 0001-01-01 and 9999-12-31 are common sentinels).
 *   quantity    trimmed; empty (also `""`) = null = NaN; else an integer as above (trimmed once more) -> that value
 *               as a double; else whatever C's strtod takes IN FULL in the C locale (leading white space, decimal or
 *               hexadecimal floating literal, "nan") -- a NUL byte or anything else left over fails the field, and
 *               so does an infinite result ("inf", 1e999); underflow gives 0.
 *   A trailing '?' in layout ("dtq?") = Spark's default CSV mode PERMISSIVE: a line that does not
 *   match the schema (a field that does not convert, too few fields) is not an error.  Spark 2.4 turns
 *   it into a row of nulls (every column, dim_id included); a null y is dropped by the fit, and a null
 *   key cannot be expressed in the int64 columns here, so the record is DROPPED by the reader and
 *   counted (tsf_csv_malformed) -- never emitted under a made-up key.  Without the '?' the first such
 *   line fails the read (FAILFAST).
 * Returns 0; TSF_CSV_E_OPEN / TSF_CSV_E_PARSE with *err_file (index into paths) and *err_line
 * (1-based) set; -1 bad arguments, -2 out of memory, -3 other failure. */
enum { TSF_CSV_E_OPEN = -10, TSF_CSV_E_PARSE = -11, TSF_CSV_E_CODEC = -12 };
typedef struct tsf_csv tsf_csv;
int tsf_csv_read(int32_t n_files, const char *const *paths, const int64_t *series_id,
                 const char *layout, int32_t n_threads, tsf_csv **out, int64_t *n_rows,
                 int32_t *err_file, int64_t *err_line);
int tsf_csv_fetch(tsf_csv *t, int64_t *series_id, int64_t *dim_id, int64_t *ds, double *y);
/* The table's own columns ([n_rows] each, valid until tsf_csv_free): a caller that can adopt foreign memory
 * (numpy can) saves the copy of tsf_csv_fetch. */
int tsf_csv_columns(tsf_csv *t, const int64_t **series_id, const int64_t **dim_id, const int64_t **ds,
                    const double **y);
int64_t tsf_csv_malformed(const tsf_csv *t);     /* records dropped in permissive mode */
void tsf_csv_free(tsf_csv *t);

/* ---- input discovery (host side) -----------------------------------------------------------
 * What spark.read.csv(path) lists under a directory (prophet_modeler.py:109-114): every regular file below
 * `root` whose name, and every directory's name on the way, does not start with '_' or '.' (_SUCCESS, .crc,
 * _temporary); a `series_id=<int>` directory supplies series_id for the files below it (Hive partition
 * discovery).  A root that is a regular file is that file alone.  The files come out partitioned ones first,
 * by partition value, then by path -- so that the reader's rows arrive grouped --: *n_partitioned of the
 * *n_files.  tsf_csv_dir_paths / _series_id can be handed to tsf_csv_read as they are (layout "dtq" for the
 * first n_partitioned, "sdtq" for the rest).
 * Returns 0, or with the handle still valid (free it) TSF_CSV_E_OPEN (a directory could not be read),
 * TSF_CSV_E_PARSE (a `series_id=` directory whose value is not an integer) or TSF_CSV_E_CODEC (a part in a
 * codec the reader does not inflate: .bz2 .snappy .lz4 .zst .xz; .gz and .deflate are read) with the offending
 * path in tsf_csv_dir_error_path; -1 bad arguments, -2 out of memory. */
typedef struct tsf_csv_dir tsf_csv_dir;
int tsf_csv_discover(const char *root, int32_t n_threads, tsf_csv_dir **out, int32_t *n_files,
                     int32_t *n_partitioned);
/* The walk and the read in one pass (round 4): tsf_csv_discover_load lists like tsf_csv_discover and the thread that
 * lists a directory reads its files straight away (no second pass over 10 000 paths: the 16 ms walk disappears under
 * the reads); tsf_csv_read_loaded(d, first, count, ...) is tsf_csv_read over files [first, first + count) of the
 * sorted list with the bytes already in memory (a range can be handed over once; err_file is relative to `first`).
 * Files in a codec the reader refuses are listed but not loaded (TSF_CSV_E_CODEC from the discover call). */
int tsf_csv_discover_load(const char *root, int32_t n_threads, tsf_csv_dir **out, int32_t *n_files,
                          int32_t *n_partitioned);
int tsf_csv_read_loaded(tsf_csv_dir *d, int32_t first, int32_t count, const char *layout, int32_t n_threads,
                        tsf_csv **out, int64_t *n_rows, int32_t *err_file, int64_t *err_line);
/* The input directory in chunks (round 6): tsf_csv_root_open lists the CHILDREN of `root` once (hidden names skipped;
 * `series_id=<int>` directories first, by value, then the rest by name); tsf_csv_root_load is tsf_csv_discover_load over
 * the subtrees of children [first, first + count) -- its handle goes to tsf_csv_read_loaded / tsf_csv_dir_* as usual.
 * A job reads, fits and persists such ranges as a pipeline (files of chunk k + 1 are read while chunk k is on the GPU).
 * *hive_only = 1 when every child is a `series_id=<int>` directory and no value occurs twice -- the layout the reference
 * reads (spark.read.csv over `series_id=751/...`, prophet_modeler.py:109-114): ranges of children then hold disjoint
 * series, so fitting range by range fits every series once, on all of its rows.  *nested = 1 from a load that met a
 * `series_id=` directory below another one with a different value (the same series could then sit in two ranges): read
 * the tree whole instead.  Returns as tsf_csv_discover; tsf_csv_root_open also TSF_CSV_E_OPEN if root cannot be listed. */
typedef struct tsf_csv_root tsf_csv_root;
int tsf_csv_root_open(const char *root, tsf_csv_root **out, int32_t *n_children, int32_t *hive_only);
int tsf_csv_root_load(tsf_csv_root *r, int32_t first, int32_t count, int32_t n_threads, tsf_csv_dir **out,
                      int32_t *n_files, int32_t *n_partitioned, int32_t *nested);
void tsf_csv_root_free(tsf_csv_root *r);
const char *const *tsf_csv_dir_paths(const tsf_csv_dir *d);
const int64_t *tsf_csv_dir_series_id(const tsf_csv_dir *d);
const char *tsf_csv_dir_error_path(const tsf_csv_dir *d);
void tsf_csv_dir_free(tsf_csv_dir *d);

/* ---- forecast sink (host side) -------------------------------------------------------------
 * ProphetScorer.convert_forecasts + write_forecasts in one pass
 * (/root/reference/src/jobs/prophet_scorer.py:130-150): a CSV with header
 *   created_timestamp,series_id,dim_id,forecast_date,forecast_timestamp,forecast_quantity
 * forecast_date = the date of ds as %Y-%m-%d (:107-108); forecast_timestamp in Spark 2.4's default
 * CSV timestampFormat yyyy-MM-dd'T'HH:mm:ss.SSSXXX with the wall time taken as UTC
 * (2002-12-28T22:00:00.000Z).  ds: int64 ns since the epoch.  Overwrites `path`.
 * Returns 0, TSF_CSV_E_OPEN if the file cannot be written, -1 bad arguments, -2 out of memory. */
int tsf_csv_write_forecasts(const char *path, const char *created_timestamp, int64_t n,
                            const int64_t *series_id, const int64_t *dim_id, const int64_t *ds,
                            const int64_t *quantity, int32_t n_threads);
/* the same sink for int32 id / quantity columns (what the scorer's forecast frame holds: no widening copies) */
int tsf_csv_write_forecasts_i32(const char *path, const char *created_timestamp, int64_t n,
                                const int32_t *series_id, const int32_t *dim_id, const int64_t *ds,
                                const int32_t *quantity, int32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif /* TSF_H */
