"""ctypes binding of libtsf_amd.so (C-ABI declared in include/tsf.h).

This is the only place Python touches the native library.  There is NO CPU fallback: if the
shared library is missing or no GPU is visible, the functions raise.
"""
import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TSF_LIB_PATH') or os.path.join(_HERE, 'libtsf_amd.so')   # override: A/B runs of two builds

MAX_SEAS = 8
TREE_MAX_LEVELS = 4         # TSF_TREE_MAX_LEVELS: levels above the groups of a roll-up's tree
MAX_EXTRA = 64
MAX_S = 60
MAX_K = 64
MAX_P = 128
MAX_COMP = 128
MAX_QUANT = 64
MAX_WINDOWS = 4096

GROWTH_LINEAR, GROWTH_LOGISTIC = 0, 1
MODE_ADDITIVE, MODE_MULTIPLICATIVE = 0, 1
Y_F64, Y_F32, Y_I32 = 0, 1, 2
EVAL_AUTO, EVAL_RESIDUAL, EVAL_QUADRATIC = 0, 1, 2
ALGO_LBFGS, ALGO_NEWTON, ALGO_AUTO = 0, 1, 2
RK_AUTO, RK_WAVE, RK_MFMA, RK_COOP = 0, 1, 2, 3
CONVERGE_STAN, CONVERGE_MAP = 0, 1

ST_ABSX, ST_ABSF, ST_RELF, ST_ABSGRAD, ST_RELGRAD, ST_MAXIT = 10, 20, 21, 30, 31, 40
ST_CONSTANT, ST_LSFAIL, ST_INIT_NONFINITE, ST_TOO_FEW, ST_CAP = 50, -1, -2, -10, -11
ST_EVAL_LIMIT = -3
ST_CHANGEPOINT = -12
ST_NEWTON_CONVERGED, ST_NEWTON_FAIL = 60, -4
ST_MAP_KKT, ST_MAP_FTOL, ST_MAP_MAXIT, ST_MAP_LS = 70, 71, 72, 73
STATUS_NAMES = {10: 'ABSX', 20: 'ABSF', 21: 'RELF', 30: 'ABSGRAD', 31: 'RELGRAD', 40: 'MAXIT',
                50: 'CONSTANT', -1: 'LSFAIL', -2: 'INIT_NONFINITE', -3: 'EVAL_LIMIT', -10: 'TOO_FEW',
                -11: 'CAP', -12: 'CHANGEPOINT', 60: 'NEWTON_CONVERGED', -4: 'NEWTON_FAIL', 70: 'MAP_KKT', 71: 'MAP_FTOL', 72: 'MAP_MAXIT',
                73: 'MAP_LS'}


class TsfSpec(ctypes.Structure):
    """tsf_spec (include/tsf.h)."""
    _fields_ = [('growth', ctypes.c_int32), ('n_changepoints', ctypes.c_int32),
                ('changepoint_range', ctypes.c_double),
                ('changepoint_prior_scale', ctypes.c_double),
                ('n_seas', ctypes.c_int32), ('n_extra', ctypes.c_int32),
                ('seas_period', ctypes.c_double * MAX_SEAS),
                ('seas_prior_scale', ctypes.c_double * MAX_SEAS),
                ('seas_order', ctypes.c_int32 * MAX_SEAS),
                ('seas_mode', ctypes.c_int32 * MAX_SEAS),
                ('extra_prior_scale', ctypes.c_double * MAX_EXTRA),
                ('extra_mode', ctypes.c_int32 * MAX_EXTRA),
                ('max_iter', ctypes.c_int32), ('history', ctypes.c_int32),
                ('init_alpha', ctypes.c_double), ('tol_obj', ctypes.c_double),
                ('tol_rel_obj', ctypes.c_double), ('tol_grad', ctypes.c_double),
                ('tol_rel_grad', ctypes.c_double), ('tol_param', ctypes.c_double),
                ('eval_form', ctypes.c_int32), ('recenter_every', ctypes.c_int32),
                ('recenter_ratio', ctypes.c_double),
                ('algorithm', ctypes.c_int32), ('residual_kernel', ctypes.c_int32),
                ('coop_after', ctypes.c_int32), ('converge', ctypes.c_int32), ('map_max_iter', ctypes.c_int32),
                ('map_tol', ctypes.c_double),
                ('changepoints_specified', ctypes.c_int32), ('changepoint_ns', ctypes.c_int64 * MAX_S)]


class TsfCvArgs(ctypes.Structure):
    """tsf_cv_args (include/tsf.h)."""
    _fields_ = [('horizon_ns', ctypes.c_int64), ('period_ns', ctypes.c_int64), ('initial_ns', ctypes.c_int64),
                ('rolling_window', ctypes.c_double)]


class TsfGridInfo(ctypes.Structure):
    """tsf_grid_info (include/tsf.h)."""
    _fields_ = [('start_ns', ctypes.c_int64), ('t_scale_ns', ctypes.c_int64),
                ('T', ctypes.c_int32), ('S', ctypes.c_int32), ('i1', ctypes.c_int32),
                ('NT', ctypes.c_int32), ('t_change', ctypes.c_double * (MAX_S + 4))]


GRID_DTYPE = np.dtype([('start_ns', '<i8'), ('t_scale_ns', '<i8'), ('T', '<i4'), ('S', '<i4'),
                       ('i1', '<i4'), ('NT', '<i4'), ('t_change', '<f8', (MAX_S + 4,))])


class TsfFitOut(ctypes.Structure):
    """tsf_fit_out (include/tsf.h)."""
    _fields_ = [('theta', ctypes.c_void_p), ('y_scale', ctypes.c_void_p),
                ('fval', ctypes.c_void_p), ('status', ctypes.c_void_p),
                ('n_iter', ctypes.c_void_p), ('n_eval', ctypes.c_void_p),
                ('grid', ctypes.c_void_p)]


class TsfCvOut(ctypes.Structure):
    """tsf_cv_out (include/tsf.h)."""
    _fields_ = [('fit', TsfFitOut), ('yhat', ctypes.c_void_p), ('yhat_lower', ctypes.c_void_p),
                ('yhat_upper', ctypes.c_void_p), ('horizon_ns', ctypes.c_void_p), ('mse', ctypes.c_void_p),
                ('rmse', ctypes.c_void_p), ('mae', ctypes.c_void_p), ('mape', ctypes.c_void_p),
                ('coverage', ctypes.c_void_p), ('series_status', ctypes.c_void_p)]


class TsfQuantileOut(ctypes.Structure):
    """tsf_quantile_out (include/tsf.h)."""
    _fields_ = [('yhat', ctypes.c_void_p), ('q', ctypes.c_void_p), ('cum_q', ctypes.c_void_p),
                ('trend_q', ctypes.c_void_p), ('samples', ctypes.c_void_p), ('trend_samples', ctypes.c_void_p)]


class TsfScoreOut(ctypes.Structure):
    """tsf_score_out (include/tsf.h)."""
    _fields_ = [('yhat', ctypes.c_void_p), ('pit', ctypes.c_void_p), ('crps', ctypes.c_void_p), ('q', ctypes.c_void_p),
                ('pinball', ctypes.c_void_p), ('n_obs', ctypes.c_void_p), ('mean_crps', ctypes.c_void_p),
                ('mean_pinball', ctypes.c_void_p), ('coverage', ctypes.c_void_p)]


class TsfRollupOut(ctypes.Structure):
    """tsf_rollup_out (include/tsf.h)."""
    _fields_ = [('yhat', ctypes.c_void_p), ('count', ctypes.c_void_p), ('q', ctypes.c_void_p), ('cum_q', ctypes.c_void_p),
                ('samples', ctypes.c_void_p)]


class TsfWindowOut(ctypes.Structure):
    """tsf_window_out (include/tsf.h)."""
    _fields_ = [('yhat', ctypes.c_void_p), ('total', ctypes.c_void_p), ('q', ctypes.c_void_p), ('pit', ctypes.c_void_p),
                ('crps', ctypes.c_void_p), ('pinball', ctypes.c_void_p), ('n_obs', ctypes.c_void_p),
                ('mean_crps', ctypes.c_void_p), ('mean_pinball', ctypes.c_void_p), ('coverage', ctypes.c_void_p)]


class TsfReconcileOut(ctypes.Structure):
    """tsf_reconcile_out (include/tsf.h)."""
    _fields_ = [('yhat', ctypes.c_void_p), ('q', ctypes.c_void_p), ('cum_q', ctypes.c_void_p), ('samples', ctypes.c_void_p)]


class TsfTemporalOut(ctypes.Structure):
    """tsf_temporal_out (include/tsf.h)."""
    _fields_ = [('yhat', ctypes.c_void_p), ('q', ctypes.c_void_p), ('cum_q', ctypes.c_void_p), ('total', ctypes.c_void_p),
                ('win_q', ctypes.c_void_p), ('samples', ctypes.c_void_p), ('win_samples', ctypes.c_void_p)]


class TsfTuneOut(ctypes.Structure):
    """tsf_tune_out (include/tsf.h)."""
    _fields_ = [('score', ctypes.c_void_p), ('cand_status', ctypes.c_void_p), ('best', ctypes.c_void_p),
                ('series_status', ctypes.c_void_p), ('fit', TsfFitOut)]


class TsfSelectOut(ctypes.Structure):
    """tsf_select_out (include/tsf.h)."""
    _fields_ = [('score', ctypes.c_void_p), ('cand_status', ctypes.c_void_p), ('best', ctypes.c_void_p),
                ('chosen', ctypes.c_void_p), ('series_status', ctypes.c_void_p), ('fit', TsfFitOut)]


class TsfScreenArgs(ctypes.Structure):
    """tsf_screen_args (include/tsf.h)."""
    _fields_ = [('threshold', ctypes.c_double), ('max_share', ctypes.c_double), ('min_rows', ctypes.c_int32),
                ('max_passes', ctypes.c_int32)]


class TsfScreenOut(ctypes.Structure):
    """tsf_screen_out (include/tsf.h)."""
    _fields_ = [('flag', ctypes.c_void_p), ('resid', ctypes.c_void_p), ('center', ctypes.c_void_p),
                ('scale', ctypes.c_void_p), ('n_new', ctypes.c_void_p), ('n_flagged', ctypes.c_void_p),
                ('status', ctypes.c_void_p)]


class TsfFitScreenedOut(ctypes.Structure):
    """tsf_fit_screened_out (include/tsf.h)."""
    _fields_ = [('fit', TsfFitOut), ('first', ctypes.POINTER(TsfFitOut)), ('screen', TsfScreenOut),
                ('rounds', ctypes.c_void_p)]


class TsfCalibArgs(ctypes.Structure):
    """tsf_calib_args (include/tsf.h)."""
    _fields_ = [('mode', ctypes.c_int32), ('n_levels', ctypes.c_int32), ('levels', ctypes.c_double * 16),
                ('horizon_ns', ctypes.c_int64), ('n_buckets', ctypes.c_int32), ('min_scores', ctypes.c_int32)]


class TsfCalibTable(ctypes.Structure):
    """tsf_calib_table (include/tsf.h)."""
    _fields_ = [('q', ctypes.c_void_p), ('n', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class TsfCorrArgs(ctypes.Structure):
    """tsf_corr_args (include/tsf.h)."""
    _fields_ = [('rho_max', ctypes.c_double), ('min_rows', ctypes.c_int32), ('reserved_', ctypes.c_int32)]


class TsfCorrOut(ctypes.Structure):
    """tsf_corr_out (include/tsf.h)."""
    _fields_ = [('rho', ctypes.c_void_p), ('rho_raw', ctypes.c_void_p), ('n_pairs', ctypes.c_void_p),
                ('n_used', ctypes.c_void_p), ('status', ctypes.c_void_p), ('scale', ctypes.c_void_p)]


class TsfArArgs(ctypes.Structure):
    """tsf_ar_args (include/tsf.h)."""
    _fields_ = [('phi_max', ctypes.c_double), ('min_pairs', ctypes.c_int32), ('reserved_', ctypes.c_int32)]


class TsfArOut(ctypes.Structure):
    """tsf_ar_out (include/tsf.h)."""
    _fields_ = [('phi', ctypes.c_void_p), ('phi_raw', ctypes.c_void_p), ('n_pairs', ctypes.c_void_p),
                ('scale', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class TsfArLastOut(ctypes.Structure):
    """tsf_ar_last_out (include/tsf.h)."""
    _fields_ = [('last_resid', ctypes.c_void_p), ('last_gap', ctypes.c_void_p), ('status', ctypes.c_void_p)]


class TsfNoiseStateOut(ctypes.Structure):
    """tsf_noise_state_out (include/tsf.h)."""
    _fields_ = [('phi', ctypes.c_void_p), ('phi_raw', ctypes.c_void_p), ('n_pairs', ctypes.c_void_p),
                ('scale', ctypes.c_void_p), ('status', ctypes.c_void_p), ('last_resid', ctypes.c_void_p),
                ('last_gap', ctypes.c_void_p), ('last_status', ctypes.c_void_p), ('last_ds_ns', ctypes.c_void_p)]


class TsfCondSeas(ctypes.Structure):
    """tsf_cond_seas (include/tsf.h)."""
    _fields_ = [('n', ctypes.c_int32), ('period', ctypes.c_double * MAX_SEAS), ('order', ctypes.c_int32 * MAX_SEAS),
                ('cond', ctypes.c_int32 * MAX_SEAS)]


class TsfFitShape(ctypes.Structure):
    """tsf_fit_shape (include/tsf_dev.h)."""
    _fields_ = [('N', ctypes.c_int64), ('n_distinct', ctypes.c_int64), ('lat_step', ctypes.c_int64), ('lat_U', ctypes.c_int64),
                ('aligned', ctypes.c_int32), ('Tm', ctypes.c_int32), ('call', ctypes.c_int32), ('classes', ctypes.c_int32)]


# tsf_fit_plan_info (include/tsf_dev.h), field by field; PLAN_FIELDS: what a plan says (all but the padding)
_PLAN_I64 = ['n_grids', 'lat_U', 'quad_pre']
_PLAN_I32 = ['err', 'route', 'NTmax', 'shared_grids', 'quad_P4', 'quad_PPL', 'quad_NW', 'quad_blocks', 'quad_slots',
             'quad_ragged', 'mfma_on', 'mfma_NG', 'mfma_KF', 'mfma_NCB', 'mfma_rr0', 'mfma_blocks', 'coop', 'coop_after',
             'coop_slots', 'coop_stride', 'sparse_try', 'harm', 'gram_harm', 'resid_harm', 'map_harm', 'bw_ns', 'raw_y']
PLAN_FIELDS = _PLAN_I64 + _PLAN_I32


class TsfFitPlanInfo(ctypes.Structure):
    """tsf_fit_plan_info (include/tsf_dev.h)."""
    _fields_ = ([(f, ctypes.c_int64) for f in _PLAN_I64] + [(f, ctypes.c_int32) for f in _PLAN_I32]
                + [('reserved_', ctypes.c_int32)])

    def as_dict(self):
        return {f: int(getattr(self, f)) for f in PLAN_FIELDS}


# every symbol include/tsf.h declares; tests check the library exports all of them
EXPORTS = ['tsf_create', 'tsf_destroy', 'tsf_last_error', 'tsf_device_count', 'tsf_spec_default',
           'tsf_spec_size', 'tsf_grid_info_size', 'tsf_spec_K', 'tsf_theta_stride',
           'tsf_fit_aligned', 'tsf_fit_aligned_dev', 'tsf_fit_ragged', 'tsf_fit_ragged_dev',
           'tsf_predict', 'tsf_predict_dev', 'tsf_predict_intervals', 'tsf_predict_intervals_dev', 'tsf_predict_components', 'tsf_predict_components_dev',
           'tsf_predict_quantiles', 'tsf_predict_quantiles_dev',
           'tsf_score_out_size', 'tsf_score_actuals', 'tsf_score_actuals_dev',
           'tsf_rollup_create', 'tsf_rollup_add', 'tsf_rollup_quantiles', 'tsf_rollup_free',
           'tsf_window_out_size', 'tsf_predict_windows', 'tsf_predict_windows_dev', 'tsf_rollup_windows',
           'tsf_reconcile_shares', 'tsf_reconcile_out_size', 'tsf_rollup_set_totals', 'tsf_rollup_reconcile', 'tsf_rollup_reconciled_totals',
           'tsf_reconcile_tree_shares', 'tsf_rollup_set_tree', 'tsf_rollup_set_node_totals', 'tsf_rollup_solve_tree',
           'tsf_rollup_reconcile_tree', 'tsf_rollup_tree_totals',
           'tsf_temporal_shares', 'tsf_temporal_out_size', 'tsf_predict_temporal',
           'tsf_corr_args_size', 'tsf_corr_out_size', 'tsf_residual_corr', 'tsf_residual_corr_dev', 'tsf_rollup_set_noise_corr',
           'tsf_ar_args_size', 'tsf_ar_out_size', 'tsf_residual_autocorr', 'tsf_residual_autocorr_dev', 'tsf_set_noise_ar',
           'tsf_ar_last_out_size', 'tsf_residual_last', 'tsf_residual_last_dev', 'tsf_residual_autocorr_last',
           'tsf_set_noise_ar_start', 'tsf_noise_ar_mean',
           'tsf_noise_state_out_size', 'tsf_noise_state', 'tsf_noise_state_dev', 'tsf_predict_conditioned',
           'tsf_predict_conditioned_dev',
           'tsf_cond_columns', 'tsf_cond_columns_dev',
           'tsf_eval', 'tsf_eval_quadratic', 'tsf_design', 'tsf_selftest_math',
           'tsf_set_option', 'tsf_get_option', 'tsf_set_cost_hints', 'tsf_set_profiling', 'tsf_profile_read', 'tsf_last_fit_kernel_ms', 'tsf_last_fit_route',
           'tsf_fit_plan', 'tsf_fit_plan_info_size', 'tsf_fit_plan_error', 'tsf_last_fit_plan',
           'tsf_cv_plan', 'tsf_cross_validate', 'tsf_last_cv_grids', 'tsf_tune', 'tsf_last_tune_counts',
           'tsf_select_out_size', 'tsf_select_stride', 'tsf_select',
           'tsf_screen_args_size', 'tsf_screen_out_size', 'tsf_fit_screened_out_size', 'tsf_screen_rows', 'tsf_screen_rows_dev',
           'tsf_fit_screened',
           'tsf_calib_args_size', 'tsf_calib_table_size', 'tsf_calibrate_rows', 'tsf_calibrate_rows_dev',
           'tsf_apply_calibration', 'tsf_apply_calibration_dev', 'tsf_calibrate',
           'tsf_pack_rows', 'tsf_pack_rows_typed', 'tsf_pack_fetch', 'tsf_pack_flags', 'tsf_pack_free', 'tsf_model_blobs',
           'tsf_csv_read', 'tsf_csv_fetch', 'tsf_csv_columns', 'tsf_csv_malformed', 'tsf_csv_free', 'tsf_csv_write_forecasts', 'tsf_csv_write_forecasts_i32',
           'tsf_csv_discover', 'tsf_csv_discover_load', 'tsf_csv_root_open', 'tsf_csv_root_load', 'tsf_csv_root_free', 'tsf_csv_read_loaded', 'tsf_csv_dir_paths', 'tsf_csv_dir_series_id', 'tsf_csv_dir_error_path', 'tsf_csv_dir_free']

CSV_E_OPEN, CSV_E_PARSE, CSV_E_CODEC = -10, -11, -12          # TSF_CSV_E_* (include/tsf.h)
# TSF_CV_* (include/tsf.h): per-series outcome of a cross-validation plan / call
CV_OK, CV_LESS_THAN_HORIZON, CV_NO_CUTOFF, CV_TOO_FEW, CV_FIT_FAILED = 0, -20, -21, -22, -23
# TSF_TUNE_* (include/tsf.h): tsf_tune's metrics, its series status where no candidate scored, its candidate limit
TUNE_MSE, TUNE_RMSE, TUNE_MAE, TUNE_MAPE = 0, 1, 2, 3
TUNE_METRICS = {'mse': TUNE_MSE, 'rmse': TUNE_RMSE, 'mae': TUNE_MAE, 'mape': TUNE_MAPE}
TUNE_NO_SCORE = -24
TUNE_MAX_CAND = 256
# TSF_SCREEN_* (include/tsf.h): per-series outcome of the screening rule, its row limit
SCREEN_OK, SCREEN_TOO_FEW, SCREEN_TOO_LONG, SCREEN_NONFINITE = 0, -30, -31, -32
SCREEN_MAX_ROWS = 16384
# TSF_CALIB_* (include/tsf.h): the conformity scores, the per-series outcome of the calibration rule, its limits
CALIB_ABS, CALIB_CQR = 0, 1
CALIB_MODES = {'abs': CALIB_ABS, 'cqr': CALIB_CQR}
CALIB_OK, CALIB_NO_SCORES, CALIB_TOO_LONG = 0, -40, -41
CALIB_MAX_ROWS, CALIB_MAX_LEVELS, CALIB_MAX_BUCKETS = 16384, 16, 64
# TSF_CORR_* (include/tsf.h): per-group outcome of the residual-correlation estimator
CORR_OK, CORR_NO_PAIRS = 0, -50
# TSF_AR_* (include/tsf.h): per-series outcome of the residual-autocorrelation estimator
AR_OK, AR_NO_PAIRS = 0, -51
AR_NO_ROW = -52                 # tsf_residual_last: a series without a present row

# TSF_ROUTE_* / TSF_CALL_* / TSF_PLAN_* (include/tsf_dev.h): a fit plan's route, the kind of call, why a call has no plan
ROUTE_NEWTON, ROUTE_NEWTON_QUAD, ROUTE_QUAD_EVAL, ROUTE_QUAD_LBFGS, ROUTE_MFMA, ROUTE_WAVE = range(6)
CALL_FIT, CALL_EVAL, CALL_EVAL_QUADRATIC = 0, 1, 2
(PLAN_OK, PLAN_NO_ROWS, PLAN_TOO_LONG, PLAN_NEWTON_WIDE, PLAN_QUAD_FORM, PLAN_QUAD_EVAL, PLAN_MFMA_CHANGEPOINTS, PLAN_MFMA_SHAPE,
 PLAN_COOP_SHAPE) = range(9)

# TSF_OPT_* (include/tsf.h): route switches of one context
OPTIONS = ['harm', 'lattice', 'sparse_extra', 'fit_grouped', 'gram_share', 'grid_order', 'grid_share', 'ragged_split',
           'quad_reg', 'quad_m2_lds', 'quad_w4', 'quad_rreg', 'newton_batch', 'newton_flags', 'newton_ns', 'newton_lcap',
           'newton_fill', 'quad_raw_y', 'debug_async_scratch', 'coop_tail', 'map_direct']

_lib = None


class TsfError(RuntimeError):
    pass


def load():
    """Load libtsf_amd.so (once).  Raises if it has not been built -- no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TsfError('libtsf_amd.so not built: run `python -m time_series_spark_amd.build` '
                       '(or __graft_entry__.build()).  There is no CPU fallback.')
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    psp = ctypes.POINTER(TsfSpec)
    L.tsf_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.tsf_destroy.argtypes = [vp]
    L.tsf_destroy.restype = None
    L.tsf_last_error.argtypes = [vp]
    L.tsf_last_error.restype = ctypes.c_char_p
    L.tsf_device_count.argtypes = []
    L.tsf_spec_default.argtypes = [psp]
    L.tsf_spec_default.restype = None
    L.tsf_spec_K.argtypes = [psp]
    L.tsf_theta_stride.argtypes = [psp]
    L.tsf_fit_aligned.argtypes = [vp, psp, i64, i32, vp, vp, i32, vp, vp, vp,
                                  ctypes.POINTER(TsfFitOut)]
    L.tsf_fit_aligned_dev.argtypes = [vp, psp, i64, i32, vp, vp, i32, vp, vp, vp,
                                      ctypes.POINTER(TsfFitOut), vp]
    L.tsf_fit_ragged.argtypes = [vp, psp, i64, vp, vp, vp, i32, vp, vp, vp,
                                 ctypes.POINTER(TsfFitOut)]
    L.tsf_fit_ragged_dev.argtypes = [vp, psp, i64, vp, i64, i32, vp, vp, i32, vp, vp, vp,
                                     ctypes.POINTER(TsfFitOut), vp]
    L.tsf_predict.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.tsf_predict_dev.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp,
                                  vp]
    f64, u64 = ctypes.c_double, ctypes.c_uint64
    L.tsf_predict_intervals.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, f64,
                                        u64, vp, vp, vp]
    L.tsf_predict_intervals_dev.argtypes = L.tsf_predict_intervals.argtypes + [vp]
    L.tsf_predict_components.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32,
                                         f64, u64, vp, vp, vp, vp, vp, vp, vp]
    L.tsf_predict_components_dev.argtypes = L.tsf_predict_components.argtypes + [vp]
    L.tsf_predict_quantiles.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, u64, i32, vp,
                                        ctypes.POINTER(TsfQuantileOut)]
    L.tsf_predict_quantiles_dev.argtypes = L.tsf_predict_quantiles.argtypes + [vp]
    L.tsf_score_actuals.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, u64, vp, i32, vp,
                                    ctypes.POINTER(TsfScoreOut)]
    L.tsf_score_actuals_dev.argtypes = L.tsf_score_actuals.argtypes + [vp]
    L.tsf_rollup_create.argtypes = [vp, i64, i32, vp, i32, u64, ctypes.POINTER(vp)]
    L.tsf_rollup_add.argtypes = [vp, psp, i64, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp]
    L.tsf_rollup_quantiles.argtypes = [vp, i32, vp, ctypes.POINTER(TsfRollupOut)]
    L.tsf_rollup_free.argtypes = [vp]
    L.tsf_rollup_free.restype = None
    L.tsf_predict_windows.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, u64, i32, vp, vp, vp,
                                      i32, vp, ctypes.POINTER(TsfWindowOut)]
    L.tsf_predict_windows_dev.argtypes = L.tsf_predict_windows.argtypes + [vp]
    L.tsf_rollup_windows.argtypes = [vp, i32, vp, vp, vp, i32, vp, ctypes.POINTER(TsfWindowOut)]
    L.tsf_reconcile_shares.argtypes = [i64, vp, vp, i64, vp, vp, vp]
    L.tsf_rollup_set_totals.argtypes = L.tsf_rollup_add.argtypes
    L.tsf_rollup_reconcile.argtypes = L.tsf_rollup_add.argtypes + [vp, i32, vp, ctypes.POINTER(TsfReconcileOut)]
    L.tsf_rollup_reconciled_totals.argtypes = [vp, vp, i32, vp, ctypes.POINTER(TsfRollupOut)]
    L.tsf_reconcile_tree_shares.argtypes = [i64, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tsf_rollup_set_tree.argtypes = [vp, i32, vp, vp]
    L.tsf_rollup_set_node_totals.argtypes = [vp, i32] + L.tsf_rollup_add.argtypes[1:]
    L.tsf_rollup_solve_tree.argtypes = [vp, vp, vp]
    L.tsf_rollup_reconcile_tree.argtypes = L.tsf_rollup_reconcile.argtypes
    L.tsf_rollup_tree_totals.argtypes = [vp, i32, i64, i64, i32, vp, ctypes.POINTER(TsfRollupOut)]
    L.tsf_temporal_shares.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp]
    model = [psp, i64, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]        # (the period model's: K without N)
    L.tsf_predict_temporal.argtypes = [vp] + model + model[:1] + model[2:] + [i32, u64, vp, vp, vp, vp, i32, vp,
                                                                               ctypes.POINTER(TsfTemporalOut)]
    L.tsf_residual_corr.argtypes = [vp, i64, i32, vp, i32, vp, vp, i64, ctypes.POINTER(TsfCorrArgs), ctypes.POINTER(TsfCorrOut)]
    L.tsf_residual_corr_dev.argtypes = L.tsf_residual_corr.argtypes + [vp]
    L.tsf_rollup_set_noise_corr.argtypes = [vp, vp, vp]
    L.tsf_residual_autocorr.argtypes = [vp, i64, i32, vp, vp, i32, vp, ctypes.POINTER(TsfArArgs), ctypes.POINTER(TsfArOut)]
    L.tsf_residual_autocorr_dev.argtypes = L.tsf_residual_autocorr.argtypes + [vp]
    L.tsf_set_noise_ar.argtypes = [vp, vp, i64]
    L.tsf_residual_last.argtypes = [vp, i64, i32, vp, vp, i32, vp, ctypes.POINTER(TsfArLastOut)]
    L.tsf_residual_last_dev.argtypes = L.tsf_residual_last.argtypes + [vp]
    L.tsf_residual_autocorr_last.argtypes = L.tsf_residual_autocorr.argtypes + [ctypes.POINTER(TsfArLastOut)]
    L.tsf_set_noise_ar_start.argtypes = [vp, vp, vp, i64]
    L.tsf_noise_ar_mean.argtypes = [i64, vp, vp, vp, i32, vp]
    L.tsf_noise_state.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp,
                                  ctypes.POINTER(TsfArArgs), ctypes.POINTER(TsfNoiseStateOut)]
    L.tsf_noise_state_dev.argtypes = L.tsf_noise_state.argtypes + [vp]
    L.tsf_predict_conditioned.argtypes = L.tsf_predict.argtypes[:13] + [vp, vp, vp, vp, vp]
    L.tsf_predict_conditioned_dev.argtypes = L.tsf_predict_conditioned.argtypes + [vp]
    L.tsf_cond_columns.argtypes = [vp, ctypes.POINTER(TsfCondSeas), i64, vp, i32, vp, vp, i64]
    L.tsf_cond_columns_dev.argtypes = L.tsf_cond_columns.argtypes + [vp]
    L.tsf_eval.argtypes = [vp, psp, i64, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.tsf_eval_quadratic.argtypes = [vp, psp, i64, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.tsf_design.argtypes = [vp, psp, i32, vp, vp, vp, vp, vp]
    L.tsf_selftest_math.argtypes = [vp, i32, i64, vp, vp, vp]
    L.tsf_set_cost_hints.argtypes = [vp, vp, i64]
    L.tsf_set_option.argtypes = [vp, i32, i32]
    L.tsf_get_option.argtypes = [vp, i32]
    L.tsf_set_profiling.argtypes = [vp, i32]
    L.tsf_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_float), i32, ctypes.POINTER(i32)]
    L.tsf_last_fit_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.tsf_last_fit_route.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.tsf_fit_plan.argtypes = [psp, ctypes.POINTER(TsfFitShape), ctypes.POINTER(ctypes.c_int), ctypes.c_int, i64,
                               ctypes.POINTER(TsfFitPlanInfo)]
    L.tsf_fit_plan_error.argtypes = [i32]
    L.tsf_fit_plan_error.restype = ctypes.c_char_p
    L.tsf_last_fit_plan.argtypes = [vp, ctypes.POINTER(TsfFitPlanInfo)]
    L.tsf_cv_plan.argtypes = [i64, i32, vp, vp, ctypes.POINTER(TsfCvArgs), vp, vp, vp, vp, vp, vp, vp]
    L.tsf_cross_validate.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, vp, vp, ctypes.POINTER(TsfCvArgs), vp, i32,
                                     ctypes.c_double, ctypes.c_uint64, ctypes.POINTER(TsfCvOut)]
    L.tsf_last_cv_grids.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.tsf_tune.argtypes = [vp, psp, psp, i32, i64, i32, vp, vp, vp, i32, vp, vp, vp, ctypes.POINTER(TsfCvArgs), i32, i32,
                           ctypes.POINTER(TsfTuneOut)]
    L.tsf_last_tune_counts.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.tsf_select_stride.argtypes = [psp, i32]
    L.tsf_select.argtypes = [vp, psp, i32, i64, i32, vp, vp, vp, i32, vp, vp, vp, ctypes.POINTER(TsfCvArgs), i32,
                             ctypes.c_double, i32, i32, ctypes.POINTER(TsfSelectOut)]
    L.tsf_screen_rows.argtypes = [vp, i64, i32, vp, vp, i32, vp, vp, vp, ctypes.POINTER(TsfScreenArgs),
                                  ctypes.POINTER(TsfScreenOut)]
    L.tsf_screen_rows_dev.argtypes = L.tsf_screen_rows.argtypes + [vp]
    L.tsf_fit_screened.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, vp, vp, ctypes.c_double,
                                   ctypes.POINTER(TsfScreenArgs), ctypes.POINTER(TsfFitScreenedOut)]
    pca, pct = ctypes.POINTER(TsfCalibArgs), ctypes.POINTER(TsfCalibTable)
    L.tsf_calibrate_rows.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, pca, pct]
    L.tsf_calibrate_rows_dev.argtypes = L.tsf_calibrate_rows.argtypes + [vp]
    L.tsf_apply_calibration.argtypes = [vp, i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, pca, vp, vp, vp]
    L.tsf_apply_calibration_dev.argtypes = L.tsf_apply_calibration.argtypes + [vp]
    L.tsf_calibrate.argtypes = [vp, psp, i64, i32, vp, vp, vp, i32, vp, vp, vp, ctypes.POINTER(TsfCvArgs), vp, i32,
                                ctypes.c_double, ctypes.c_uint64, pca, pct, ctypes.POINTER(TsfCvOut)]
    L.tsf_pack_rows.argtypes = [i64, vp, vp, vp, vp, i32, ctypes.POINTER(vp), ctypes.POINTER(i64),
                                ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.tsf_pack_fetch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tsf_pack_rows_typed.argtypes = [i64, vp, vp, i32, vp, vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(i64),
                                      ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.tsf_pack_flags.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.tsf_pack_free.argtypes = [vp]
    L.tsf_pack_free.restype = None
    L.tsf_model_blobs.argtypes = [i64, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32]
    L.tsf_csv_read.argtypes = [i32, vp, vp, ctypes.c_char_p, i32,
                               ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i32),
                               ctypes.POINTER(i64)]
    L.tsf_csv_fetch.argtypes = [vp, vp, vp, vp, vp]
    L.tsf_csv_columns.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.tsf_csv_discover.argtypes = [ctypes.c_char_p, i32, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.tsf_csv_discover_load.argtypes = L.tsf_csv_discover.argtypes
    L.tsf_csv_read_loaded.argtypes = [vp, i32, i32, ctypes.c_char_p, i32, ctypes.POINTER(vp), ctypes.POINTER(i64),
                                      ctypes.POINTER(i32), ctypes.POINTER(i64)]
    L.tsf_csv_root_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.tsf_csv_root_load.argtypes = [vp, i32, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i32),
                                    ctypes.POINTER(i32)]
    L.tsf_csv_root_free.argtypes = [vp]
    L.tsf_csv_root_free.restype = None
    L.tsf_csv_dir_paths.argtypes = [vp]
    L.tsf_csv_dir_paths.restype = vp
    L.tsf_csv_dir_series_id.argtypes = [vp]
    L.tsf_csv_dir_series_id.restype = vp
    L.tsf_csv_dir_error_path.argtypes = [vp]
    L.tsf_csv_dir_error_path.restype = ctypes.c_char_p
    L.tsf_csv_dir_free.argtypes = [vp]
    L.tsf_csv_dir_free.restype = None
    L.tsf_csv_malformed.argtypes = [vp]
    L.tsf_csv_malformed.restype = ctypes.c_int64
    L.tsf_csv_free.argtypes = [vp]
    L.tsf_csv_free.restype = None
    L.tsf_csv_write_forecasts.argtypes = [ctypes.c_char_p, ctypes.c_char_p, i64, vp, vp, vp, vp, i32]
    L.tsf_csv_write_forecasts_i32.argtypes = [ctypes.c_char_p, ctypes.c_char_p, i64, vp, vp, vp, vp, i32]
    if L.tsf_spec_size() != ctypes.sizeof(TsfSpec):
        raise TsfError('tsf_spec layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_grid_info_size() != ctypes.sizeof(TsfGridInfo) or GRID_DTYPE.itemsize != ctypes.sizeof(TsfGridInfo):
        raise TsfError('tsf_grid_info layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_score_out_size() != ctypes.sizeof(TsfScoreOut):
        raise TsfError('tsf_score_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_window_out_size() != ctypes.sizeof(TsfWindowOut):
        raise TsfError('tsf_window_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_reconcile_out_size() != ctypes.sizeof(TsfReconcileOut):
        raise TsfError('tsf_reconcile_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_temporal_out_size() != ctypes.sizeof(TsfTemporalOut):
        raise TsfError('tsf_temporal_out layout mismatch between _lib.py and libtsf_amd.so')
    if (L.tsf_screen_args_size() != ctypes.sizeof(TsfScreenArgs) or L.tsf_screen_out_size() != ctypes.sizeof(TsfScreenOut)
            or L.tsf_fit_screened_out_size() != ctypes.sizeof(TsfFitScreenedOut)):
        raise TsfError('tsf_screen_args / tsf_screen_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_calib_args_size() != ctypes.sizeof(TsfCalibArgs) or L.tsf_calib_table_size() != ctypes.sizeof(TsfCalibTable):
        raise TsfError('tsf_calib_args / tsf_calib_table layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_corr_args_size() != ctypes.sizeof(TsfCorrArgs) or L.tsf_corr_out_size() != ctypes.sizeof(TsfCorrOut):
        raise TsfError('tsf_corr_args / tsf_corr_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_ar_args_size() != ctypes.sizeof(TsfArArgs) or L.tsf_ar_out_size() != ctypes.sizeof(TsfArOut):
        raise TsfError('tsf_ar_args / tsf_ar_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_ar_last_out_size() != ctypes.sizeof(TsfArLastOut):
        raise TsfError('tsf_ar_last_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_noise_state_out_size() != ctypes.sizeof(TsfNoiseStateOut):
        raise TsfError('tsf_noise_state_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_select_out_size() != ctypes.sizeof(TsfSelectOut):
        raise TsfError('tsf_select_out layout mismatch between _lib.py and libtsf_amd.so')
    if L.tsf_fit_plan_info_size() != ctypes.sizeof(TsfFitPlanInfo):
        raise TsfError('tsf_fit_plan_info layout mismatch between _lib.py and libtsf_amd.so')
    _lib = L
    return L


class Context(object):
    """One tsf_ctx: bound to one GPU, not re-entrant."""

    def __init__(self, device=0):
        L = load()
        h = ctypes.c_void_p()
        rc = L.tsf_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise TsfError('tsf_create(device=%d) failed (rc=%d): no usable MI355X visible. '
                           'This library has no CPU fallback.' % (device, rc))
        self._h = h
        self.device = int(device)
        # measurement tools: TSF_OPTIONS="harm=0,sparse_extra=0" sets route switches on every context this PROCESS
        # creates (read here, in the Python host layer; the library itself reads no environment variable for routes)
        for item in filter(None, os.environ.get('TSF_OPTIONS', '').split(',')):
            k, v = item.split('=')
            self.set_option(k.strip(), int(v))

    def close(self):
        if getattr(self, '_h', None):
            load().tsf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            msg = load().tsf_last_error(self._h)
            raise TsfError('libtsf_amd: rc=%d: %s' % (rc, msg.decode() if msg else '?'))

    @property
    def handle(self):
        return self._h

    def set_option(self, name, value=-1):
        """tsf_set_option: a route switch of THIS context (name: one of OPTIONS; -1 / None = the library's default).
        Results never depend on a route; tests and measurements use this."""
        self.check(load().tsf_set_option(self._h, OPTIONS.index(name), -1 if value is None else int(value)))

    def get_option(self, name):
        return int(load().tsf_get_option(self._h, OPTIONS.index(name)))

    @contextlib.contextmanager
    def options(self, **kw):
        """with ctx.options(harm=0, sparse_extra=0): ... -- set, run, restore."""
        old = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)


def fit_plan(spec, N, Tm, aligned=True, call=CALL_FIT, classes=False, n_distinct=0, lat_step=0, lat_U=0, opt=None, n_cu=256,
             mem_avail=-1):
    """tsf_fit_plan (include/tsf_dev.h): the route plan of one fit launch, on the host -- no context, no GPU.  spec: a
    TsfSpec; opt: {option name: value} over the defaults, or a full list.  Returns (rc, {field: value})."""
    sh = TsfFitShape(N=int(N), n_distinct=int(n_distinct), lat_step=int(lat_step), lat_U=int(lat_U), aligned=int(bool(aligned)),
                     Tm=int(Tm), call=int(call), classes=int(bool(classes)))
    if isinstance(opt, dict) or opt is None:
        vals = [-1] * len(OPTIONS)
        for k, v in (opt or {}).items():
            vals[OPTIONS.index(k)] = int(v)
    else:
        vals = [int(v) for v in opt]
    info = TsfFitPlanInfo()
    rc = load().tsf_fit_plan(ctypes.byref(spec), ctypes.byref(sh), (ctypes.c_int * len(vals))(*vals), int(n_cu), int(mem_avail),
                             ctypes.byref(info))
    return int(rc), info.as_dict()


def last_fit_plan(ctx):
    """tsf_last_fit_plan (include/tsf_dev.h): the plan the context's last fit launch used, as fit_plan returns it."""
    info = TsfFitPlanInfo()
    ctx.check(load().tsf_last_fit_plan(ctx.handle, ctypes.byref(info)))
    return info.as_dict()


def default_spec():
    s = TsfSpec()
    load().tsf_spec_default(ctypes.byref(s))
    return s


def _ptr(a):
    return None if a is None else a.ctypes.data


def y_dtype_code(y):
    if y.dtype == np.float64:
        return Y_F64
    if y.dtype == np.float32:
        return Y_F32
    if y.dtype == np.int32:
        return Y_I32
    raise TypeError('y must be float64, float32 or int32')
