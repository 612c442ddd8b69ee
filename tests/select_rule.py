"""The choice rule of tsf_select (include/tsf.h) restated in numpy, for the tests: per series m = the least finite score,
best = the lowest candidate with a finite score <= m * (1.0 + tolerance) (float64: one add, one multiply), the plan's
status kept, TSF_TUNE_NO_SCORE where no candidate has a finite score; chosen = best, or the fallback without one."""
import numpy as np

CV_OK = 0
TUNE_NO_SCORE = -24


def choose(score, plan_status, tolerance=0.0, fallback=0):
    """score [N][C] float64, plan_status [N] (TSF_CV_*: the plan's) -> (best, chosen, status), each [N] int32."""
    score = np.asarray(score, dtype=np.float64)
    plan_status = np.asarray(plan_status)
    N = score.shape[0]
    best = np.full(N, -1, np.int32)
    status = np.array(plan_status, dtype=np.int32)
    finite = np.isfinite(score)
    one_plus = np.float64(1.0) + np.float64(tolerance)
    for n in range(N):
        if plan_status[n] != CV_OK:
            continue
        if not finite[n].any():
            status[n] = TUNE_NO_SCORE
            continue
        m = score[n][finite[n]].min()
        with np.errstate(over='ignore'):
            thr = m * one_plus
        best[n] = int(np.flatnonzero(finite[n] & (score[n] <= thr))[0])
    chosen = np.where(best >= 0, best, np.int32(fallback)).astype(np.int32)
    return best, chosen, status
