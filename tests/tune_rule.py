"""The choice rule of tsf_tune (include/tsf.h) restated in numpy, for the tests: per series the first candidate
attaining the minimum finite score (np.nanargmin's first minimum), the plan's status kept, TSF_TUNE_NO_SCORE where no
candidate has a finite score."""
import numpy as np

CV_OK = 0
TUNE_NO_SCORE = -24


def choose(score, plan_status):
    """score [N][C] float64, plan_status [N] (TSF_CV_*: the plan's) -> (best [N] int32, status [N] int32)."""
    score = np.asarray(score, dtype=np.float64)
    plan_status = np.asarray(plan_status)
    N = score.shape[0]
    best = np.full(N, -1, np.int32)
    status = np.array(plan_status, dtype=np.int32)
    finite = np.isfinite(score)
    for n in range(N):
        if plan_status[n] != CV_OK:
            continue
        if not finite[n].any():
            status[n] = TUNE_NO_SCORE
            continue
        row = np.where(finite[n], score[n], np.inf)
        best[n] = int(np.argmin(row))          # first minimum
    return best, status
