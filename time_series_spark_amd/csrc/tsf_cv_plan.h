// tsf_cv_plan.h -- host side of cross-validation (tsf_cv_plan.cpp), shared with tsf_cross_validate (tsf_api.hip).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/tsf.h"

namespace tsf_cv {

struct Fold {
    int64_t cutoff;     // ns
    int64_t hist;       // rows <= cutoff: the fold's history, rows [0, hist) of its series
    int64_t hold;       // rows in (cutoff, cutoff + horizon]: rows [hist, hist + hold)
};

// defaults filled in (period <= 0: horizon / 2; initial < 0: 3 * horizon); -1 on bad arguments
int resolve_args(const tsf_cv_args *a, tsf_cv_args *r);
// w = clamp(int(rolling_window * n), 1, n)
int64_t window_rows(double rolling_window, int64_t n);
int series_plan(const int64_t *ds, int64_t len, const tsf_cv_args &a, std::vector<Fold> *folds, int64_t *n_holdout,
                int64_t *n_metric);
int check_panel(int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds);
int panel_plan(int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds, const tsf_cv_args &a,
               std::vector<std::vector<Fold>> *folds, std::vector<int32_t> *status, std::vector<int64_t> *n_holdout,
               std::vector<int64_t> *n_metric);

}  // namespace tsf_cv
