// tsf_cv_plan.cpp -- the host plan of tsf_cross_validate (include/tsf.h): fbprophet 0.5's generate_cutoffs and the
// row masks of cross_validation, per series, from the timestamps alone.  No device work, no tsf_ctx.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tsf.h"
#include "tsf_cv_plan.h"

namespace tsf_cv {

int resolve_args(const tsf_cv_args *a, tsf_cv_args *r)
{
    if (!a || a->horizon_ns <= 0) return -1;
    if (!(a->rolling_window >= 0.0 && a->rolling_window <= 1.0)) return -1;
    *r = *a;
    if (r->period_ns <= 0) r->period_ns = a->horizon_ns / 2;          // 0.5 * horizon
    if (r->initial_ns < 0) r->initial_ns = 3 * a->horizon_ns;         // 3 * horizon
    if (r->period_ns <= 0) return -1;
    return 0;
}

// rows <= v in ds[0 .. len) (sorted ascending)
static int64_t rows_le(const int64_t *ds, int64_t len, int64_t v)
{
    return std::upper_bound(ds, ds + len, v) - ds;
}

int series_plan(const int64_t *ds, int64_t len, const tsf_cv_args &a, std::vector<Fold> *folds, int64_t *n_holdout,
                int64_t *n_metric)
{
    folds->clear();
    *n_holdout = 0;
    *n_metric = 0;
    if (len < 1) return TSF_CV_LESS_THAN_HORIZON;
    const int64_t lo = ds[0], hi = ds[len - 1];
    // generate_cutoffs: the last cutoff is the latest date minus the horizon ...
    int64_t cutoff = hi - a.horizon_ns;
    if (cutoff < lo) return TSF_CV_LESS_THAN_HORIZON;
    std::vector<int64_t> res(1, cutoff);
    // ... then step back by `period` while the last one is >= min(ds) + initial
    while (res.back() >= lo + a.initial_ns) {
        cutoff -= a.period_ns;
        const int64_t i = rows_le(ds, len, cutoff);
        if (!(i < len && ds[i] <= cutoff + a.horizon_ns)) {
            // no row in (cutoff, cutoff + horizon]: the next cutoff is the last date <= cutoff, minus the horizon.  With no
            // such date pandas yields NaT, which ends the loop and is the entry dropped below -- so nothing is appended.
            if (i == 0) break;
            cutoff = ds[i - 1] - a.horizon_ns;
        }
        res.push_back(cutoff);
    }
    if (res.size() >= 1 && !(res.back() >= lo + a.initial_ns)) res.pop_back();    // result[:-1]
    if (res.empty()) return TSF_CV_NO_CUTOFF;
    std::reverse(res.begin(), res.end());
    std::vector<int64_t> h;
    for (int64_t c : res) {
        Fold f;
        f.cutoff = c;
        f.hist = rows_le(ds, len, c);
        if (f.hist < 2) { folds->clear(); *n_holdout = 0; return TSF_CV_TOO_FEW; }
        f.hold = rows_le(ds, len, c + a.horizon_ns) - f.hist;
        for (int64_t r = f.hist; r < f.hist + f.hold; ++r) h.push_back(ds[r] - c);
        *n_holdout += f.hold;
        folds->push_back(f);
    }
    // performance_metrics: one row per distinct horizon whose right-aligned window of w rows exists, i.e. whose
    // cumulative row count (horizons ascending) reaches w -- the distinct horizons among sorted rows w-1 .. n-1
    const int64_t n = (int64_t)h.size();
    std::sort(h.begin(), h.end());
    const int64_t w = window_rows(a.rolling_window, n);
    int64_t m = 0;
    for (int64_t i = w - 1; i < n; ++i)
        if (i == n - 1 || h[(size_t)i] != h[(size_t)i + 1]) ++m;
    *n_metric = m;
    return TSF_CV_OK;
}

int64_t window_rows(double rolling_window, int64_t n)
{
    int64_t w = (int64_t)(rolling_window * (double)n);       // int(): toward zero
    if (w < 1) w = 1;
    if (w > n) w = n;
    return w;
}

int panel_plan(int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds, const tsf_cv_args &a,
               std::vector<std::vector<Fold>> *folds, std::vector<int32_t> *status, std::vector<int64_t> *n_holdout,
               std::vector<int64_t> *n_metric)
{
    folds->assign((size_t)N, std::vector<Fold>());
    status->assign((size_t)N, 0);
    n_holdout->assign((size_t)N, 0);
    n_metric->assign((size_t)N, 0);
    if (!offsets) {
        // aligned panel: one timestamp vector, one plan for every series
        if (N > 0) {
            (*status)[0] = series_plan(ds, T, a, &(*folds)[0], &(*n_holdout)[0], &(*n_metric)[0]);
            for (int64_t n = 1; n < N; ++n) {
                (*folds)[(size_t)n] = (*folds)[0];
                (*status)[(size_t)n] = (*status)[0];
                (*n_holdout)[(size_t)n] = (*n_holdout)[0];
                (*n_metric)[(size_t)n] = (*n_metric)[0];
            }
        }
        return 0;
    }
    for (int64_t n = 0; n < N; ++n)
        (*status)[(size_t)n] = series_plan(ds + offsets[n], offsets[n + 1] - offsets[n], a, &(*folds)[(size_t)n],
                                           &(*n_holdout)[(size_t)n], &(*n_metric)[(size_t)n]);
    return 0;
}

int check_panel(int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds)
{
    if (N <= 0 || !ds) return -1;
    if (offsets) {
        if (T != 0 || offsets[0] != 0) return -1;
        for (int64_t n = 0; n < N; ++n)
            if (offsets[n + 1] < offsets[n] || offsets[n + 1] - offsets[n] > (int64_t)TSF_MAX_T) return -1;
    } else if (T < 1 || T > TSF_MAX_T) {
        return -1;
    }
    return 0;
}

}  // namespace tsf_cv

extern "C" int tsf_cv_plan(int64_t N, int32_t T, const int64_t *offsets, const int64_t *ds, const tsf_cv_args *args,
                           int32_t *n_folds, int32_t *status, int64_t *n_holdout, int64_t *n_metric, int64_t *cutoff,
                           int32_t *hist_rows, int32_t *hold_rows)
{
    using namespace tsf_cv;
    tsf_cv_args a;
    if (resolve_args(args, &a)) return -1;
    if (check_panel(N, T, offsets, ds)) return -1;
    if (!n_folds || !status || !n_holdout || !n_metric) return -1;
    std::vector<std::vector<Fold>> folds;
    std::vector<int32_t> st;
    std::vector<int64_t> nh, nm;
    panel_plan(N, T, offsets, ds, a, &folds, &st, &nh, &nm);
    int64_t f = 0;
    for (int64_t n = 0; n < N; ++n) {
        const std::vector<Fold> &fs = folds[(size_t)n];
        n_folds[n] = (int32_t)fs.size();
        status[n] = st[(size_t)n];
        n_holdout[n] = nh[(size_t)n];
        n_metric[n] = nm[(size_t)n];
        for (const Fold &x : fs) {
            if (cutoff) cutoff[f] = x.cutoff;
            if (hist_rows) hist_rows[f] = (int32_t)x.hist;
            if (hold_rows) hold_rows[f] = (int32_t)x.hold;
            ++f;
        }
    }
    return 0;
}
