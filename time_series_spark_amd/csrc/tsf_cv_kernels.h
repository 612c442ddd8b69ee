// tsf_cv_kernels.h -- the device side of tsf_cross_validate (include/tsf.h): the fold panel built from the caller's
// panel, fold results put back into plan order, and the per-series metrics.  Non-template __global__ functions:
// include from exactly one translation unit (tsf_api.hip).
//
// Fold f (plan order: series by series, cutoffs ascending) of series n = fold_series[f] is rows [0, fold_hist[f]) of
// that series for the fit and rows [fold_hist[f], fold_hist[f] + fold_hold[f]) for the holdout.  The caller's panel
// is aligned (src_off == nullptr: series n at rows n*T of y, ds shared, extra [n_extra][T]) or ragged (series n at
// rows src_off[n] of y / ds / extra [n_extra][src_total]).
#pragma once
#include "tsf_common.h"

namespace tsf {

struct CvPanel {
    const int64_t *ds;          // caller's timestamps: [T] aligned, [src_total] ragged
    const void *y;              // caller's y, y_dtype
    const double *extra;        // [n_extra][T or src_total] or nullptr
    const int64_t *src_off;     // [N+1] ragged, nullptr aligned
    int64_t T, src_total;
    int ysz;                    // bytes per y value (8 or 4)
    int n_extra;
};

__device__ __forceinline__ int64_t cv_row0(const CvPanel &p, int64_t n) { return p.src_off ? p.src_off[n] : n * p.T; }
__device__ __forceinline__ int64_t cv_ds0(const CvPanel &p, int64_t n) { return p.src_off ? p.src_off[n] : 0; }
__device__ __forceinline__ int64_t cv_ex_stride(const CvPanel &p) { return p.src_off ? p.src_total : p.T; }
__device__ __forceinline__ double cv_y_typed(const CvPanel &p, int y_dtype, int64_t i)
{
    if (y_dtype == TSF_Y_F64) return ((const double *)p.y)[i];
    if (y_dtype == TSF_Y_F32) return (double)((const float *)p.y)[i];
    return (double)((const int32_t *)p.y)[i];
}

// The history rows of the folds gf[0 .. G) as one ragged panel: fold g at rows [dst_off[g], dst_off[g + 1]) of
// dst_ds / dst_y / dst_extra ([n_extra][dst_total]), its series' floor / cap at [g].  One workgroup per fold.
__global__ __launch_bounds__(256) void cv_expand_kernel(CvPanel p, int64_t G, const int32_t *__restrict__ gf,
                                                        const int32_t *__restrict__ fold_series,
                                                        const int64_t *__restrict__ dst_off, int64_t dst_total,
                                                        const double *__restrict__ floor_, const double *__restrict__ cap,
                                                        int64_t *__restrict__ dst_ds, void *__restrict__ dst_y,
                                                        double *__restrict__ dst_extra, double *__restrict__ dst_floor,
                                                        double *__restrict__ dst_cap)
{
    for (int64_t g = blockIdx.x; g < G; g += gridDim.x) {
        const int64_t n = fold_series[gf[g]];
        const int64_t d0 = dst_off[g], rows = dst_off[g + 1] - d0;
        const int64_t r0 = cv_row0(p, n), s0 = cv_ds0(p, n), es = cv_ex_stride(p);
        for (int64_t i = threadIdx.x; i < rows; i += blockDim.x) {
            dst_ds[d0 + i] = p.ds[s0 + i];
            if (p.ysz == 8) ((uint64_t *)dst_y)[d0 + i] = ((const uint64_t *)p.y)[r0 + i];
            else ((uint32_t *)dst_y)[d0 + i] = ((const uint32_t *)p.y)[r0 + i];
            for (int e = 0; e < p.n_extra; ++e) dst_extra[(size_t)e * dst_total + d0 + i] = p.extra[(size_t)e * es + s0 + i];
        }
        if (threadIdx.x == 0) {
            if (floor_) dst_floor[g] = floor_[n];
            if (cap) dst_cap[g] = cap[n];
        }
    }
}

// The holdout rows of every fold as a padded future panel [F][Hmax] (rows past a fold's last holdout row repeat it:
// neither the point forecast nor the interval samples of a row depend on rows after it, and the largest future time
// stays the fold's own), extra_future [F][n_extra][Hmax], and the fold's random-stream key (include/tsf.h).
__global__ __launch_bounds__(256) void cv_holdout_kernel(CvPanel p, int64_t F, int32_t Hmax,
                                                         const int32_t *__restrict__ fold_series,
                                                         const int32_t *__restrict__ fold_c,
                                                         const int64_t *__restrict__ fold_hist,
                                                         const int64_t *__restrict__ fold_hold,
                                                         const int64_t *__restrict__ series_key,
                                                         int64_t *__restrict__ ds_fut, double *__restrict__ ex_fut,
                                                         int64_t *__restrict__ key_out)
{
    for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
        const int64_t n = fold_series[f], h0 = fold_hist[f], hn = fold_hold[f];
        const int64_t s0 = cv_ds0(p, n) + h0, es = cv_ex_stride(p);
        for (int i = threadIdx.x; i < Hmax; i += blockDim.x) {
            const int64_t r = s0 + (i < hn ? i : hn - 1);
            ds_fut[(size_t)f * Hmax + i] = p.ds[r];
            for (int e = 0; e < p.n_extra; ++e) ex_fut[((size_t)f * p.n_extra + e) * Hmax + i] = p.extra[(size_t)e * es + r];
        }
        if (threadIdx.x == 0) {
            const uint64_t k = series_key ? (uint64_t)series_key[n] : (uint64_t)n;
            key_out[f] = (int64_t)(k * 0x9E3779B97F4A7C15ULL + (uint64_t)fold_c[f]);
        }
    }
}

// Fit outputs of one launch (folds gf[0 .. G), in launch order) to their plan positions.  One wave per fold.
__global__ __launch_bounds__(64) void cv_scatter_kernel(int64_t G, const int32_t *__restrict__ gf, int stride,
                                                        tsf_fit_out src, tsf_fit_out dst)
{
    const int64_t g = blockIdx.x;
    if (g >= G) return;
    const int64_t f = gf[g];
    for (int k = threadIdx.x; k < stride; k += 64) dst.theta[(size_t)f * stride + k] = src.theta[(size_t)g * stride + k];
    constexpr int GW = (int)(sizeof(tsf_grid_info) / 8);
    static_assert(sizeof(tsf_grid_info) % 8 == 0, "grid info in 8-byte words");
    for (int k = threadIdx.x; k < GW; k += 64)
        ((uint64_t *)(dst.grid + f))[k] = ((const uint64_t *)(src.grid + g))[k];
    if (threadIdx.x == 0) {
        dst.y_scale[f] = src.y_scale[g]; dst.fval[f] = src.fval[g]; dst.status[f] = src.status[g];
        dst.n_iter[f] = src.n_iter[g]; dst.n_eval[f] = src.n_eval[g];
    }
}

struct CvMetricArgs {
    CvPanel p;
    int y_dtype;
    int64_t N;
    int32_t Hmax;
    const int64_t *fold_off;    // [N+1] folds of series n: [fold_off[n], fold_off[n+1])
    const int64_t *rows_off;    // [N+1] holdout rows of series n (all folds, fold by fold): [rows_off[n], rows_off[n+1])
    const int64_t *m_off;       // [N+1] metric rows of series n
    const int64_t *cutoff, *fold_hist, *fold_hold, *fold_row0;   // [F]; fold_row0: first holdout row of the fold in [R]
    const int32_t *fit_status;  // [F]
    const double *yhat, *lo, *hi;                       // [F][Hmax] (lo / hi nullptr without intervals)
    double rolling_window;
    // scratch [R]: the rows sorted by horizon, and per quantity the levels of a tree of block sums [R + 64 N] (series n
    // at rows_off[n] + 64 n; its levels 1, 2, .. take fewer than its rows + 64 slots)
    int64_t *h_s;
    double *t_s;                // [4][R]: squared error, absolute error, absolute percentage error, covered
    double *pre;                // [4][R + 64 N]
    int64_t R;
    // outputs
    double *yhat_out, *lo_out, *hi_out;                 // [R]
    int64_t *horizon;                                   // [M]
    double *mse, *rmse, *mae, *mape, *coverage;         // [M]
    int32_t *series_status;                             // [N] in: the plan's, out: TSF_CV_FIT_FAILED where a fit failed
};

// k-th holdout horizon of fold f (ascending in k: ds is sorted)
__device__ __forceinline__ int64_t cv_h(const CvMetricArgs &a, int64_t s0, int64_t f, int64_t k)
{
    return a.p.ds[s0 + a.fold_hist[f] + k] - a.cutoff[f];
}
// rows of fold f with horizon < v (lt) or <= v
__device__ __forceinline__ int64_t cv_count(const CvMetricArgs &a, int64_t s0, int64_t f, int64_t v, bool le)
{
    int64_t lo = 0, hi = a.fold_hold[f];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t x = cv_h(a, s0, f, mid);
        if (le ? (x <= v) : (x < v)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sum of the terms t[lo, hi) of one series from its tree (level 0: t [len0], level k >= 1: node i = the sum of nodes 2i
// and 2i + 1 of level k - 1, stored level after level from `tree`): the O(log) nodes that tile [lo, hi) exactly.
__device__ __forceinline__ double cv_tree_sum(const double *t, const double *tree, int64_t len0, int64_t lo, int64_t hi)
{
    const double *lev = t;
    int64_t len = len0, off = 0;
    double s = 0.0;
    while (lo < hi) {
        if (lo & 1) s += lev[lo++];
        if (hi & 1) s += lev[--hi];
        lo >>= 1; hi >>= 1;
        const int64_t nl = (len + 1) >> 1;
        lev = tree + off; off += nl; len = nl;
    }
    return s;
}

// performance_metrics of one series per wave (include/tsf.h): its C holdout runs (each sorted by horizon) are merged
// by rank -- every row counts, by binary search in each run, the rows that precede it (smaller horizon, or equal
// horizon in an earlier fold / earlier in its own) -- so all lanes place rows at once; then a tree of pairwise block
// sums of the terms in merged order, and for every distinct horizon h whose window of w rows exists, the window's left
// end: the group [gb, ge) holding merged row E - w (E = rows up to and including h's group), found by binary search.
// The window is S[ge, E) + (ge - E + w) / (ge - gb) * S[gb, ge), each S from tree nodes inside it: every term is >= 0
// and no row outside [gb, E) enters, so one large term cannot cancel the windows that do not hold it (as differences
// of prefix sums over all rows would).
__global__ __launch_bounds__(64) void cv_metrics_kernel(CvMetricArgs a)
{
    const int64_t n = blockIdx.x;
    const int lane = threadIdx.x;
    if (n >= a.N) return;
    const int64_t f0 = a.fold_off[n], f1 = a.fold_off[n + 1];
    const int64_t r0 = a.rows_off[n], nr = a.rows_off[n + 1] - r0;
    if (f1 == f0 || nr == 0) return;
    const int64_t s0 = cv_ds0(a.p, n), y0 = cv_row0(a.p, n);
    const bool iv = a.lo != nullptr;
    // 1) place every row at its merged position; copy the forecasts out; smallest |y|; failed fits
    double ymin = __builtin_huge_val();
    int bad = 0;
    for (int64_t f = f0 + lane; f < f1; f += 64) bad |= a.fit_status[f] < 0 ? 1 : 0;
    for (int64_t r = lane; r < nr; r += 64) {
        int64_t lo_f = f0, hi_f = f1 - 1;          // the fold holding row r: last f with fold_row0[f] <= r0 + r
        while (lo_f < hi_f) {
            const int64_t mid = (lo_f + hi_f + 1) >> 1;
            if (a.fold_row0[mid] <= r0 + r) lo_f = mid; else hi_f = mid - 1;
        }
        const int64_t f = lo_f, k = r0 + r - a.fold_row0[f];
        const int64_t h = cv_h(a, s0, f, k);
        int64_t rank = k - cv_count(a, s0, f, h, false);
        for (int64_t g = f0; g < f1; ++g) rank += cv_count(a, s0, g, h, g < f);
        const double yv = cv_y_typed(a.p, a.y_dtype, y0 + a.fold_hist[f] + k);
        const double yh = a.yhat[(size_t)f * a.Hmax + k];
        const double err = yv - yh;
        a.yhat_out[r0 + r] = yh;
        double cov = 0.0;
        if (iv) {
            const double l = a.lo[(size_t)f * a.Hmax + k], u = a.hi[(size_t)f * a.Hmax + k];
            a.lo_out[r0 + r] = l; a.hi_out[r0 + r] = u;
            cov = (yv >= l && yv <= u) ? 1.0 : 0.0;
        }
        const int64_t q = r0 + rank;
        a.h_s[q] = h;
        a.t_s[q] = err * err;
        a.t_s[a.R + q] = __builtin_fabs(err);
        a.t_s[2 * a.R + q] = __builtin_fabs(err / yv);
        a.t_s[3 * a.R + q] = cov;
        const double ay = __builtin_fabs(yv);
        ymin = ay < ymin ? ay : ymin;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(ymin, d, 64);
        ymin = o < ymin ? o : ymin;
    }
    bad = __any(bad) ? 1 : 0;
    __syncthreads();
    // 2) the tree of block sums of the four terms in merged order, level by level
    const int64_t p0 = r0 + 64 * n;
    const size_t qs = (size_t)(a.R + 64 * a.N);
    for (int64_t len = nr, src = -1, dst = 0; len > 1;) {
        const int64_t nl = (len + 1) >> 1;
        for (int qn = 0; qn < 4; ++qn) {
            double *tree = a.pre + qn * qs + p0;
            const double *x = src < 0 ? a.t_s + (size_t)qn * a.R + r0 : tree + src;
            for (int64_t i = lane; i < nl; i += 64)
                tree[dst + i] = 2 * i + 1 < len ? x[2 * i] + x[2 * i + 1] : x[2 * i];
        }
        __syncthreads();
        src = dst; dst += nl; len = nl;
    }
    // 3) one metric row per distinct horizon whose cumulative count reaches w
    const int64_t w = [&] { int64_t x = (int64_t)(a.rolling_window * (double)nr); return x < 1 ? 1 : (x > nr ? nr : x); }();
    const int64_t *hs = a.h_s + r0;
    const int64_t m0 = a.m_off[n];
    const bool mape_ok = !(ymin < 1e-8);
    const double NaN = __builtin_nan("");
    if (bad && lane == 0) a.series_status[n] = TSF_CV_FIT_FAILED;
    int64_t out_base = 0;
    for (int64_t b = w - 1; b < nr; b += 64) {
        const int64_t i = b + lane;
        const bool end = i < nr && (i == nr - 1 || hs[i] != hs[i + 1]);
        const unsigned long long mask = __ballot(end);
        if (end) {
            const int64_t o = m0 + out_base + __popcll(mask & ((1ull << lane) - 1ull));
            const int64_t E = i + 1, qrow = E - w, hq = hs[qrow];
            int64_t lo = 0, hi = qrow;                          // group start: first row with horizon hq
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (hs[mid] < hq) lo = mid + 1; else hi = mid; }
            const int64_t gb = lo;
            lo = qrow + 1; hi = nr;                             // group end: first row with horizon > hq
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (hs[mid] <= hq) lo = mid + 1; else hi = mid; }
            const int64_t ge = lo;
            double v[4];
            for (int qn = 0; qn < 4; ++qn) {
                const double *t = a.t_s + (size_t)qn * a.R + r0, *tree = a.pre + qn * qs + p0;
                const double whole = cv_tree_sum(t, tree, nr, ge, E);
                const double left = cv_tree_sum(t, tree, nr, gb, ge);
                v[qn] = (whole + (double)(ge - E + w) * left / (double)(ge - gb)) / (double)w;
            }
            a.horizon[o] = hs[i];
            a.mse[o] = bad ? NaN : v[0];
            a.rmse[o] = bad ? NaN : __builtin_sqrt(v[0]);
            a.mae[o] = bad ? NaN : v[1];
            a.mape[o] = (bad || !mape_ok) ? NaN : v[2];
            if (iv) a.coverage[o] = bad ? NaN : v[3];
        }
        out_base += __popcll(mask);
    }
}

}  // namespace tsf
