// tsf_calib_kernels.h -- conformal interval calibration (include/tsf.h, "conformal interval calibration"):
//   calib_rows_kernel      one workgroup per series: the rule of include/tsf.h on a ragged set of holdout rows
//   calib_apply_kernel     a table applied to a forecast, elementwise over [N][L][H]
//   calib_cv_rows_kernel   tsf_calibrate: the horizon (cv_h) and the observed value of every holdout row of a
//                          cross-validation, in the order of its yhat [R]
//   calib_mask_kernel      tsf_calibrate: no table for a series whose cross-validation did not end TSF_CV_OK
//
// The sort choice.  Per distinct score set (one under ABS, one per level under CQR) the kernel runs TWO sorts of
// screen_sort's network over the launch's NSP rows (NSP = the row count rounded up to a power of two): one on the key
// (bucket, score), which leaves every bucket's scores ascending in one contiguous run of the array, then one on the
// score alone for the pooled cell.  The alternative -- B + 1 sorts, each cell compacted to its own power of two --
// needs no second array but a prefix scan and a pass over global memory per cell, up to 65 of them; the pair of sorts
// needs one byte per row beside the double: 9 NSP bytes + 520 of run bounds = 147 976 bytes at NSP = 16384, inside the
// 160 KiB a workgroup gets on gfx950.  So TSF_CALIB_MAX_ROWS is 16384, and a series costs two sorts whatever B is.
// Dead rows and padding enter as (bucket 255, +inf): behind every live row in both orders.
//
// Exchanges move values and round nothing, a cell's quantile is read at a rank of its own run, and the runs are found
// from the sorted keys: a series' table is a function of its multiset of (bucket, score) alone; neither the launch's NSP
// nor the rest of the batch nor the row order can show.  No atomics: a run's bounds are stored by the one thread that
// sees the key change.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_cv_kernels.h"
#include "tsf_screen_kernels.h"

namespace tsf {

struct CalibRowsArgs {
    const int64_t *row_off;     // [N+1]
    const int64_t *h;           // [R] ds - cutoff
    const double *y, *yhat;     // [R]
    const double *lower, *upper;// [L][R] (CQR) or nullptr
    const int32_t *sel;         // the series of this launch (block b works on sel[b]), or nullptr (block b on series b)
    int64_t R;
    int64_t horizon, w;         // w = (horizon + B - 1) / B
    int32_t mode, L, B, min_scores;
    double levels[TSF_CALIB_MAX_LEVELS];
    double *q;                  // [N][B+1][L]
    int32_t *n;                 // [N][B+1][L]
    int32_t *status;            // [N]
};

constexpr int CALIB_DEAD = 255;                         // the bucket of a row that is not live, and of the padding
constexpr size_t CALIB_RUN_BYTES = 2 * (TSF_CALIB_MAX_BUCKETS + 1) * sizeof(int);

__host__ __device__ inline size_t calib_lds_bytes(int NSP)
{
    return sizeof(double) * (size_t)NSP + (((size_t)NSP + 7) & ~(size_t)7) + CALIB_RUN_BYTES;
}

// the bucket of horizon h, or CALIB_DEAD where the row is not eligible (0 < h <= horizon)
__device__ __forceinline__ int calib_bucket(int64_t h, int64_t horizon, int64_t w, int32_t B)
{
    if (!(h > 0 && h <= horizon)) return CALIB_DEAD;
    const int64_t b = (h - 1) / w;
    return (int)(b < (int64_t)(B - 1) ? b : (int64_t)(B - 1));
}

// screen_sort's network on the key (bucket, score): begins and ends behind a barrier
__device__ __forceinline__ void calib_sort_keyed(double *v, uint8_t *bk, int NSP)
{
    __syncthreads();
    for (int k = 2; k <= NSP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < NSP; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool asc = (i & k) == 0;
                    const double x = v[i], y = v[ixj];
                    const uint8_t bx = bk[i], by = bk[ixj];
                    const bool gt = bx > by || (bx == by && x > y);
                    if (gt == asc) { v[i] = y; v[ixj] = x; bk[i] = by; bk[ixj] = bx; }
                }
            }
            __syncthreads();
        }
}

// rank rule of include/tsf.h on the ascending scores a[0 .. m): k = ceil((m + 1) * level), the k-th smallest, the
// largest where k > m; a zero comes out as +0.0
__device__ __forceinline__ double calib_quantile(const double *a, int64_t m, double level)
{
    const int64_t k = (int64_t)__builtin_ceil((double)(m + 1) * level);
    return a[(k < m ? k : m) - 1] + 0.0;
}

// Every branch around a barrier is on the launch's arguments or on the series' row count, the same for all threads of
// the workgroup: every barrier is reached by all threads or by none.  A series longer than the launch's NSP (or than
// TSF_CALIB_MAX_ROWS) never touches the sort arrays.
__global__ __launch_bounds__(256) void calib_rows_kernel(CalibRowsArgs a, int NSP)
{
    extern __shared__ __align__(16) unsigned char calib_smem[];
    double *v = reinterpret_cast<double *>(calib_smem);
    uint8_t *bk = calib_smem + sizeof(double) * (size_t)NSP;
    int *run_lo = reinterpret_cast<int *>(calib_smem + sizeof(double) * (size_t)NSP + (((size_t)NSP + 7) & ~(size_t)7));
    int *run_hi = run_lo + (TSF_CALIB_MAX_BUCKETS + 1);
    const int64_t n = a.sel ? a.sel[blockIdx.x] : (int64_t)blockIdx.x;
    const int64_t r0 = a.row_off[n], m0 = a.row_off[n + 1] - r0;
    const int B = a.B, L = a.L;
    const int cells = (B + 1) * L;
    double *q = a.q + (size_t)n * cells;
    int32_t *cnt = a.n + (size_t)n * cells;
    const double NaN = __builtin_nan(""), inf = __builtin_huge_val();
    if (m0 > (int64_t)TSF_CALIB_MAX_ROWS || m0 > (int64_t)NSP) {
        for (int c = threadIdx.x; c < cells; c += blockDim.x) { q[c] = NaN; cnt[c] = 0; }
        if (threadIdx.x == 0) a.status[n] = TSF_CALIB_TOO_LONG;
        return;
    }
    const int n_sets = a.mode == TSF_CALIB_CQR ? L : 1;
    bool any_pool = false;
    for (int set = 0; set < n_sets; ++set) {
        const int l0 = set, l1 = a.mode == TSF_CALIB_CQR ? set + 1 : L;     // the levels this score set serves
        const double *lo = a.mode == TSF_CALIB_CQR ? a.lower + (size_t)set * a.R + r0 : nullptr;
        const double *hi = a.mode == TSF_CALIB_CQR ? a.upper + (size_t)set * a.R + r0 : nullptr;
        __syncthreads();                // (the previous set's reads of the arrays are done)
        for (int i = threadIdx.x; i < B + 1; i += blockDim.x) { run_lo[i] = 0; run_hi[i] = 0; }
        for (int64_t i = threadIdx.x; i < (int64_t)NSP; i += blockDim.x) {
            double s = inf;
            int b = CALIB_DEAD;
            if (i < m0) {
                const double yv = a.y[r0 + i];
                bool live;
                if (a.mode == TSF_CALIB_CQR) {
                    const double l = lo[i], u = hi[i];
                    s = __builtin_fmax(l - yv, yv - u);
                    live = __builtin_isfinite(yv) && __builtin_isfinite(l) && __builtin_isfinite(u);
                } else {
                    s = __builtin_fabs(yv - a.yhat[r0 + i]);
                    live = __builtin_isfinite(s);
                }
                b = live ? calib_bucket(a.h[r0 + i], a.horizon, a.w, B) : CALIB_DEAD;
                if (b == CALIB_DEAD) s = inf;
            }
            v[i] = s;
            bk[i] = (uint8_t)b;
        }
        calib_sort_keyed(v, bk, NSP);
        // the run of every bucket that has rows: stored by the thread at the run's first row and the one at its last
        for (int i = threadIdx.x; i < NSP; i += blockDim.x) {
            const int b = bk[i];
            if (b == CALIB_DEAD) continue;
            if (i == 0 || bk[i - 1] != b) run_lo[b] = i;
            if (i == NSP - 1 || bk[i + 1] != b) run_hi[b] = i + 1;
        }
        __syncthreads();
        int64_t m_pool = 0;
        for (int b = 0; b < B; ++b) m_pool += run_hi[b] - run_lo[b];
        for (int c = threadIdx.x; c < B * (l1 - l0); c += blockDim.x) {
            const int b = c / (l1 - l0), l = l0 + c % (l1 - l0);
            const int64_t m = run_hi[b] - run_lo[b];
            cnt[b * L + l] = (int32_t)m;
            q[b * L + l] = m < (int64_t)a.min_scores ? NaN : calib_quantile(v + run_lo[b], m, a.levels[l]);
        }
        screen_sort(v, NSP);            // the pooled cell: the same scores, the buckets forgotten (dead rows stay +inf)
        for (int l = l0 + (int)threadIdx.x; l < l1; l += blockDim.x) {
            cnt[B * L + l] = (int32_t)m_pool;
            q[B * L + l] = m_pool < (int64_t)a.min_scores ? NaN : calib_quantile(v, m_pool, a.levels[l]);
        }
        any_pool = any_pool || m_pool >= (int64_t)a.min_scores;
    }
    if (threadIdx.x == 0) a.status[n] = any_pool ? TSF_CALIB_OK : TSF_CALIB_NO_SCORES;
}

struct CalibApplyArgs {
    int64_t N;
    int32_t H, L, B, mode, min_scores, shared_future;
    int64_t w;
    const double *yhat;         // [N][H]
    const double *lower, *upper;// [N][L][H] (CQR) or nullptr
    const int64_t *ds_future;   // [H] shared, [N][H] otherwise
    const int64_t *origin;      // [N]
    const double *q;            // [N][B+1][L]
    const int32_t *n;           // [N][B+1][L]
    double *lo, *hi;            // [N][L][H]
    int8_t *cell;               // [N][L][H] or nullptr
};

// one element (series, level, row) per thread, a grid-stride loop over N * L * H of them
__global__ __launch_bounds__(256) void calib_apply_kernel(CalibApplyArgs a)
{
    const int64_t total = a.N * a.L * a.H;
    const double NaN = __builtin_nan("");
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e % a.H, l = (e / a.H) % a.L, s = e / ((int64_t)a.H * a.L);
        const int64_t h = a.ds_future[a.shared_future ? i : s * a.H + i] - a.origin[s];
        int64_t b = 0;
        if (h > 0) { b = (h - 1) / a.w; b = b < (int64_t)(a.B - 1) ? b : (int64_t)(a.B - 1); }
        const size_t t0 = (size_t)s * (a.B + 1) * a.L;
        int64_t c = -1;
        if (a.n[t0 + (size_t)b * a.L + l] >= a.min_scores) c = b;
        else if (a.n[t0 + (size_t)a.B * a.L + l] >= a.min_scores) c = a.B;
        const double yh = a.yhat[s * a.H + i];
        double lo = NaN, hi = NaN;
        if (c >= 0 && __builtin_isfinite(yh)) {
            const double qv = a.q[t0 + (size_t)c * a.L + l];
            if (a.mode == TSF_CALIB_CQR) {
                lo = __builtin_fmin(a.lower[e] - qv, yh);
                hi = __builtin_fmax(a.upper[e] + qv, yh);
            } else {
                lo = yh - qv;
                hi = yh + qv;
            }
        }
        a.lo[e] = lo;
        a.hi[e] = hi;
        if (a.cell) a.cell[e] = (int8_t)c;
    }
}

// The holdout rows of a cross-validation as the rule's input: row r of series n (its folds' rows, fold by fold: the
// order of cv_metrics_kernel's yhat_out) gets h = ds - its fold's cutoff (cv_h) and its observed y as a double.  One
// workgroup per series.
__global__ __launch_bounds__(256) void calib_cv_rows_kernel(CvMetricArgs a, int64_t *__restrict__ h_out,
                                                            double *__restrict__ y_out)
{
    for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
        const int64_t f0 = a.fold_off[n], f1 = a.fold_off[n + 1];
        const int64_t r0 = a.rows_off[n], nr = a.rows_off[n + 1] - r0;
        if (f1 == f0) continue;
        const int64_t s0 = cv_ds0(a.p, n), y0 = cv_row0(a.p, n);
        for (int64_t r = threadIdx.x; r < nr; r += blockDim.x) {
            int64_t lo_f = f0, hi_f = f1 - 1;           // the fold holding row r: last f with fold_row0[f] <= r0 + r
            while (lo_f < hi_f) {
                const int64_t mid = (lo_f + hi_f + 1) >> 1;
                if (a.fold_row0[mid] <= r0 + r) lo_f = mid; else hi_f = mid - 1;
            }
            const int64_t f = lo_f, k = r0 + r - a.fold_row0[f];
            h_out[r0 + r] = cv_h(a, s0, f, k);
            y_out[r0 + r] = cv_y_typed(a.p, a.y_dtype, y0 + a.fold_hist[f] + k);
        }
    }
}

// A series whose cross-validation status is not TSF_CV_OK has no table: q NaN, n 0, TSF_CALIB_NO_SCORES.
__global__ __launch_bounds__(256) void calib_mask_kernel(int64_t N, int cells, const int32_t *__restrict__ cv_status,
                                                         double *__restrict__ q, int32_t *__restrict__ cnt,
                                                         int32_t *__restrict__ status)
{
    for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
        if (cv_status[n] == TSF_CV_OK) continue;
        for (int c = threadIdx.x; c < cells; c += blockDim.x) { q[(size_t)n * cells + c] = __builtin_nan(""); cnt[(size_t)n * cells + c] = 0; }
        if (threadIdx.x == 0) status[n] = TSF_CALIB_NO_SCORES;
    }
}

}  // namespace tsf
