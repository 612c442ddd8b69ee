// tsf_score_kernels.h -- observed values scored against the predictive distribution (include/tsf.h, "scoring
// observed values"): tsf_score_actuals.  The draws and the one sort per row are tsf_predict_quantiles'
// (tsf_interval_kernels.h); what is new is what is read from the sorted row.
//   score_kernel         one workgroup per (series, row) of a chunk's sample buffer, quantile_kernel's grid and LDS:
//                        the levels and their pinball losses, the PIT from two binary searches, the sample CRPS
//                        regrouped to non-negative terms and summed by a fixed halving tree in the same LDS
//   score_series_kernel  one thread per (series, column), columns = crps and every level: the means over the observed
//                        rows and the empirical coverage of every level, a sequential loop in the caller's row order
// No floating-point atomics; a row's results are a function of its sorted draws and its y alone, a series' of its rows
// alone, so neither the chunking nor the rest of the batch can show.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_interval_kernels.h"

namespace tsf {

struct ScoreArgs {
    const double *src;          // [n_chunk][H][NS] of the chunk
    const double *y;            // [N][H] of the call: the observed values, NaN = not observed
    double *pit, *crps;         // [N][H] of the call; null: not wanted
    double *q, *pinball;        // [N][n_q][H] of the call; null: not wanted
    int64_t n0;                 // first series of the chunk
    int H, NS, n_q;
    double level[TSF_MAX_QUANT];
};

// What score_kernel (and window_score_kernel, tsf_window_kernels.h) reads from one sorted row v[0 .. NS) in LDS (NSP
// doubles, the padding +inf) and the row's observed value y (NaN: not observed): the levels by quantile_kernel's
// expression and their pinball losses into q[i * stride] / pinball[i * stride], the PIT from two binary searches, the
// sample CRPS regrouped to non-negative terms and summed by a fixed halving tree in the same LDS (the sorted row is
// overwritten).  A null output is not wanted.  y is one value per workgroup, so every branch on it is uniform and every
// barrier is reached by all threads of the workgroup or by none.
__device__ __forceinline__ void score_sorted_row(double *v, int NS, int NSP, double y, const double *level, int n_q,
                                                 double *q, double *pinball, size_t stride, double *pit_out,
                                                 double *crps_out)
{
    const bool observed = y == y;
    const double NaN = __builtin_nan("");
    if (q || pinball)
        for (int i = threadIdx.x; i < n_q; i += blockDim.x) {
            // quantile_kernel's expression
            const double pos = level[i] * (double)(NS - 1);
            int lo = (int)__builtin_floor(pos);
            if (lo > NS - 1) lo = NS - 1;
            const int hi = lo + 1 < NS ? lo + 1 : NS - 1;
            const double val = v[lo] + (v[hi] - v[lo]) * (pos - (double)lo);
            if (q) q[(size_t)i * stride] = val;
            if (pinball) {
                const double e = y - val;
                pinball[(size_t)i * stride] = !observed ? NaN : (e >= 0.0 ? level[i] * e : (level[i] - 1.0) * e);
            }
        }
    // the PIT from exact counts over the NS real entries: lt = #{v < y}, le = #{v <= y} (the last thread: another wave
    // than the one that reads the levels)
    if (pit_out && threadIdx.x == blockDim.x - 1) {
        double pit = NaN;
        if (observed) {
            int lo = 0, hi = NS;
            while (lo < hi) { const int m = (lo + hi) >> 1; if (v[m] < y) lo = m + 1; else hi = m; }
            const int lt = lo;
            hi = NS;
            while (lo < hi) { const int m = (lo + hi) >> 1; if (v[m] <= y) lo = m + 1; else hi = m; }
            const int eq = lo - lt;
            pit = ((double)lt + 0.5 * (double)eq) / (double)NS;
        }
        *pit_out = pit;
    }
    if (!crps_out) return;
    if (!observed) {
        if (threadIdx.x == 0) *crps_out = NaN;
        return;
    }
    __syncthreads();            // every read of the sorted row is done: it is overwritten in place
    // mean|X - y| - mean|X - X'| / 2 over the sorted row = (1 / NS) sum_i (|d_i| - w_i d_i), d_i = v[i] - y,
    // w_i = (2 i - (NS - 1)) / NS: |w_i| < 1, so every term is >= 0 and the sum cancels nothing
    for (int i = threadIdx.x; i < NSP; i += blockDim.x) {
        double c = 0.0;
        if (i < NS) {
            const double d = v[i] - y;
            const double w = (double)(2 * i - (NS - 1)) / (double)NS;
            c = __builtin_fabs(d) - w * d;
        }
        v[i] = c;
    }
    __syncthreads();
    for (int s = NSP >> 1; s >= 1; s >>= 1) {
        for (int i = threadIdx.x; i < s; i += blockDim.x) v[i] = v[i] + v[i + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *crps_out = v[0] / (double)NS;
}

// NSP: NS rounded up to a power of two (<= 4096); LDS: NSP doubles (<= 32 KB, five workgroups of four waves per CU),
// as quantile_kernel.
__global__ __launch_bounds__(256) void score_kernel(ScoreArgs a, int NSP)
{
    extern __shared__ __align__(16) unsigned char iv_smem[];
    double *v = reinterpret_cast<double *>(iv_smem);
    const int64_t nl = blockIdx.x / a.H;
    const int h = (int)(blockIdx.x - nl * a.H);
    const int NS = a.NS;
    iv_load_sort(v, a.src + ((size_t)nl * a.H + h) * NS, NS, NSP);
    const size_t row = (size_t)(a.n0 + nl) * a.H + h;
    const size_t at = (size_t)(a.n0 + nl) * a.n_q * a.H + h;       // level 0 of the row; level i: + i * H
    score_sorted_row(v, NS, NSP, a.y[row], a.level, a.n_q, a.q ? a.q + at : nullptr, a.pinball ? a.pinball + at : nullptr,
                     (size_t)a.H, a.pit ? a.pit + row : nullptr, a.crps ? a.crps + row : nullptr);
}

struct ScoreSeriesArgs {
    const double *y;            // [N][H]
    const double *crps;         // [N][H]; null where mean_crps is
    const double *q, *pinball;  // [N][n_q][H]; null where coverage / mean_pinball is
    int32_t *n_obs;             // [N]; the outputs: null = not wanted
    double *mean_crps;          // [N]
    double *mean_pinball, *coverage;    // [N][n_q]
    int64_t N;
    int H, n_q;
};

// thread (n, c): c = 0 the crps column (and n_obs), c = 1 + i level i
__global__ __launch_bounds__(256) void score_series_kernel(ScoreSeriesArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int cols = 1 + a.n_q;
    if (g >= a.N * cols) return;
    const int64_t n = g / cols;
    const int c = (int)(g - n * cols);
    const double *y = a.y + (size_t)n * a.H;
    const double NaN = __builtin_nan("");
    int n_obs = 0;
    for (int h = 0; h < a.H; ++h) if (y[h] == y[h]) ++n_obs;
    if (c == 0) {
        if (a.n_obs) a.n_obs[n] = n_obs;
        if (a.mean_crps) {
            const double *x = a.crps + (size_t)n * a.H;
            double sum = 0.0;
            for (int h = 0; h < a.H; ++h) if (y[h] == y[h]) sum = sum + x[h];
            a.mean_crps[n] = n_obs ? sum / (double)n_obs : NaN;
        }
        return;
    }
    const size_t at = (size_t)n * a.n_q + (c - 1);
    if (a.mean_pinball) {
        const double *x = a.pinball + at * a.H;
        double sum = 0.0;
        for (int h = 0; h < a.H; ++h) if (y[h] == y[h]) sum = sum + x[h];
        a.mean_pinball[at] = n_obs ? sum / (double)n_obs : NaN;
    }
    if (a.coverage) {
        const double *x = a.q + at * a.H;
        int below = 0;
        for (int h = 0; h < a.H; ++h) if (y[h] <= x[h]) ++below;       // (false for a NaN y)
        a.coverage[at] = n_obs ? (double)below / (double)n_obs : NaN;
    }
}

}  // namespace tsf
