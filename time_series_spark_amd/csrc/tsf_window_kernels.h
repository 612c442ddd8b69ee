// tsf_window_kernels.h -- quantiles and scores of totals over row windows (include/tsf.h, "totals over row windows"):
// tsf_predict_windows, tsf_rollup_windows.  The draws are tsf_predict_quantiles' (or a roll-up's accumulators, the same
// layout); what is new is that a row window [a, b) of every sample is summed on its way into LDS, so that no second
// sample buffer is needed (the running sums of `cumulative` take one).
//   window_score_kernel  one workgroup per (series of the chunk, window): the window sums of the samples into LDS, then
//                        the per-row kernels' sort (iv_sort_network) and score_kernel's reading of the sorted row
//                        (score_sorted_row): the levels, their pinball losses, the PIT, the CRPS of the window total
//   window_total_kernel  one thread per (series, window): the sum of the point forecasts of the window's rows
// The per-series means come from score_series_kernel (tsf_score_kernels.h) with the windows in the place of the rows.
// No floating-point atomics; a window's results are a function of its rows' draws and its y alone.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_score_kernels.h"

namespace tsf {

struct WindowArgs {
    const double *src;          // [n_chunk][H][NS] of the chunk (or a range of a roll-up's groups)
    const double *y;            // [N][K] of the call: the observed window totals, NaN = not observed; null: none given
    const int32_t *w0, *w1;     // [K] first row and one past the last row of every window, 0 <= w0 < w1 <= H
    double *pit, *crps;         // [N][K] of the call; null: not wanted
    double *q, *pinball;        // [N][n_q][K] of the call; null: not wanted
    int64_t n0;                 // first series of the chunk
    int H, K, NS, n_q;
    double level[TSF_MAX_QUANT];
};

// grid: n_chunk * K workgroups of 256 threads; NSP: NS rounded up to a power of two (<= 4096); LDS: NSP doubles
// (<= 32 KB), as quantile_kernel.  Thread t owns samples t, t + 256, ...: at every row of the window the lanes of a wave
// read 64 consecutive doubles.  The sum is interval_sample_kernel's running-sum expression started at row a: the first
// row's value, then one plain add per further row in the caller's row order.
__global__ __launch_bounds__(256) void window_score_kernel(WindowArgs a, int NSP)
{
    extern __shared__ __align__(16) unsigned char iv_smem[];
    double *v = reinterpret_cast<double *>(iv_smem);
    const int64_t nl = blockIdx.x / a.K;
    const int k = (int)(blockIdx.x - nl * a.K);
    const int NS = a.NS;
    const int r0 = a.w0[k], r1 = a.w1[k];
    const double *src = a.src + ((size_t)nl * a.H + r0) * NS;
    for (int i = threadIdx.x; i < NSP; i += blockDim.x) {
        double c = __builtin_huge_val();
        if (i < NS) {
            c = src[i];
            for (int h = r0 + 1; h < r1; ++h) c = c + src[(size_t)(h - r0) * NS + i];
        }
        v[i] = c;
    }
    __syncthreads();
    iv_sort_network(v, NSP);
    const size_t cell = (size_t)(a.n0 + nl) * a.K + k;
    const size_t at = (size_t)(a.n0 + nl) * a.n_q * a.K + k;       // level 0 of the window; level i: + i * K
    const double y = a.y ? a.y[cell] : __builtin_nan("");
    score_sorted_row(v, NS, NSP, y, a.level, a.n_q, a.q ? a.q + at : nullptr, a.pinball ? a.pinball + at : nullptr,
                     (size_t)a.K, a.pit ? a.pit + cell : nullptr, a.crps ? a.crps + cell : nullptr);
}

// total[n][k] = yhat[n][w0[k]] + ... + yhat[n][w1[k] - 1], added one row at a time in row order (the point forecast of
// the window's total: the sum of the point forecasts, not the mean of the draws)
__global__ __launch_bounds__(256) void window_total_kernel(const double *yhat, const int32_t *w0, const int32_t *w1,
                                                           double *total, int64_t N, int H, int K)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N * K) return;
    const int64_t n = g / K;
    const int k = (int)(g - n * K);
    const double *row = yhat + (size_t)n * H;
    const int r0 = w0[k], r1 = w1[k];
    double c = row[r0];
    for (int h = r0 + 1; h < r1; ++h) c = c + row[h];
    total[g] = c;
}

}  // namespace tsf
