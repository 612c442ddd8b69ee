// Temporal reconciliation (include/tsf.h "temporal reconciliation"): the rows of a forecast are the members, the draws of
// a model fitted on the period totals are the total, each row window is a group.  Reconciliation's projection applied
// along each sample's path inside one series.
//   temporal_reconcile_kernel  one thread per (chunk series, window, sample): the window's rows summed in row order,
//                              d = t - sum, the period draw rewritten to sum + share_total * d and the window's rows to
//                              x + share * d, both in place.  A streaming kernel: lanes are contiguous in the sample
//                              index at every row (coalesced), no LDS, no cross-lane traffic, no atomics.  The second
//                              sweep re-reads what the first just read with the same lanes on the same samples: a
//                              window's slice of a block is (rows * 2 KB), which the L2 still holds.
//   temporal_point_kernel      one thread per (series, window): the same rule on the two point forecasts
// Windows do not overlap (the driver refuses them), so no two blocks write one row; a row in no window is never touched.
// An inactive window (share_total NaN) has d = +0.0: the same operations then leave every finite value as it is.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

struct TemporalArgs {
    double *samp;               // [n_chunk][H][NS] the chunk's daily draws, the windows' rows rewritten in place
    double *win;                // [n_chunk][K][NS] the chunk's period draws, rewritten in place to the reconciled totals
    const int32_t *w0, *w1;     // [K] first row and one past the last row of every window, 0 <= w0 < w1 <= H, disjoint
    const double *share;        // [n_chunk][H] of the chunk's series
    const double *share_total;  // [n_chunk][K]; NaN: the window is not reconciled
    int H, K, NS;
};

// grid (n_chunk * K, ceil(NS / 256)), 256 threads: thread t of block (x, y) owns sample 256 y + t of one (series, window).
// w0, w1, share and share_total are the same for the whole block (scalar loads).
__global__ __launch_bounds__(256) void temporal_reconcile_kernel(TemporalArgs a)
{
    const int64_t nl = blockIdx.x / (unsigned)a.K;
    const int k = (int)(blockIdx.x - (unsigned)nl * (unsigned)a.K);
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s >= a.NS) return;
    const int r0 = a.w0[k], r1 = a.w1[k];
    const double mu_in = a.share_total[(size_t)nl * a.K + k];
    const bool active = mu_in == mu_in;
    const double mu = active ? mu_in : 0.0;
    const size_t NS = (size_t)a.NS;
    double *x = a.samp + ((size_t)nl * a.H + r0) * NS + s;
    double sum = x[0];
    for (int h = r0 + 1; h < r1; ++h) sum = sum + x[(size_t)(h - r0) * NS];
    double *t = a.win + ((size_t)nl * a.K + k) * NS + s;
    const double d = active ? *t - sum : 0.0;
    *t = sum + mu * d;
    const double *lam = a.share + (size_t)nl * a.H;
    for (int h = r0; h < r1; ++h) {
        double *xh = x + (size_t)(h - r0) * NS;
        *xh = *xh + lam[h] * d;
    }
}

// yhat [N][H] rewritten in place, total [N][K] written (null: not wanted); yp [N][K] the period model's point forecast
__global__ __launch_bounds__(256) void temporal_point_kernel(double *yhat, const double *yp, const int32_t *w0, const int32_t *w1,
                                                             const double *share, const double *share_total, double *total,
                                                             int64_t N, int H, int K)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N * K) return;
    const int64_t n = g / K;
    const int k = (int)(g - n * K);
    double *row = yhat + (size_t)n * H;
    const double *lam = share + (size_t)n * H;
    const int r0 = w0[k], r1 = w1[k];
    const double mu_in = share_total[g];
    const bool active = mu_in == mu_in;
    double ysum = row[r0];
    for (int h = r0 + 1; h < r1; ++h) ysum = ysum + row[h];
    const double dy = active ? yp[g] - ysum : 0.0;
    if (total) total[g] = ysum + (active ? mu_in : 0.0) * dy;
    for (int h = r0; h < r1; ++h) row[h] = row[h] + lam[h] * dy;
}

}  // namespace tsf
