// tsf_ar_kernels.h -- the estimator of a series' lag-one residual autocorrelation (include/tsf.h, "serially correlated
// observation noise": tsf_residual_autocorr).  One launch, no atomics, each result a function of its own series alone:
//   ar_series_kernel    one wave per series: y and fitted are read once; the residual of row t - 1 comes from the
//                       neighbouring lane (lane 0: from lane 63 of the sweep's step before), which is the value a
//                       second read would form, bit for bit
//   ar_last_kernel      one wave per series: the last present row's residual and the rows behind it (tsf_residual_last,
//                       what the conditioned start of the chain is formed from); described at the kernel
// The two sums over the rows (ss over the present rows, C over the pairs) have the library's shape: lane l adds rows
// (pairs) l, l + 64, ... in ascending order from +0.0, the 64 partials are combined by the xor butterfly 1, 2, 4, 8,
// 16, 32 (corr_wave_sum).  An absent row or pair adds +0.0, which changes no bit of a partial.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip), behind tsf_corr_kernels.h.
#pragma once
#include "tsf_common.h"
#include "tsf_corr_kernels.h"

namespace tsf {

struct ArArgs {
    const void *y;              // rows of every series in y_dtype: [N][T], or ragged by offsets
    const double *fitted;       // the same layout
    const int64_t *offsets;     // [N + 1], or null = aligned [N][T]
    int64_t N;
    int32_t T, y_dtype, min_pairs;
    double phi_max;
    double *phi, *phi_raw;      // [N]; phi_raw, n_pairs, scale may be null
    int64_t *n_pairs;
    double *scale;
    int32_t *status;
};

constexpr int AR_WAVES = 4;     // series per workgroup

__global__ __launch_bounds__(AR_WAVES * 64) void ar_series_kernel(ArArgs a, int ok_status, int no_pairs_status)
{
    const int64_t n = (int64_t)blockIdx.x * AR_WAVES + (threadIdx.x >> 6);
    if (n >= a.N) return;       // (a whole wave: no lane of it reaches a shuffle)
    const int lane = threadIdx.x & 63;
    const int64_t r0 = a.offsets ? a.offsets[n] : n * a.T;
    const int64_t len = a.offsets ? a.offsets[n + 1] - r0 : (int64_t)a.T;
    const double NaN = __builtin_nan("");
    double ss = 0.0, C = 0.0;
    int64_t cnt = 0, np = 0;
    double carry = NaN;         // the residual of the row before this step's first (row -1: absent)
    for (int64_t base = 0; base < len; base += 64) {        // (the bound is the wave's: every lane takes every step)
        const int64_t t = base + lane;
        const double r = (t < len) ? load_y(a.y, a.y_dtype, r0 + t) - a.fitted[r0 + t] : NaN;
        const double left = __shfl(r, (lane + 63) & 63, 64);
        const double prev = (lane == 0) ? carry : left;
        carry = __shfl(r, 63, 64);
        const bool present = __builtin_isfinite(r);
        const bool pair = present && __builtin_isfinite(prev);
        ss = ss + (present ? r * r : 0.0);
        C = C + (pair ? r * prev : 0.0);
        cnt += present ? 1 : 0;
        np += pair ? 1 : 0;
    }
    ss = corr_wave_sum(ss);
    C = corr_wave_sum(C);
    cnt = corr_wave_sum(cnt);
    np = corr_wave_sum(np);
    if (lane != 0) return;
    const bool none = np < (int64_t)a.min_pairs || ss == 0.0;       // (a NaN ss cannot arise: only finite r are squared)
    const double var = ss / (double)cnt;                            // (NaN where cnt == 0: used only behind ss != 0)
    const double raw = none ? NaN : (C / (double)np) / var;
    a.phi[n] = none ? 0.0 : __builtin_fmin(__builtin_fmax(raw, 0.0), a.phi_max);
    a.status[n] = none ? no_pairs_status : ok_status;
    if (a.phi_raw) a.phi_raw[n] = raw;
    if (a.n_pairs) a.n_pairs[n] = np;
    if (a.scale) a.scale[n] = (ss == 0.0) ? NaN : __builtin_sqrt(var);
}

// ar_last_kernel (tsf_residual_last): the residual of each series' last present row and the number of rows behind it.
// One wave per series.  The wave walks the series from its end in blocks of 64 rows (the first block holds rows
// len - 64 .. len - 1; a lane in front of row 0 holds an absent row), every lane forms its row's residual, and a ballot
// over "finite" names the highest present row of the block; its value comes from that lane by a shuffle.  The loop ends
// at the first block with a present row, so a series whose final row is present reads 64 rows.
struct ArLastArgs {
    const void *y;              // as ArArgs
    const double *fitted;
    const int64_t *offsets;     // [N + 1], or null = aligned [N][T]
    int64_t N;
    int32_t T, y_dtype;
    double *last_resid;         // [N]
    int32_t *last_gap, *status; // [N]
};

__global__ __launch_bounds__(AR_WAVES * 64) void ar_last_kernel(ArLastArgs a, int ok_status, int no_row_status)
{
    const int64_t n = (int64_t)blockIdx.x * AR_WAVES + (threadIdx.x >> 6);
    if (n >= a.N) return;       // (a whole wave: no lane of it reaches the ballot)
    const int lane = threadIdx.x & 63;
    const int64_t r0 = a.offsets ? a.offsets[n] : n * a.T;
    const int64_t len = a.offsets ? a.offsets[n + 1] - r0 : (int64_t)a.T;
    double resid = 0.0;
    int64_t gap = len;
    int st = no_row_status;
    for (int64_t top = len; top > 0; top -= 64) {           // (the bound is the wave's: every lane takes every step)
        const int64_t t = top - 64 + lane;
        const double r = (t >= 0) ? load_y(a.y, a.y_dtype, r0 + t) - a.fitted[r0 + t] : __builtin_nan("");
        const unsigned long long present = __ballot(__builtin_isfinite(r));
        if (present) {
            const int hi = 63 - __builtin_clzll(present);
            resid = __shfl(r, hi, 64);
            gap = len - 1 - (top - 64 + hi);
            st = ok_status;
            break;
        }
    }
    if (lane != 0) return;
    a.last_resid[n] = resid;
    a.last_gap[n] = (int32_t)gap;
    a.status[n] = st;
}

}  // namespace tsf
