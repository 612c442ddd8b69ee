// tsf_corr_kernels.h -- the estimator of a group's residual correlation (include/tsf.h, "correlated group roll-ups":
// tsf_residual_corr).  Three launches, none with atomics, each result a function of its own series / group alone:
//   corr_scale_kernel   one wave per series: the residuals' root mean square over the present rows (scale) and the
//                       standardised residuals e [N][T] (NaN where the row is absent or the series unused)
//   corr_rows_kernel    one thread per (group, row), consecutive threads on consecutive rows: walks the group's members
//                       (a host-built CSR, ascending series index) and writes c = u u - q and p = k (k - 1)
//   corr_group_kernel   one wave per group: the sums of c and p over the rows, the used members counted, rho
// The two sums over the rows (ss of a series, A of a group) have the library's shape: lane l adds rows l, l + 64, ...
// in ascending order from +0.0, the 64 partials are combined by the xor butterfly 1, 2, 4, 8, 16, 32 (a + b is
// commutative, so every lane ends with the same bits).  An absent row adds +0.0, which changes no bit of a partial.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

__device__ __forceinline__ double corr_wave_sum(double v)
{
    for (int d = 1; d <= 32; d <<= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int64_t corr_wave_sum(int64_t v)
{
    for (int d = 1; d <= 32; d <<= 1) v = v + (int64_t)__shfl_xor((long long)v, d, 64);
    return v;
}

struct CorrScaleArgs {
    const void *y;              // [N][T] in y_dtype
    const double *fitted;       // [N][T]
    int64_t N;
    int32_t T, y_dtype, min_rows;
    double *scale;              // [N]
    double *e;                  // [N][T]
};

constexpr int CORR_WAVES = 4;   // series per workgroup of corr_scale_kernel, groups per workgroup of corr_group_kernel

__global__ __launch_bounds__(CORR_WAVES * 64) void corr_scale_kernel(CorrScaleArgs a)
{
    const int64_t n = (int64_t)blockIdx.x * CORR_WAVES + (threadIdx.x >> 6);
    if (n >= a.N) return;       // (a whole wave: no lane of it reaches the butterfly)
    const int lane = threadIdx.x & 63;
    const int64_t r0 = n * a.T;
    double ss = 0.0;
    int64_t cnt = 0;
    for (int t = lane; t < a.T; t += 64) {
        const double r = load_y(a.y, a.y_dtype, r0 + t) - a.fitted[r0 + t];
        const bool present = __builtin_isfinite(r);
        ss = ss + (present ? r * r : 0.0);
        cnt += present ? 1 : 0;
    }
    ss = corr_wave_sum(ss);
    cnt = corr_wave_sum(cnt);
    const bool used = cnt >= (int64_t)a.min_rows && ss != 0.0;      // (a NaN ss cannot arise: only finite r are squared)
    const double NaN = __builtin_nan("");
    const double sc = used ? __builtin_sqrt(ss / (double)cnt) : NaN;
    if (lane == 0) a.scale[n] = sc;
    for (int t = lane; t < a.T; t += 64) {
        const double r = load_y(a.y, a.y_dtype, r0 + t) - a.fitted[r0 + t];
        a.e[r0 + t] = (used && __builtin_isfinite(r)) ? r / sc : NaN;
    }
}

struct CorrRowsArgs {
    const double *e;            // [N][T]
    const int32_t *first;       // [G + 1] offsets into member
    const int32_t *member;      // series indices, sorted by group, then ascending
    int32_t T, blocks_per_group;
    double *c;                  // [G][T]
    int64_t *p;                 // [G][T]
};

// grid G * blocks_per_group, 256 threads: thread t of block (g, b) owns row 256 b + t of group g.  A row is present for
// a member where its e is not NaN (corr_scale_kernel writes NaN for an absent row and for every row of an unused series).
__global__ __launch_bounds__(256) void corr_rows_kernel(CorrRowsArgs a)
{
    const int64_t g = blockIdx.x / (unsigned)a.blocks_per_group;
    const int t = (int)(blockIdx.x - (unsigned)g * (unsigned)a.blocks_per_group) * 256 + (int)threadIdx.x;
    if (t >= a.T) return;
    const int m0 = a.first[g], m1 = a.first[g + 1];
    double u = 0.0, q = 0.0;
    int64_t k = 0;
    for (int i = m0; i < m1; ++i) {
        const double e = a.e[(size_t)a.member[i] * a.T + t];
        if (e == e) {
            u = u + e;
            q = q + e * e;
            k += 1;
        }
    }
    a.c[(size_t)g * a.T + t] = u * u - q;
    a.p[(size_t)g * a.T + t] = k * (k - 1);
}

struct CorrGroupArgs {
    const double *c;            // [G][T]
    const int64_t *p;           // [G][T]
    const double *scale;        // [N]
    const int32_t *first, *member;
    int64_t G;
    int32_t T;
    double rho_max;
    double *rho, *rho_raw;      // [G]; rho_raw, n_pairs, n_used may be null
    int64_t *n_pairs;
    int32_t *n_used, *status;
};

__global__ __launch_bounds__(CORR_WAVES * 64) void corr_group_kernel(CorrGroupArgs a, int ok_status, int no_pairs_status)
{
    const int64_t g = (int64_t)blockIdx.x * CORR_WAVES + (threadIdx.x >> 6);
    if (g >= a.G) return;
    const int lane = threadIdx.x & 63;
    double A = 0.0;
    int64_t P = 0;
    for (int t = lane; t < a.T; t += 64) {
        A = A + a.c[(size_t)g * a.T + t];
        P += a.p[(size_t)g * a.T + t];
    }
    A = corr_wave_sum(A);
    P = corr_wave_sum(P);
    int64_t used = 0;
    for (int i = a.first[g] + lane; i < a.first[g + 1]; i += 64) {
        const double sc = a.scale[a.member[i]];
        used += (sc == sc) ? 1 : 0;
    }
    used = corr_wave_sum(used);
    if (lane != 0) return;
    const double raw = (P == 0) ? __builtin_nan("") : A / (double)P;
    a.rho[g] = (P == 0) ? 0.0 : __builtin_fmin(__builtin_fmax(raw, 0.0), a.rho_max);
    if (a.rho_raw) a.rho_raw[g] = raw;
    if (a.n_pairs) a.n_pairs[g] = P / 2;
    if (a.n_used) a.n_used[g] = (int32_t)used;
    a.status[g] = (P == 0) ? no_pairs_status : ok_status;
}

}  // namespace tsf
