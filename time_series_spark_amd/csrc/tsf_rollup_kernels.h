// Group roll-ups (include/tsf.h "group roll-ups"): the draws of interval_sample_kernel summed across the series
// of a group, sample by sample, into accumulators that live across calls (tsf_rollup).
//   rollup_add_kernel     one thread per (touched group, row, sample): it adds the group's members of this chunk one
//                         at a time in list order -- a streaming pass with a fixed order of double adds per
//                         accumulator cell (no atomics, no LDS, no cross-lane traffic)
//   rollup_add_corr_kernel  the same pass on a handle with a noise correlation set: per member the term that gives the
//                         group's members a shared noise factor (with rollup_noise_scale_kernel, below)
//   rollup_cumsum_kernel  one thread per (group, sample): the running sum of the accumulator over the rows, for the
//                         cumulative quantiles (quantile_kernel sorts it, as it sorts the accumulator itself)
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

struct RollupAddArgs {
    const double *samples;      // [n_chunk][H][NS] of the chunk (interval_sample_kernel's output)
    const double *yhat;         // [n_chunk][H] of the chunk (predict_kernel's output)
    double *acc;                // [G][H][NS]
    double *ysum;               // [G][H]
    const int32_t *touched;     // [n_touched] groups this chunk has members of
    const int32_t *first;       // [n_touched + 1] offsets into `member`
    const int32_t *member;      // chunk-local series indices, ascending within a group
    int H, NS;
};

// grid (n_touched * H, ceil(NS / 256)), 256 threads: thread t of block (x, y) owns sample 256 y + t of one (touched
// group, row).  Lanes are contiguous in the sample index: every load and store is a coalesced 8-byte-per-lane stream.
// A cell's adds happen in one thread, in the order of `member`; the loads of the next members do not wait for them.
__global__ __launch_bounds__(256) void rollup_add_kernel(RollupAddArgs a)
{
    const int k = (int)(blockIdx.x / (unsigned)a.H);
    const int h = (int)(blockIdx.x - (unsigned)k * (unsigned)a.H);
    const int64_t g = a.touched[k];
    const int m0 = a.first[k], m1 = a.first[k + 1];
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        double *acc = a.acc + ((size_t)g * a.H + h) * a.NS + s;
        const double *src = a.samples + (size_t)h * a.NS + s;
        const size_t stride = (size_t)a.H * a.NS;
        double v = *acc;
#pragma unroll 4
        for (int i = m0; i < m1; ++i) v = v + src[(size_t)a.member[i] * stride];
        *acc = v;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        double y = a.ysum[(size_t)g * a.H + h];
        for (int i = m0; i < m1; ++i) y = y + a.yhat[(size_t)a.member[i] * a.H + h];
        a.ysum[(size_t)g * a.H + h] = y;
    }
}

// ---- the correlated add (include/tsf.h "correlated group roll-ups") ------------------------------------------------
// A handle with a noise correlation set (tsf_rollup_set_noise_corr) adds through rollup_add_corr_kernel: the same
// grid, ownership and order of adds as rollup_add_kernel, and per member the term that turns its observation noise
// (z sigma) y_scale into ((sqrt(1 - rho) z + sqrt(rho) w) sigma) y_scale, w the group's factor for this (row, sample).
// Nothing is stored per draw: z is regenerated from the member's noise stream (interval_sample_kernel's expression at
// the same key and counters), w comes from a stream of the group's own (stream 2).

// sn[n] = sigma_n * y_scale_n for the N series of one add call
__global__ __launch_bounds__(256) void rollup_noise_scale_kernel(const double *theta, int theta_stride, const double *y_scale,
                                                                 int64_t N, double *sn)
{
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < N) sn[n] = dm_exp(theta[(size_t)n * theta_stride + 2]) * y_scale[n];
}

// the standard normal of a noise stream at row h: interval_sample_kernel's Box-Muller expression
__device__ __forceinline__ double rollup_stream_normal(uint64_t key, uint64_t h)
{
    const double u1 = iv_u01(key, 2 * h), u2 = iv_u01(key, 2 * h + 1);
    double sn, cs;
    dm_sincos(6.283185307179586 * u2, sn, cs);
    return __builtin_sqrt(-2.0 * dm_log(u1)) * cs;
}

struct RollupCorrArgs {
    RollupAddArgs add;
    const double *a, *b;        // [G] sqrt(1 - rho) - 1 and sqrt(rho), formed on the host
    const int64_t *group_key;   // [G]
    const double *sn;           // [n_chunk] of the chunk (rollup_noise_scale_kernel's output)
    const int64_t *series_key;  // [n_chunk] of the chunk
    uint64_t seed;
};

// rollup_add_kernel's grid and ownership.  A group with rho == 0 (b == 0: uniform over the workgroup) takes that
// kernel's expression, so its bits are the independent roll-up's.
__global__ __launch_bounds__(256) void rollup_add_corr_kernel(RollupCorrArgs c)
{
    const RollupAddArgs &a = c.add;
    const int k = (int)(blockIdx.x / (unsigned)a.H);
    const int h = (int)(blockIdx.x - (unsigned)k * (unsigned)a.H);
    const int64_t g = a.touched[k];
    const int m0 = a.first[k], m1 = a.first[k + 1];
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        double *acc = a.acc + ((size_t)g * a.H + h) * a.NS + s;
        const double *src = a.samples + (size_t)h * a.NS + s;
        const size_t stride = (size_t)a.H * a.NS;
        const double ag = c.a[g], bg = c.b[g];
        double v = *acc;
        if (bg == 0.0) {
#pragma unroll 4
            for (int i = m0; i < m1; ++i) v = v + src[(size_t)a.member[i] * stride];
        } else {
            const double w = rollup_stream_normal(iv_key(c.seed, (uint64_t)c.group_key[g], (uint64_t)s, 2), (uint64_t)h);
            for (int i = m0; i < m1; ++i) {
                const int m = a.member[i];
                const double x = src[(size_t)m * stride];
                const double z = rollup_stream_normal(iv_key(c.seed, (uint64_t)c.series_key[m], (uint64_t)s, 1), (uint64_t)h);
                v = v + (x + ((ag * z + bg * w) * c.sn[m]));
            }
        }
        *acc = v;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        double y = a.ysum[(size_t)g * a.H + h];
        for (int i = m0; i < m1; ++i) y = y + a.yhat[(size_t)a.member[i] * a.H + h];
        a.ysum[(size_t)g * a.H + h] = y;
    }
}

// c[g][0][s] = acc[g][0][s], c[g][h][s] = c[g][h-1][s] + acc[g][h][s] for n_groups groups (acc and c point at the
// first of them).  One thread per (group, sample), consecutive threads on consecutive samples.
__global__ __launch_bounds__(256) void rollup_cumsum_kernel(const double *acc, double *c, int64_t n_groups, int H, int NS)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_groups * NS) return;
    const int64_t g = i / NS;
    const int s = (int)(i - g * NS);
    const double *src = acc + (size_t)g * H * NS + s;
    double *dst = c + (size_t)g * H * NS + s;
    double run = 0.0;
    for (int h = 0; h < H; ++h) {
        const double v = src[(size_t)h * NS];
        run = (h == 0) ? v : run + v;
        dst[(size_t)h * NS] = run;
    }
}

}  // namespace tsf
