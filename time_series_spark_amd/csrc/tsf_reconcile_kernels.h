// Forecast reconciliation in group roll-ups (include/tsf.h "reconciliation"): the draws of a group's members and the
// draws of its directly fitted total moved onto the coherent subspace, sample by sample.
//   reconcile_member_kernel  one thread per (chunk series, row, sample), in place on the chunk's sample buffer:
//                            samp = samp + share[n] * (top[g] - acc[g]), g = group[n]; three 8-byte reads and one
//                            write per cell, all coalesced streams (no atomics, no LDS, no cross-lane traffic)
//   reconcile_total_kernel   one thread per (group of a range, row, sample), from the two accumulators into scratch:
//                            out = acc + share_total[g] * (top - acc)
// Both do the point forecast's cells ([.][H]) with one thread per (series or group, row).  A group without a total has
// the incoherence d = +0.0: the same three operations then leave every finite value as it is.
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

struct ReconcileMemberArgs {
    double *samp;               // [n_chunk][H][NS] of the chunk (interval_sample_kernel's output), rewritten in place
    double *yhat;               // [n_chunk][H] of the chunk (predict_kernel's output), rewritten in place
    const double *acc, *top;    // [G][H][NS] the roll-up's two accumulators
    const double *ysum, *ytop;  // [G][H]
    const int32_t *has_top;     // [G]
    const int32_t *group;       // [n_chunk] of the chunk's series
    const double *share;        // [n_chunk]
    int H, NS;
};

// grid (n_chunk * H, ceil(NS / 256)), 256 threads: thread t of block (x, y) owns sample 256 y + t of one (series, row).
// Lanes are contiguous in the sample index; group, share and has_top are the same for the whole block (scalar loads).
__global__ __launch_bounds__(256) void reconcile_member_kernel(ReconcileMemberArgs a)
{
    const int64_t nl = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)nl * (unsigned)a.H);
    const int64_t g = a.group[nl];
    const double lam = a.share[nl];
    const bool has = a.has_top[g] != 0;
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        double *x = a.samp + ((size_t)nl * a.H + h) * a.NS + s;
        const size_t cell = ((size_t)g * a.H + h) * a.NS + s;
        const double d = has ? a.top[cell] - a.acc[cell] : 0.0;
        *x = *x + lam * d;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const size_t cell = (size_t)g * a.H + h;
        const double d = has ? a.ytop[cell] - a.ysum[cell] : 0.0;
        double *y = a.yhat + (size_t)nl * a.H + h;
        *y = *y + lam * d;
    }
}

struct ReconcileTotalArgs {
    const double *acc, *top;    // [G][H][NS]
    const double *ysum, *ytop;  // [G][H]
    const int32_t *has_top;     // [G]
    const double *share;        // [G] share_total
    double *out;                // [n_groups][H][NS] of the range (scratch)
    double *yout;               // [G][H]
    int64_t g0;                 // first group of the range
    int H, NS;
};

// grid (n_groups * H, ceil(NS / 256)), 256 threads, as above with (group of the range, row) in place of (series, row)
__global__ __launch_bounds__(256) void reconcile_total_kernel(ReconcileTotalArgs a)
{
    const int64_t gl = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)gl * (unsigned)a.H);
    const int64_t g = a.g0 + gl;
    const double mu = a.share[g];
    const bool has = a.has_top[g] != 0;
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        const size_t cell = ((size_t)g * a.H + h) * a.NS + s;
        const double v = a.acc[cell];
        const double d = has ? a.top[cell] - v : 0.0;
        a.out[((size_t)gl * a.H + h) * a.NS + s] = v + mu * d;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const size_t cell = (size_t)g * a.H + h;
        const double v = a.ysum[cell];
        const double d = has ? a.ytop[cell] - v : 0.0;
        a.yout[cell] = v + mu * d;
    }
}

}  // namespace tsf
