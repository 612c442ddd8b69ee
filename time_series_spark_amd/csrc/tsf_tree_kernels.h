// Reconciliation over a tree of levels above a roll-up's groups (include/tsf.h "tree reconciliation"): one sweep up and
// one sweep down over the sample buffers the roll-up holds, then the members' second pass.
//   tree_blend_kernel   one thread per (node, row, sample) of a level: m = A + mu[n] * (t - A) where the node has a
//                       total, m = A where it has none (level 1: A = acc, t = top)
//   tree_gather_kernel  one thread per (parent, row, sample): A_p = the sum of its children's m from +0.0, in ascending
//                       child index (a CSR child list built by the host: block-uniform scalar loads)
//   tree_push_kernel    one thread per (node, row, sample) of a level below the top, in place on m:
//                       c = m + kappa[n] * (c_p - A_p), p the node's parent; at level 1 what is kept is c - acc
//   tree_member_kernel  one thread per (chunk series, row, sample), in place on the chunk's sample buffer:
//                       samp = samp + share[n] * delta[g], delta = c - acc of level 1: two 8-byte reads and one write
//   tree_total_kernel   one thread per (group of a range, row, sample): out = acc + delta, the reconciled group total
// All five are streaming kernels in reconcile_member_kernel's shape: grid (nodes * H, ceil(NS / 256)), 256 threads, lanes
// contiguous in the sample index, a guarded tail block, the point forecast's cell ([.][H]) done by thread 0 of the first
// block of a row; no atomics, no LDS, no cross-lane traffic, one writer per cell.  Every expression is the header's, in
// plain double operations (-ffp-contract=off).
// Non-template __global__ functions: include from exactly one translation unit (tsf_api.hip).
#pragma once
#include "tsf_common.h"

namespace tsf {

struct TreeBlendArgs {
    const double *A, *t;        // [n][H][NS] the bottom-up sum and the draws of the directly fitted totals (t: null = no total)
    double *m;                  // [n][H][NS]
    const double *yA, *yt;      // [n][H]
    double *ym;                 // [n][H]
    const int32_t *has;         // [n] the node has a total (null: none has)
    const double *mu;           // [n]
    int H, NS;
};

__global__ __launch_bounds__(256) void tree_blend_kernel(TreeBlendArgs a)
{
    const int64_t n = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)n * (unsigned)a.H);
    const bool has = a.has && a.has[n] != 0;
    const double mu = a.mu[n];
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        const size_t cell = ((size_t)n * a.H + h) * a.NS + s;
        const double v = a.A[cell];
        a.m[cell] = has ? v + mu * (a.t[cell] - v) : v;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const size_t cell = (size_t)n * a.H + h;
        const double v = a.yA[cell];
        a.ym[cell] = has ? v + mu * (a.yt[cell] - v) : v;
    }
}

struct TreeGatherArgs {
    const double *m;            // [n_children][H][NS] the level below
    double *A;                  // [n_parents][H][NS]
    const double *ym;           // [n_children][H]
    double *yA;                 // [n_parents][H]
    const int32_t *first;       // [n_parents + 1] into child
    const int32_t *child;       // [n_children] the children of each parent, ascending
    int H, NS;
};

__global__ __launch_bounds__(256) void tree_gather_kernel(TreeGatherArgs a)
{
    const int64_t p = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)p * (unsigned)a.H);
    const int j0 = a.first[p], j1 = a.first[p + 1];
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        double sum = 0.0;
        for (int j = j0; j < j1; ++j) sum = sum + a.m[((size_t)a.child[j] * a.H + h) * a.NS + s];
        a.A[((size_t)p * a.H + h) * a.NS + s] = sum;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        double sum = 0.0;
        for (int j = j0; j < j1; ++j) sum = sum + a.ym[(size_t)a.child[j] * a.H + h];
        a.yA[(size_t)p * a.H + h] = sum;
    }
}

struct TreePushArgs {
    double *m;                  // [n][H][NS] in: m; out: c, or c - acc where acc is given
    const double *cp, *Ap;      // [n_parents][H][NS] the level above: its c and its bottom-up sum
    const double *acc;          // [n][H][NS] level 1 only (null above it)
    double *ym;                 // [n][H]
    const double *ycp, *yAp;    // [n_parents][H]
    const double *yacc;         // [n][H] or null
    const int32_t *parent;      // [n]
    const double *kappa;        // [n]
    int H, NS;
};

__global__ __launch_bounds__(256) void tree_push_kernel(TreePushArgs a)
{
    const int64_t n = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)n * (unsigned)a.H);
    const int64_t p = a.parent[n];
    const double kappa = a.kappa[n];
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        const size_t cell = ((size_t)n * a.H + h) * a.NS + s, up = ((size_t)p * a.H + h) * a.NS + s;
        const double c = a.m[cell] + kappa * (a.cp[up] - a.Ap[up]);
        a.m[cell] = a.acc ? c - a.acc[cell] : c;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const size_t cell = (size_t)n * a.H + h, up = (size_t)p * a.H + h;
        const double c = a.ym[cell] + kappa * (a.ycp[up] - a.yAp[up]);
        a.ym[cell] = a.yacc ? c - a.yacc[cell] : c;
    }
}

struct TreeMemberArgs {
    double *samp;               // [n_chunk][H][NS] of the chunk (interval_sample_kernel's output), rewritten in place
    double *yhat;               // [n_chunk][H] of the chunk (predict_kernel's output), rewritten in place
    const double *delta;        // [G][H][NS] c - acc of the solved tree
    const double *ydelta;       // [G][H]
    const int32_t *group;       // [n_chunk] of the chunk's series
    const double *share;        // [n_chunk]
    int H, NS;
};

__global__ __launch_bounds__(256) void tree_member_kernel(TreeMemberArgs a)
{
    const int64_t nl = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)nl * (unsigned)a.H);
    const int64_t g = a.group[nl];
    const double lam = a.share[nl];
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        double *x = a.samp + ((size_t)nl * a.H + h) * a.NS + s;
        *x = *x + lam * a.delta[((size_t)g * a.H + h) * a.NS + s];
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        double *y = a.yhat + (size_t)nl * a.H + h;
        *y = *y + lam * a.ydelta[(size_t)g * a.H + h];
    }
}

struct TreeTotalArgs {
    const double *acc, *delta;  // [G][H][NS]
    const double *ysum, *ydelta;    // [G][H]
    double *out;                // [n_groups][H][NS] of the range (scratch)
    double *yout;               // [n_groups][H] of the range
    int64_t g0;                 // first group of the range
    int H, NS;
};

__global__ __launch_bounds__(256) void tree_total_kernel(TreeTotalArgs a)
{
    const int64_t gl = blockIdx.x / (unsigned)a.H;
    const int h = (int)(blockIdx.x - (unsigned)gl * (unsigned)a.H);
    const int64_t g = a.g0 + gl;
    const int s = (int)(blockIdx.y * 256 + threadIdx.x);
    if (s < a.NS) {
        const size_t cell = ((size_t)g * a.H + h) * a.NS + s;
        a.out[((size_t)gl * a.H + h) * a.NS + s] = a.acc[cell] + a.delta[cell];
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        const size_t cell = (size_t)g * a.H + h;
        a.yout[(size_t)gl * a.H + h] = a.ysum[cell] + a.ydelta[cell];
    }
}

}  // namespace tsf
