/* Plain C99 caller of model-structure selection through the C-ABI (include/tsf.h): two candidates of different theta
 * stride, tsf_select with the refit on an aligned panel read from raw binary files -- no Python in the process.
 * Usage: abi_select N T ds.i64 y.f64 out.f64   (candidate 0: linear growth, 5 changepoints, additive weekly order 3;
 * candidate 1: linear growth, 25 changepoints, multiplicative weekly order 3; horizon 30 days, fbprophet's default
 * period / initial, rmse, tolerance 0.02, fallback 1)
 * Checked here: tsf_select_out_size, tsf_select_stride, and the padding of the refit rows (+0.0, sign included).
 * out: N*2 score, then N best and N chosen (as double), then N*stride_max refit theta. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tsf.h"

static void *slurp(const char *path, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    void *p = malloc(bytes ? bytes : 1);
    if (!f || !p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", path); exit(10); }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t T = atoi(argv[2]);
    int64_t *ds = slurp(argv[3], sizeof(int64_t) * (size_t)T);
    double *y = slurp(argv[4], sizeof(double) * (size_t)(N * T));

    tsf_spec cand[2];
    for (int c = 0; c < 2; ++c) {
        tsf_spec_default(&cand[c]);
        cand[c].growth = TSF_GROWTH_LINEAR;
        cand[c].n_seas = 1;
        cand[c].seas_period[0] = 7.0;
        cand[c].seas_order[0] = 3;
        cand[c].seas_prior_scale[0] = 10.0;
    }
    cand[0].n_changepoints = 5;
    cand[0].seas_mode[0] = TSF_MODE_ADDITIVE;
    cand[1].seas_mode[0] = TSF_MODE_MULTIPLICATIVE;
    const int32_t C = 2;
    if (tsf_select_out_size() != (int)sizeof(tsf_select_out)) { fprintf(stderr, "tsf_select_out size\n"); return 3; }
    const int s0 = tsf_theta_stride(&cand[0]), s1 = tsf_theta_stride(&cand[1]);
    const int stride = tsf_select_stride(cand, C);
    if (s0 >= s1 || stride != s1 || tsf_select_stride(cand, 1) != s0) { fprintf(stderr, "tsf_select_stride\n"); return 3; }
    tsf_cv_args args;
    args.horizon_ns = (int64_t)30 * 86400 * 1000000000;
    args.period_ns = -1;
    args.initial_ns = -1;
    args.rolling_window = 0.1;          /* (ignored by tsf_select) */

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed: no GPU\n"); return 4; }
    tsf_select_out out;
    memset(&out, 0, sizeof(out));
    out.score = calloc((size_t)(N * C), sizeof(double));
    out.cand_status = calloc((size_t)(N * C), sizeof(int32_t));
    out.best = calloc((size_t)N, sizeof(int32_t));
    out.chosen = calloc((size_t)N, sizeof(int32_t));
    out.series_status = calloc((size_t)N, sizeof(int32_t));
    out.fit.theta = malloc((size_t)(N * stride) * sizeof(double));
    for (int64_t i = 0; i < N * stride; ++i) out.fit.theta[i] = -1.0;       /* (the padding has to be written) */
    out.fit.y_scale = calloc((size_t)N, sizeof(double));
    out.fit.fval = calloc((size_t)N, sizeof(double));
    out.fit.status = calloc((size_t)N, sizeof(int32_t));
    out.fit.n_iter = calloc((size_t)N, sizeof(int32_t));
    out.fit.n_eval = calloc((size_t)N, sizeof(int32_t));
    out.fit.grid = calloc((size_t)C, sizeof(tsf_grid_info));
    const int rc = tsf_select(ctx, cand, C, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, NULL, &args, TSF_TUNE_RMSE, 0.02, 1, 1,
                              &out);
    if (rc != 0) { fprintf(stderr, "select rc=%d: %s\n", rc, tsf_last_error(ctx)); return 5; }
    tsf_destroy(ctx);

    for (int64_t n = 0; n < N; ++n) {
        if (out.chosen[n] < 0 || out.chosen[n] >= C) { fprintf(stderr, "chosen[%lld] out of range\n", (long long)n); return 7; }
        if (out.best[n] >= 0 && out.chosen[n] != out.best[n]) { fprintf(stderr, "chosen is not best\n"); return 7; }
        for (int k = out.chosen[n] == 0 ? s0 : s1; k < stride; ++k) {
            const double v = out.fit.theta[n * stride + k];
            if (v != 0.0 || signbit(v)) { fprintf(stderr, "padding of series %lld is not +0.0\n", (long long)n); return 8; }
        }
    }

    double *best = calloc((size_t)(2 * N), sizeof(double));
    for (int64_t n = 0; n < N; ++n) { best[n] = (double)out.best[n]; best[N + n] = (double)out.chosen[n]; }
    FILE *f = fopen(argv[5], "wb");
    if (!f) return 6;
    fwrite(out.score, sizeof(double), (size_t)(N * C), f);
    fwrite(best, sizeof(double), (size_t)(2 * N), f);
    fwrite(out.fit.theta, sizeof(double), (size_t)(N * stride), f);
    fclose(f);
    printf("series=%lld candidates=%d stride_max=%d\n", (long long)N, (int)C, stride);
    return 0;
}
