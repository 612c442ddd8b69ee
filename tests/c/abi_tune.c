/* Plain C99 caller of prior-scale tuning through the C-ABI (include/tsf.h): two candidates that differ in
 * changepoint_prior_scale, tsf_tune with the refit on an aligned panel read from raw binary files -- no Python in the
 * process.
 * Usage: abi_tune N T ds.i64 y.f64 out.f64   (linear growth, additive weekly order 3, horizon 30 days, fbprophet's
 * default period / initial, rmse; candidates changepoint_prior_scale 0.01 and 0.5)
 * out: N*2 score, then N best (as double), then N*stride refit theta. */
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

    tsf_spec spec;
    tsf_spec_default(&spec);
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_seas = 1;
    spec.seas_period[0] = 7.0;
    spec.seas_order[0] = 3;
    spec.seas_prior_scale[0] = 10.0;
    spec.seas_mode[0] = TSF_MODE_ADDITIVE;
    const int stride = tsf_theta_stride(&spec);
    tsf_spec cand[2];
    cand[0] = spec;
    cand[0].changepoint_prior_scale = 0.01;
    cand[1] = spec;
    cand[1].changepoint_prior_scale = 0.5;
    const int32_t C = 2;
    tsf_cv_args args;
    args.horizon_ns = (int64_t)30 * 86400 * 1000000000;
    args.period_ns = -1;
    args.initial_ns = -1;
    args.rolling_window = 0.1;          /* (ignored by tsf_tune) */

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed: no GPU\n"); return 4; }
    tsf_tune_out out;
    memset(&out, 0, sizeof(out));
    out.score = calloc((size_t)(N * C), sizeof(double));
    out.cand_status = calloc((size_t)(N * C), sizeof(int32_t));
    out.best = calloc((size_t)N, sizeof(int32_t));
    out.series_status = calloc((size_t)N, sizeof(int32_t));
    out.fit.theta = calloc((size_t)(N * stride), sizeof(double));
    out.fit.y_scale = calloc((size_t)N, sizeof(double));
    out.fit.fval = calloc((size_t)N, sizeof(double));
    out.fit.status = calloc((size_t)N, sizeof(int32_t));
    out.fit.n_iter = calloc((size_t)N, sizeof(int32_t));
    out.fit.n_eval = calloc((size_t)N, sizeof(int32_t));
    out.fit.grid = calloc(1, sizeof(tsf_grid_info));
    const int rc = tsf_tune(ctx, &spec, cand, C, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, NULL, &args, TSF_TUNE_RMSE, 1,
                            &out);
    if (rc != 0) { fprintf(stderr, "tune rc=%d: %s\n", rc, tsf_last_error(ctx)); return 5; }
    tsf_destroy(ctx);

    double *best = calloc((size_t)N, sizeof(double));
    for (int64_t n = 0; n < N; ++n) best[n] = (double)out.best[n];
    FILE *f = fopen(argv[5], "wb");
    if (!f) return 6;
    fwrite(out.score, sizeof(double), (size_t)(N * C), f);
    fwrite(best, sizeof(double), (size_t)N, f);
    fwrite(out.fit.theta, sizeof(double), (size_t)(N * stride), f);
    fclose(f);
    printf("series=%lld candidates=%d\n", (long long)N, (int)C);
    return 0;
}
