/* Plain C99 caller of cross-validation through the C-ABI (include/tsf.h): plans with tsf_cv_plan, sizes the outputs
 * from it, runs tsf_cross_validate on an aligned panel read from raw binary files -- no Python in the process.
 * Usage: abi_cv N T ds.i64 y.f64 out.f64   (linear growth, additive weekly order 3, horizon 30 days, fbprophet's
 * default period / initial, rolling window 0.1, no intervals)
 * out: F*stride theta, then R yhat, then M mse, then M mape. */
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
    tsf_cv_args args;
    args.horizon_ns = (int64_t)30 * 86400 * 1000000000;
    args.period_ns = -1;
    args.initial_ns = -1;
    args.rolling_window = 0.1;

    int32_t *n_folds = calloc((size_t)N, sizeof(int32_t)), *status = calloc((size_t)N, sizeof(int32_t));
    int64_t *n_holdout = calloc((size_t)N, sizeof(int64_t)), *n_metric = calloc((size_t)N, sizeof(int64_t));
    if (tsf_cv_plan(N, T, NULL, ds, &args, n_folds, status, n_holdout, n_metric, NULL, NULL, NULL) != 0) return 3;
    int64_t F = 0, R = 0, M = 0;
    for (int64_t n = 0; n < N; ++n) { F += n_folds[n]; R += n_holdout[n]; M += n_metric[n]; }

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed: no GPU\n"); return 4; }
    tsf_cv_out out;
    memset(&out, 0, sizeof(out));
    out.fit.theta = calloc((size_t)(F * stride), sizeof(double));
    out.fit.y_scale = calloc((size_t)F, sizeof(double));
    out.fit.fval = calloc((size_t)F, sizeof(double));
    out.fit.status = calloc((size_t)F, sizeof(int32_t));
    out.fit.n_iter = calloc((size_t)F, sizeof(int32_t));
    out.fit.n_eval = calloc((size_t)F, sizeof(int32_t));
    out.fit.grid = calloc((size_t)F, sizeof(tsf_grid_info));
    out.yhat = calloc((size_t)R, sizeof(double));
    out.horizon_ns = calloc((size_t)M, sizeof(int64_t));
    out.mse = calloc((size_t)M, sizeof(double));
    out.rmse = calloc((size_t)M, sizeof(double));
    out.mae = calloc((size_t)M, sizeof(double));
    out.mape = calloc((size_t)M, sizeof(double));
    out.series_status = calloc((size_t)N, sizeof(int32_t));
    const int rc = tsf_cross_validate(ctx, &spec, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, NULL, &args, NULL, 0, 0.8, 0,
                                      &out);
    if (rc != 0) { fprintf(stderr, "cross-validate rc=%d: %s\n", rc, tsf_last_error(ctx)); return 5; }
    tsf_destroy(ctx);

    FILE *f = fopen(argv[5], "wb");
    if (!f) return 6;
    fwrite(out.fit.theta, sizeof(double), (size_t)(F * stride), f);
    fwrite(out.yhat, sizeof(double), (size_t)R, f);
    fwrite(out.mse, sizeof(double), (size_t)M, f);
    fwrite(out.mape, sizeof(double), (size_t)M, f);
    fclose(f);
    printf("folds=%lld holdout rows=%lld metric rows=%lld\n", (long long)F, (long long)R, (long long)M);
    return 0;
}
