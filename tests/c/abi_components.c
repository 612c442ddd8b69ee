/* Plain C99 caller of the forecast decomposition through the C-ABI (include/tsf.h): tsf_predict_components on the
 * model of tests/forecast_cases.py case iv129 (linear growth, yearly order 10 + weekly order 3 additive, one additive and
 * one multiplicative extra column, 60 changepoints, a shared future grid) read from raw binary files -- no Python in the
 * process.  Components: additive_terms, extra_regressors_additive, extra_regressors_multiplicative; 200 samples, width
 * 0.8, seed 5, series_key NULL.
 * Usage: abi_components N H dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64; writes dir/out.f64:
 * yhat, trend, comp [N][3][H], yhat_lower, yhat_upper, trend_lower, trend_upper) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tsf.h"

static void *slurp(const char *dir, const char *name, size_t bytes)
{
    char path[4096];
    snprintf(path, sizeof(path), "%s/%s", dir, name);
    FILE *f = fopen(path, "rb");
    void *p = malloc(bytes ? bytes : 1);
    if (!f || !p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", path); exit(10); }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t H = atoi(argv[2]);
    const char *dir = argv[3];

    tsf_spec spec;
    tsf_spec_default(&spec);
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_changepoints = 60;
    spec.n_seas = 2;
    spec.seas_period[0] = 365.25; spec.seas_order[0] = 10; spec.seas_mode[0] = TSF_MODE_ADDITIVE;
    spec.seas_period[1] = 7.0; spec.seas_order[1] = 3; spec.seas_mode[1] = TSF_MODE_ADDITIVE;
    spec.seas_prior_scale[0] = spec.seas_prior_scale[1] = 10.0;
    spec.n_extra = 2;
    spec.extra_prior_scale[0] = spec.extra_prior_scale[1] = 10.0;
    spec.extra_mode[0] = TSF_MODE_ADDITIVE;
    spec.extra_mode[1] = TSF_MODE_MULTIPLICATIVE;
    const int K = tsf_spec_K(&spec), stride = tsf_theta_stride(&spec);
    if (K != 28) return 3;

    double *theta = slurp(dir, "theta.f64", sizeof(double) * (size_t)(N * stride));
    double *ys = slurp(dir, "ys.f64", sizeof(double) * (size_t)N);
    tsf_grid_info *grid = slurp(dir, "grid.bin", (size_t)tsf_grid_info_size() * (size_t)N);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * 2 * (size_t)H);

    /* design columns 0-19 yearly, 20-25 weekly, 26 the additive extra, 27 the multiplicative one */
    const uint64_t cols[3] = {((uint64_t)1 << 27) - 1, (uint64_t)1 << 26, (uint64_t)1 << 27};
    const int32_t scaled[3] = {1, 1, 0};
    const size_t nh = (size_t)(N * H);
    double *out = calloc(nh * 9, sizeof(double));
    if (!out) return 4;
    double *yhat = out, *trend = out + nh, *comp = out + 2 * nh, *iv = out + 5 * nh;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    int rc = tsf_predict_components(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, 3, cols,
                                    scaled, NULL, 200, 0.8, 5, yhat, trend, comp, iv, iv + nh, iv + 2 * nh, iv + 3 * nh);
    if (rc != 0) { fprintf(stderr, "tsf_predict_components: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* a table with a column at or above K is refused */
    const uint64_t bad = (uint64_t)1 << 28;
    if (tsf_predict_components(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, 1, &bad,
                               scaled, NULL, 0, 0.8, 5, yhat, trend, comp, NULL, NULL, NULL, NULL) >= 0) return 7;
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(out, sizeof(double), nh * 9, f) != nh * 9) return 8;
    fclose(f);
    free(out); free(theta); free(ys); free(grid); free(fut); free(extra);
    return 0;
}
