/* Plain C99 caller of the scoring entry through the C-ABI (include/tsf.h): tsf_score_actuals on the model of
 * tests/forecast_cases.py case iv129 (linear growth, yearly order 10 + weekly order 3 additive, one additive and one
 * multiplicative extra column, 60 changepoints, a shared future grid) read from raw binary files -- no Python in the
 * process.  Levels 0.1, 0.5, 0.9; 50 samples, seed 5, series_key NULL; every output requested.
 * Usage: abi_scores N H dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64 yobs.f64; writes dir/out.f64:
 * yhat, pit, crps [N][H] each, q, pinball [N][3][H] each, mean_crps [N], mean_pinball, coverage [N][3] each, then n_obs
 * [N] as doubles) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tsf.h"

#define NQ 3
#define NS 50

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
    const int stride = tsf_theta_stride(&spec);
    if (tsf_spec_K(&spec) != 28) return 3;
    if (tsf_score_out_size() != (int)sizeof(tsf_score_out)) return 3;

    double *theta = slurp(dir, "theta.f64", sizeof(double) * (size_t)(N * stride));
    double *ys = slurp(dir, "ys.f64", sizeof(double) * (size_t)N);
    tsf_grid_info *grid = slurp(dir, "grid.bin", (size_t)tsf_grid_info_size() * (size_t)N);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * 2 * (size_t)H);
    double *yobs = slurp(dir, "yobs.f64", sizeof(double) * (size_t)(N * H));

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t nh = (size_t)(N * H), n = (size_t)N;
    const size_t total = nh * (3 + 2 * NQ) + n * (1 + 2 * NQ) + n;
    double *buf = calloc(total, sizeof(double));
    int32_t *n_obs = calloc(n, sizeof(int32_t));
    if (!buf || !n_obs) return 4;
    tsf_score_out out;
    out.yhat = buf;
    out.pit = out.yhat + nh;
    out.crps = out.pit + nh;
    out.q = out.crps + nh;
    out.pinball = out.q + nh * NQ;
    out.mean_crps = out.pinball + nh * NQ;
    out.mean_pinball = out.mean_crps + n;
    out.coverage = out.mean_pinball + n * NQ;
    out.n_obs = n_obs;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    int rc = tsf_score_actuals(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, NULL, NS, 5, yobs,
                               NQ, levels, &out);
    if (rc != 0) { fprintf(stderr, "tsf_score_actuals: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    for (size_t i = 0; i < n; ++i) (out.coverage + n * NQ)[i] = (double)n_obs[i];
    /* a level outside [0, 1], a call that wants nothing and a NULL y_obs are refused; no series is a no-op */
    const double bad[1] = {1.5};
    if (tsf_score_actuals(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, NULL, NS, 5, yobs, 1, bad,
                          &out) >= 0) return 7;
    tsf_score_out none;
    memset(&none, 0, sizeof(none));
    none.yhat = buf;
    if (tsf_score_actuals(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, NULL, NS, 5, yobs, NQ,
                          levels, &none) >= 0) return 7;
    if (tsf_score_actuals(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, NULL, NS, 5, NULL, NQ,
                          levels, &out) >= 0) return 7;
    if (tsf_score_actuals(ctx, &spec, 0, H, theta, ys, grid, 1, fut, 1, NULL, NULL, extra, NULL, NS, 5, yobs, NQ, levels,
                          &out) != 0) return 7;
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    free(buf); free(n_obs); free(theta); free(ys); free(grid); free(fut); free(extra); free(yobs);
    return 0;
}
