/* Plain C99 caller of the window entries through the C-ABI (include/tsf.h, "totals over row windows"):
 * tsf_predict_windows on the models of tests/forecast_cases.py case iv129 (linear growth, yearly order 10 + weekly
 * order 3 additive, one additive and one multiplicative extra column, 60 changepoints, a shared future grid) read from
 * raw binary files, then tsf_rollup_windows on a roll-up of the same models into one group -- no Python in the process.
 * Levels 0.1, 0.5, 0.9; 50 samples, seed 5; every output requested.
 * Usage: abi_windows N H K dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64 key.i64 w0.i32 w1.i32
 * ywin.f64 [N][K] gwin.f64 [1][K]; writes dir/out.f64: per entry (the series, then the one group) yhat [n][H], total,
 * pit, crps [n][K] each, q, pinball [n][3][K] each, mean_crps [n], mean_pinball, coverage [n][3] each, then n_obs [n]
 * as doubles) */
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

/* the doubles one entry returns for n series (groups) */
static size_t block(size_t n, size_t H, size_t K) { return n * H + n * K * (3 + 2 * NQ) + n * (1 + 2 * NQ) + n; }

static void carve(tsf_window_out *o, double *buf, size_t n, size_t H, size_t K, int32_t *n_obs)
{
    o->yhat = buf;
    o->total = o->yhat + n * H;
    o->pit = o->total + n * K;
    o->crps = o->pit + n * K;
    o->q = o->crps + n * K;
    o->pinball = o->q + n * K * NQ;
    o->mean_crps = o->pinball + n * K * NQ;
    o->mean_pinball = o->mean_crps + n;
    o->coverage = o->mean_pinball + n * NQ;
    o->n_obs = n_obs;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t H = atoi(argv[2]);
    const int32_t K = atoi(argv[3]);
    const char *dir = argv[4];

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
    if (tsf_window_out_size() != (int)sizeof(tsf_window_out)) return 3;
    if (K < 1 || K > TSF_MAX_WINDOWS) return 3;

    double *theta = slurp(dir, "theta.f64", sizeof(double) * (size_t)(N * stride));
    double *ys = slurp(dir, "ys.f64", sizeof(double) * (size_t)N);
    tsf_grid_info *grid = slurp(dir, "grid.bin", (size_t)tsf_grid_info_size() * (size_t)N);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * 2 * (size_t)H);
    int64_t *key = slurp(dir, "key.i64", sizeof(int64_t) * (size_t)N);
    int32_t *w0 = slurp(dir, "w0.i32", sizeof(int32_t) * (size_t)K);
    int32_t *w1 = slurp(dir, "w1.i32", sizeof(int32_t) * (size_t)K);
    double *ywin = slurp(dir, "ywin.f64", sizeof(double) * (size_t)(N * K));
    double *gwin = slurp(dir, "gwin.f64", sizeof(double) * (size_t)K);

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t n = (size_t)N, first = block(n, (size_t)H, (size_t)K), total = first + block(1, (size_t)H, (size_t)K);
    double *buf = calloc(total, sizeof(double));
    int32_t *n_obs = calloc(n + 1, sizeof(int32_t));
    int64_t *group = calloc(n, sizeof(int64_t));            /* every series in group 0 */
    if (!buf || !n_obs || !group) return 4;
    tsf_window_out out, gout, none;
    carve(&out, buf, n, (size_t)H, (size_t)K, n_obs);
    carve(&gout, buf + first, 1, (size_t)H, (size_t)K, n_obs + n);
    memset(&none, 0, sizeof(none));

    tsf_ctx *ctx = NULL;
    tsf_rollup *r = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    int rc = tsf_predict_windows(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, key, NS, 5, K, w0,
                                 w1, ywin, NQ, levels, &out);
    if (rc != 0) { fprintf(stderr, "tsf_predict_windows: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    for (size_t i = 0; i < n; ++i) (out.coverage + n * NQ)[i] = (double)n_obs[i];
    /* refused: a level outside [0, 1], a call that wants nothing, a score output without y_win, no windows, a window
     * that ends behind the rows */
    const double bad[1] = {1.5};
    if (tsf_predict_windows(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, key, NS, 5, K, w0, w1,
                            ywin, 1, bad, &out) >= 0) return 7;
    if (tsf_predict_windows(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, key, NS, 5, K, w0, w1,
                            ywin, NQ, levels, &none) >= 0) return 7;
    if (tsf_predict_windows(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, key, NS, 5, K, w0, w1,
                            NULL, NQ, levels, &out) >= 0) return 7;
    if (tsf_predict_windows(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, key, NS, 5, 0, w0, w1,
                            ywin, NQ, levels, &out) >= 0) return 7;
    const int32_t a0[1] = {0}, a1[1] = {0};
    int32_t past[1];
    past[0] = H + 1;
    if (tsf_predict_windows(ctx, &spec, N, H, theta, ys, grid, (int32_t)N, fut, 1, NULL, NULL, extra, key, NS, 5, 1, a0, past,
                            ywin, NQ, levels, &out) >= 0) return 7;

    if (tsf_rollup_create(ctx, 1, H, fut, NS, 5, &r) != 0) { fprintf(stderr, "create: %s\n", tsf_last_error(ctx)); return 6; }
    rc = tsf_rollup_add(r, &spec, N, theta, ys, grid, (int32_t)N, NULL, NULL, extra, 1, key, group);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_add: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: an empty window, a call that wants nothing */
    if (tsf_rollup_windows(r, 1, a0, a1, NULL, NQ, levels, &gout) >= 0) return 7;
    if (tsf_rollup_windows(r, K, w0, w1, gwin, NQ, levels, &none) >= 0) return 7;
    rc = tsf_rollup_windows(r, K, w0, w1, gwin, NQ, levels, &gout);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_windows: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    (gout.coverage + NQ)[0] = (double)n_obs[n];
    tsf_rollup_free(r);
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    free(buf); free(n_obs); free(group); free(theta); free(ys); free(grid); free(fut); free(extra); free(key);
    free(w0); free(w1); free(ywin); free(gwin);
    return 0;
}
