/* Plain C99 caller of the correlated group roll-ups through the C-ABI (include/tsf.h): tsf_residual_corr on an aligned
 * panel of residuals, then tsf_rollup_create, tsf_rollup_set_noise_corr with the estimate, tsf_rollup_add,
 * tsf_rollup_quantiles, tsf_rollup_free on models of tests/sampler_cases.py's noise-only spec (linear growth, no
 * changepoint, no seasonality, one additive extra column shared by the series) read from raw binary files -- no Python
 * in the process.  Levels 0.1, 0.5, 0.9; 50 samples, seed 5; the default group keys and estimator arguments.
 * Usage: abi_rollup_corr N H G T dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64 key.i64 group.i64 y.f64
 * fitted.f64; writes dir/out.f64: rho, rho_raw [G], scale [N], yhat [G][H], q [G][3][H], samples [G][H][50]; and
 * dir/ints.i64: n_pairs, n_used, status, count [G] each) */
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
    if (argc != 6) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t H = atoi(argv[2]);
    const int64_t G = atoll(argv[3]);
    const int32_t T = atoi(argv[4]);
    const char *dir = argv[5];

    tsf_spec spec;
    tsf_spec_default(&spec);
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_changepoints = 0;
    spec.n_seas = 0;
    spec.n_extra = 1;
    spec.extra_prior_scale[0] = 10.0;
    spec.extra_mode[0] = TSF_MODE_ADDITIVE;
    const int stride = tsf_theta_stride(&spec);
    if (stride != 4) return 3;
    if (tsf_corr_args_size() != (int)sizeof(tsf_corr_args) || tsf_corr_out_size() != (int)sizeof(tsf_corr_out)) return 3;

    double *theta = slurp(dir, "theta.f64", sizeof(double) * (size_t)(N * stride));
    double *ys = slurp(dir, "ys.f64", sizeof(double) * (size_t)N);
    const size_t gsz = (size_t)tsf_grid_info_size();
    char *grid = slurp(dir, "grid.bin", gsz * (size_t)N);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * (size_t)H);
    int64_t *key = slurp(dir, "key.i64", sizeof(int64_t) * (size_t)N);
    int64_t *group = slurp(dir, "group.i64", sizeof(int64_t) * (size_t)N);
    double *y = slurp(dir, "y.f64", sizeof(double) * (size_t)(N * T));
    double *fitted = slurp(dir, "fitted.f64", sizeof(double) * (size_t)(N * T));

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t g = (size_t)G, gh = (size_t)(G * H), total = 2 * g + (size_t)N + gh * (1 + NQ + NS);
    double *buf = calloc(total, sizeof(double));
    int64_t *ints = calloc(4 * g, sizeof(int64_t));
    int32_t *n_used = calloc(g, sizeof(int32_t)), *status = calloc(g, sizeof(int32_t));
    if (!buf || !ints || !n_used || !status) return 4;
    tsf_corr_out est;
    est.rho = buf;
    est.rho_raw = buf + g;
    est.scale = buf + 2 * g;
    est.n_pairs = ints;
    est.n_used = n_used;
    est.status = status;
    tsf_rollup_out out;
    out.yhat = est.scale + N;
    out.count = ints + 3 * g;
    out.q = out.yhat + gh;
    out.cum_q = NULL;
    out.samples = out.q + gh * NQ;

    tsf_ctx *ctx = NULL;
    tsf_rollup *r = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    /* refused: a group value of G; rho_max above 1 */
    const int64_t g0 = group[0];
    group[0] = G;
    if (tsf_residual_corr(ctx, N, T, y, TSF_Y_F64, fitted, group, G, NULL, &est) >= 0) return 7;
    group[0] = g0;
    tsf_corr_args bad_args;
    bad_args.rho_max = 1.5; bad_args.min_rows = 8; bad_args.reserved_ = 0;
    if (tsf_residual_corr(ctx, N, T, y, TSF_Y_F64, fitted, group, G, &bad_args, &est) >= 0) return 7;
    int rc = tsf_residual_corr(ctx, N, T, y, TSF_Y_F64, fitted, group, G, NULL, &est);
    if (rc != 0) { fprintf(stderr, "tsf_residual_corr: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    for (size_t i = 0; i < g; ++i) { ints[g + i] = n_used[i]; ints[2 * g + i] = status[i]; }

    if (tsf_rollup_create(ctx, G, H, fut, NS, 5, &r) != 0) { fprintf(stderr, "create: %s\n", tsf_last_error(ctx)); return 6; }
    /* refused: a correlation above 1 */
    const double rho0 = est.rho[0];
    est.rho[0] = 1.25;
    if (tsf_rollup_set_noise_corr(r, est.rho, NULL) >= 0) return 7;
    est.rho[0] = rho0;
    rc = tsf_rollup_set_noise_corr(r, est.rho, NULL);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_set_noise_corr: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    rc = tsf_rollup_add(r, &spec, N, theta, ys, (const tsf_grid_info *)grid, (int32_t)N, NULL, NULL, extra, 1, key, group);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_add: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: a correlation once something has been added; a total on a correlated handle */
    if (tsf_rollup_set_noise_corr(r, est.rho, NULL) >= 0) return 7;
    if (tsf_rollup_set_totals(r, &spec, 1, theta, ys, (const tsf_grid_info *)grid, 1, NULL, NULL, extra, 1, key, group) >= 0)
        return 7;
    rc = tsf_rollup_quantiles(r, NQ, levels, &out);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_quantiles: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_rollup_free(r);
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    snprintf(path, sizeof(path), "%s/ints.i64", dir);
    f = fopen(path, "wb");
    if (!f || fwrite(ints, sizeof(int64_t), 4 * g, f) != 4 * g) return 8;
    fclose(f);
    free(buf); free(ints); free(n_used); free(status); free(theta); free(ys); free(grid); free(fut); free(extra); free(key);
    free(group); free(y); free(fitted);
    return 0;
}
