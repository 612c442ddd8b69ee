/* Plain C99 caller of the group roll-ups through the C-ABI (include/tsf.h): tsf_rollup_create, tsf_rollup_add twice
 * (series [0, N / 2) and [N / 2, N)), tsf_rollup_quantiles, tsf_rollup_free on models of tests/forecast_cases.py case
 * iv129's spec (linear growth, yearly order 10 + weekly order 3 additive, one additive and one multiplicative extra
 * column shared by the series, 60 changepoints) read from raw binary files -- no Python in the process.
 * Levels 0.1, 0.5, 0.9; 50 samples, seed 5; every output requested.
 * Usage: abi_rollup N H G dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64 key.i64 group.i64; writes
 * dir/out.f64: yhat [G][H], q, cum_q [G][3][H] each, samples [G][H][50]; and dir/count.i64 [G]) */
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
    if (argc != 5) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t H = atoi(argv[2]);
    const int64_t G = atoll(argv[3]);
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

    double *theta = slurp(dir, "theta.f64", sizeof(double) * (size_t)(N * stride));
    double *ys = slurp(dir, "ys.f64", sizeof(double) * (size_t)N);
    const size_t gsz = (size_t)tsf_grid_info_size();
    char *grid = slurp(dir, "grid.bin", gsz * (size_t)N);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * 2 * (size_t)H);
    int64_t *key = slurp(dir, "key.i64", sizeof(int64_t) * (size_t)N);
    int64_t *group = slurp(dir, "group.i64", sizeof(int64_t) * (size_t)N);

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t gh = (size_t)(G * H), total = gh * (1 + 2 * NQ + NS);
    double *buf = calloc(total, sizeof(double));
    int64_t *count = calloc((size_t)G, sizeof(int64_t));
    if (!buf || !count) return 4;
    tsf_rollup_out out;
    out.yhat = buf;
    out.count = count;
    out.q = buf + gh;
    out.cum_q = out.q + gh * NQ;
    out.samples = out.cum_q + gh * NQ;

    tsf_ctx *ctx = NULL;
    tsf_rollup *r = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    /* refused: no groups, one sample */
    if (tsf_rollup_create(ctx, 0, H, fut, NS, 5, &r) >= 0 || r) return 7;
    if (tsf_rollup_create(ctx, G, H, fut, 1, 5, &r) >= 0 || r) return 7;
    if (tsf_rollup_create(ctx, G, H, fut, NS, 5, &r) != 0) { fprintf(stderr, "create: %s\n", tsf_last_error(ctx)); return 6; }
    /* refused: no keys; a group index of G */
    if (tsf_rollup_add(r, &spec, N, theta, ys, (const tsf_grid_info *)grid, (int32_t)N, NULL, NULL, extra, 1, NULL, group) >= 0)
        return 7;
    const int64_t g0 = group[0];
    group[0] = G;
    if (tsf_rollup_add(r, &spec, N, theta, ys, (const tsf_grid_info *)grid, (int32_t)N, NULL, NULL, extra, 1, key, group) >= 0)
        return 7;
    group[0] = g0;
    const int64_t half = N / 2;
    int rc = tsf_rollup_add(r, &spec, half, theta, ys, (const tsf_grid_info *)grid, (int32_t)half, NULL, NULL, extra, 1,
                            key, group);
    if (rc == 0)
        rc = tsf_rollup_add(r, &spec, N - half, theta + half * stride, ys + half,
                            (const tsf_grid_info *)(grid + gsz * (size_t)half), (int32_t)(N - half), NULL, NULL, extra, 1,
                            key + half, group + half);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_add: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: a level outside [0, 1]; an output set that wants nothing */
    const double bad[1] = {1.5};
    if (tsf_rollup_quantiles(r, 1, bad, &out) >= 0) return 7;
    tsf_rollup_out none;
    memset(&none, 0, sizeof(none));
    none.yhat = buf;
    none.count = count;
    if (tsf_rollup_quantiles(r, NQ, levels, &none) >= 0) return 7;
    rc = tsf_rollup_quantiles(r, NQ, levels, &out);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_quantiles: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_rollup_free(r);
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    snprintf(path, sizeof(path), "%s/count.i64", dir);
    f = fopen(path, "wb");
    if (!f || fwrite(count, sizeof(int64_t), (size_t)G, f) != (size_t)G) return 8;
    fclose(f);
    free(buf); free(count); free(theta); free(ys); free(grid); free(fut); free(extra); free(key); free(group);
    return 0;
}
