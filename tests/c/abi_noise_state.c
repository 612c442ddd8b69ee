/* Plain C99 caller of the noise state of a fitted panel through the C-ABI (include/tsf.h): tsf_noise_state on a small
 * aligned panel and its fit (linear growth, 25 automatic changepoints, a weekly seasonality of order 3, one additive
 * explicit column), both read from raw binary files, then tsf_predict_conditioned from what it returned (steps =
 * last_gap + 1) -- no Python in the process.  The default estimator arguments.
 * Usage: abi_noise_state N T H stride dir   (dir holds theta.f64 ys.f64 grid.bin status.i32 ds.i64 y.f64 extra.f64
 * fut.i64 extra_fut.f64 floor.f64; writes dir/out.f64: phi, phi_raw, scale, last_resid [N], yhat [N][H]; dir/out.i64:
 * n_pairs, last_ds_ns [N]; dir/out.i32: status, last_gap, last_status [N], yhat_int [N][H]) */
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

static int dump(const char *dir, const char *name, const void *p, size_t bytes)
{
    char path[4096];
    snprintf(path, sizeof(path), "%s/%s", dir, name);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) return 8;
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t T = atoi(argv[2]);
    const int32_t H = atoi(argv[3]);
    const int want_stride = atoi(argv[4]);
    const char *dir = argv[5];

    tsf_spec spec;
    tsf_spec_default(&spec);
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_seas = 1;
    spec.seas_period[0] = 7.0;
    spec.seas_order[0] = 3;
    spec.seas_prior_scale[0] = 10.0;
    spec.seas_mode[0] = TSF_MODE_ADDITIVE;
    spec.n_extra = 1;
    spec.extra_prior_scale[0] = 10.0;
    spec.extra_mode[0] = TSF_MODE_ADDITIVE;
    const int stride = tsf_theta_stride(&spec);
    if (stride != want_stride) return 3;
    if (tsf_noise_state_out_size() != (int)sizeof(tsf_noise_state_out)) return 3;

    const size_t n = (size_t)N, nt = (size_t)(N * T), nh = (size_t)(N * H);
    double *theta = slurp(dir, "theta.f64", sizeof(double) * n * (size_t)stride);
    double *ys = slurp(dir, "ys.f64", sizeof(double) * n);
    tsf_grid_info *grid = slurp(dir, "grid.bin", (size_t)tsf_grid_info_size());
    int32_t *status = slurp(dir, "status.i32", sizeof(int32_t) * n);
    int64_t *ds = slurp(dir, "ds.i64", sizeof(int64_t) * (size_t)T);
    double *y = slurp(dir, "y.f64", sizeof(double) * nt);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * (size_t)T);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra_fut = slurp(dir, "extra_fut.f64", sizeof(double) * (size_t)H);
    double *floor_ = slurp(dir, "floor.f64", sizeof(double) * n);

    double *f64 = calloc(4 * n + nh, sizeof(double));
    int64_t *i64 = calloc(2 * n, sizeof(int64_t));
    int32_t *i32 = calloc(3 * n + nh, sizeof(int32_t));
    int32_t *steps = calloc(n, sizeof(int32_t));
    if (!f64 || !i64 || !i32 || !steps) return 4;
    tsf_noise_state_out out;
    out.phi = f64;
    out.phi_raw = f64 + n;
    out.scale = f64 + 2 * n;
    out.last_resid = f64 + 3 * n;
    out.n_pairs = i64;
    out.last_ds_ns = i64 + n;
    out.status = i32;
    out.last_gap = i32 + n;
    out.last_status = i32 + 2 * n;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    /* refused: a required output missing; a bad dtype; the explicit column missing; N = 0 is a no-op */
    out.last_gap = NULL;
    if (tsf_noise_state(ctx, &spec, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, extra, theta, ys, grid, 1, status, NULL, NULL,
                        &out) >= 0) return 7;
    out.last_gap = i32 + n;
    if (tsf_noise_state(ctx, &spec, N, T, NULL, ds, y, 7, NULL, NULL, extra, theta, ys, grid, 1, status, NULL, NULL, &out) >= 0)
        return 7;
    if (tsf_noise_state(ctx, &spec, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, NULL, theta, ys, grid, 1, status, NULL, NULL,
                        &out) >= 0) return 7;
    if (tsf_noise_state(ctx, &spec, 0, T, NULL, NULL, NULL, TSF_Y_F64, NULL, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL, NULL,
                        &out) != 0) return 7;
    int rc = tsf_noise_state(ctx, &spec, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, extra, theta, ys, grid, 1, status, NULL,
                             NULL, &out);
    if (rc != 0) { fprintf(stderr, "tsf_noise_state: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    for (size_t i = 0; i < n; ++i) steps[i] = out.last_gap[i] + 1;

    double *yhat = f64 + 4 * n;
    int32_t *yhat_int = i32 + 3 * n;
    /* refused: a step count of 0 */
    steps[0] = 0;
    if (tsf_predict_conditioned(ctx, &spec, N, H, theta, ys, grid, 1, fut, 1, floor_, NULL, extra_fut, out.phi, out.last_resid,
                                steps, yhat, yhat_int) >= 0) return 7;
    steps[0] = out.last_gap[0] + 1;
    rc = tsf_predict_conditioned(ctx, &spec, N, H, theta, ys, grid, 1, fut, 1, floor_, NULL, extra_fut, out.phi,
                                 out.last_resid, steps, yhat, yhat_int);
    if (rc != 0) { fprintf(stderr, "tsf_predict_conditioned: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_destroy(ctx);

    if (dump(dir, "out.f64", f64, sizeof(double) * (4 * n + nh))) return 8;
    if (dump(dir, "out.i64", i64, sizeof(int64_t) * 2 * n)) return 8;
    if (dump(dir, "out.i32", i32, sizeof(int32_t) * (3 * n + nh))) return 8;
    free(f64); free(i64); free(i32); free(steps); free(theta); free(ys); free(grid); free(status); free(ds); free(y);
    free(extra); free(fut); free(extra_fut); free(floor_);
    return 0;
}
