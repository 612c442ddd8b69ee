/* Plain C99 caller of the screening entries through the C-ABI (include/tsf.h): tsf_screen_rows on an aligned panel
 * (y, fitted) read from raw binary files, then tsf_fit_screened (linear growth, weekly order 3 additive, two passes) on
 * the same y -- no Python in the process.  threshold 5, max_share 0.1, min_rows 10, scale_floor_rel 1e-8.
 * Usage: abi_screen N T dir   (dir holds ds.i64 [T], y.f64 [N][T], fitted.f64 [N][T]; writes dir/out.f64, everything as
 * doubles: the rule's flag, resid [N][T], center, scale, n_new, n_flagged, status [N]; then fit_screened's fit.theta
 * [N][stride], fit.y_scale, fit.status, fit.n_iter [N], first.theta [N][stride], screen.flag [N][T], screen.n_flagged,
 * rounds [N]; and dir/grid.bin: fit.grid [N]) */
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

static void fit_out_alloc(tsf_fit_out *o, size_t n, size_t stride, size_t n_grids)
{
    o->theta = calloc(n * stride, sizeof(double));
    o->y_scale = calloc(n, sizeof(double));
    o->fval = calloc(n, sizeof(double));
    o->status = calloc(n, sizeof(int32_t));
    o->n_iter = calloc(n, sizeof(int32_t));
    o->n_eval = calloc(n, sizeof(int32_t));
    o->grid = calloc(n_grids, sizeof(tsf_grid_info));
    if (!o->theta || !o->y_scale || !o->fval || !o->status || !o->n_iter || !o->n_eval || !o->grid) exit(4);
}

static void screen_out_alloc(tsf_screen_out *o, size_t n, size_t rows)
{
    o->flag = calloc(rows, 1);
    o->resid = calloc(rows, sizeof(double));
    o->center = calloc(n, sizeof(double));
    o->scale = calloc(n, sizeof(double));
    o->n_new = calloc(n, sizeof(int32_t));
    o->n_flagged = calloc(n, sizeof(int32_t));
    o->status = calloc(n, sizeof(int32_t));
    if (!o->flag || !o->resid || !o->center || !o->scale || !o->n_new || !o->n_flagged || !o->status) exit(4);
}

static double *put_f64(double *at, const double *v, size_t n) { memcpy(at, v, n * sizeof(double)); return at + n; }
static double *put_i32(double *at, const int32_t *v, size_t n) { for (size_t i = 0; i < n; ++i) at[i] = (double)v[i]; return at + n; }
static double *put_u8(double *at, const uint8_t *v, size_t n) { for (size_t i = 0; i < n; ++i) at[i] = (double)v[i]; return at + n; }

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t T = atoi(argv[2]);
    const char *dir = argv[3];
    const size_t n = (size_t)N, rows = (size_t)(N * T);

    tsf_spec spec;
    tsf_spec_default(&spec);
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_seas = 1;
    spec.seas_period[0] = 7.0; spec.seas_order[0] = 3; spec.seas_mode[0] = TSF_MODE_ADDITIVE;
    spec.seas_prior_scale[0] = 10.0;
    const size_t stride = (size_t)tsf_theta_stride(&spec);
    if (tsf_spec_K(&spec) != 6) return 3;
    if (tsf_screen_args_size() != (int)sizeof(tsf_screen_args) || tsf_screen_out_size() != (int)sizeof(tsf_screen_out) ||
        tsf_fit_screened_out_size() != (int)sizeof(tsf_fit_screened_out))
        return 3;

    int64_t *ds = slurp(dir, "ds.i64", sizeof(int64_t) * (size_t)T);
    double *y = slurp(dir, "y.f64", sizeof(double) * rows);
    double *fitted = slurp(dir, "fitted.f64", sizeof(double) * rows);

    tsf_screen_args args;
    args.threshold = 5.0; args.max_share = 0.1; args.min_rows = 10; args.max_passes = 1;
    tsf_screen_out so;
    screen_out_alloc(&so, n, rows);

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    int rc = tsf_screen_rows(ctx, N, T, NULL, y, TSF_Y_F64, fitted, NULL, NULL, &args, &so);
    if (rc != 0) { fprintf(stderr, "tsf_screen_rows: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* a share above one half, a NULL fitted and a NULL status are refused; no series is a no-op */
    tsf_screen_args bad = args;
    bad.max_share = 0.75;
    if (tsf_screen_rows(ctx, N, T, NULL, y, TSF_Y_F64, fitted, NULL, NULL, &bad, &so) >= 0) return 7;
    if (tsf_screen_rows(ctx, N, T, NULL, y, TSF_Y_F64, NULL, NULL, NULL, &args, &so) >= 0) return 7;
    tsf_screen_out none = so;
    none.status = NULL;
    if (tsf_screen_rows(ctx, N, T, NULL, y, TSF_Y_F64, fitted, NULL, NULL, &args, &none) >= 0) return 7;
    if (tsf_screen_rows(ctx, 0, T, NULL, y, TSF_Y_F64, fitted, NULL, NULL, &args, &so) != 0) return 7;

    tsf_fit_out first;
    tsf_fit_screened_out fs;
    memset(&fs, 0, sizeof(fs));
    fit_out_alloc(&fs.fit, n, stride, n);
    fit_out_alloc(&first, n, stride, 1);
    fs.first = &first;
    screen_out_alloc(&fs.screen, n, rows);
    fs.rounds = calloc(n, sizeof(int32_t));
    if (!fs.rounds) return 4;
    args.max_passes = 2;
    rc = tsf_fit_screened(ctx, &spec, N, T, NULL, ds, y, TSF_Y_F64, NULL, NULL, NULL, 1e-8, &args, &fs);
    if (rc != 0) { fprintf(stderr, "tsf_fit_screened: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_destroy(ctx);

    const size_t total = 2 * rows + 5 * n + n * stride + 3 * n + n * stride + rows + 2 * n;
    double *buf = calloc(total, sizeof(double));
    if (!buf) return 4;
    double *at = buf;
    at = put_u8(at, so.flag, rows); at = put_f64(at, so.resid, rows);
    at = put_f64(at, so.center, n); at = put_f64(at, so.scale, n);
    at = put_i32(at, so.n_new, n); at = put_i32(at, so.n_flagged, n); at = put_i32(at, so.status, n);
    at = put_f64(at, fs.fit.theta, n * stride); at = put_f64(at, fs.fit.y_scale, n);
    at = put_i32(at, fs.fit.status, n); at = put_i32(at, fs.fit.n_iter, n);
    at = put_f64(at, first.theta, n * stride);
    at = put_u8(at, fs.screen.flag, rows); at = put_i32(at, fs.screen.n_flagged, n); at = put_i32(at, fs.rounds, n);
    if ((size_t)(at - buf) != total) return 9;

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    snprintf(path, sizeof(path), "%s/grid.bin", dir);
    f = fopen(path, "wb");
    if (!f || fwrite(fs.fit.grid, sizeof(tsf_grid_info), n, f) != n) return 8;
    fclose(f);
    return 0;
}
