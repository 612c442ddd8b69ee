/* Plain C99 caller of the calibration entries through the C-ABI (include/tsf.h): tsf_calibrate_rows on a ragged set of
 * rows read from raw binary files, tsf_apply_calibration of that table on a forecast, then tsf_calibrate (linear growth,
 * weekly order 3 additive; horizon 20 d, period 10 d, initial 100 d) on an aligned panel -- no Python in the process.
 * Levels 0.8 and 0.95, TSF_CALIB_ABS, 4 buckets, min_scores 5.
 * Usage: abi_calibrate N T H dir   (dir holds off.i64 [N+1], h.i64, y.f64, yhat.f64 [off[N]]; fut.i64 [H], origin.i64
 * [N], fyhat.f64 [N][H]; ds.i64 [T], panel.f64 [N][T]; writes dir/out.f64, everything as doubles: the rule's q, n
 * [N][5][2], status [N]; apply's lo, hi, cell [N][2][H]; tsf_calibrate's q, n [N][5][2], status [N]) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tsf.h"

#define DAY_NS 86400000000000LL

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

static double *put_f64(double *at, const double *v, size_t n) { memcpy(at, v, n * sizeof(double)); return at + n; }
static double *put_i32(double *at, const int32_t *v, size_t n) { for (size_t i = 0; i < n; ++i) at[i] = (double)v[i]; return at + n; }
static double *put_i8(double *at, const int8_t *v, size_t n) { for (size_t i = 0; i < n; ++i) at[i] = (double)v[i]; return at + n; }

static void table_alloc(tsf_calib_table *t, size_t n, size_t cells)
{
    t->q = calloc(n * cells, sizeof(double));
    t->n = calloc(n * cells, sizeof(int32_t));
    t->status = calloc(n, sizeof(int32_t));
    if (!t->q || !t->n || !t->status) exit(4);
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t T = atoi(argv[2]), H = atoi(argv[3]);
    const char *dir = argv[4];
    const size_t n = (size_t)N, cells = 5 * 2, nlh = n * 2 * (size_t)H;

    if (tsf_calib_args_size() != (int)sizeof(tsf_calib_args) || tsf_calib_table_size() != (int)sizeof(tsf_calib_table))
        return 3;

    int64_t *off = slurp(dir, "off.i64", sizeof(int64_t) * (n + 1));
    const size_t R = (size_t)off[N];
    int64_t *h = slurp(dir, "h.i64", sizeof(int64_t) * R);
    double *y = slurp(dir, "y.f64", sizeof(double) * R);
    double *yhat = slurp(dir, "yhat.f64", sizeof(double) * R);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    int64_t *origin = slurp(dir, "origin.i64", sizeof(int64_t) * n);
    double *fyhat = slurp(dir, "fyhat.f64", sizeof(double) * n * (size_t)H);
    int64_t *ds = slurp(dir, "ds.i64", sizeof(int64_t) * (size_t)T);
    double *panel = slurp(dir, "panel.f64", sizeof(double) * n * (size_t)T);

    tsf_calib_args args;
    memset(&args, 0, sizeof(args));
    args.mode = TSF_CALIB_ABS; args.n_levels = 2; args.levels[0] = 0.8; args.levels[1] = 0.95;
    args.horizon_ns = 20 * DAY_NS; args.n_buckets = 4; args.min_scores = 5;
    tsf_calib_table rule, one;
    table_alloc(&rule, n, cells);
    table_alloc(&one, n, cells);

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    int rc = tsf_calibrate_rows(ctx, N, off, h, y, yhat, NULL, NULL, &args, &rule);
    if (rc != 0) { fprintf(stderr, "tsf_calibrate_rows: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* a level of 1, CQR without bounds, a NULL yhat and a NULL status are refused; no series is a no-op */
    tsf_calib_args bad = args;
    bad.levels[1] = 1.0;
    if (tsf_calibrate_rows(ctx, N, off, h, y, yhat, NULL, NULL, &bad, &rule) >= 0) return 7;
    bad = args;
    bad.mode = TSF_CALIB_CQR;
    if (tsf_calibrate_rows(ctx, N, off, h, y, yhat, NULL, NULL, &bad, &rule) >= 0) return 7;
    if (tsf_calibrate_rows(ctx, N, off, h, y, NULL, NULL, NULL, &args, &rule) >= 0) return 7;
    tsf_calib_table none = rule;
    none.status = NULL;
    if (tsf_calibrate_rows(ctx, N, off, h, y, yhat, NULL, NULL, &args, &none) >= 0) return 7;
    if (tsf_calibrate_rows(ctx, 0, off, h, y, yhat, NULL, NULL, &args, &rule) != 0) return 7;

    double *lo = calloc(nlh, sizeof(double)), *hi = calloc(nlh, sizeof(double));
    int8_t *cell = calloc(nlh, 1);
    if (!lo || !hi || !cell) return 4;
    rc = tsf_apply_calibration(ctx, N, H, fyhat, NULL, NULL, fut, 1, origin, rule.q, rule.n, &args, lo, hi, cell);
    if (rc != 0) { fprintf(stderr, "tsf_apply_calibration: %d %s\n", rc, tsf_last_error(ctx)); return 6; }

    tsf_spec spec;
    tsf_spec_default(&spec);
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_seas = 1;
    spec.seas_period[0] = 7.0; spec.seas_order[0] = 3; spec.seas_mode[0] = TSF_MODE_ADDITIVE;
    spec.seas_prior_scale[0] = 10.0;
    tsf_cv_args cv;
    cv.horizon_ns = 20 * DAY_NS; cv.period_ns = 10 * DAY_NS; cv.initial_ns = 100 * DAY_NS; cv.rolling_window = 0.1;
    bad = args;
    bad.horizon_ns = 19 * DAY_NS;           /* not the cross-validation's horizon */
    if (tsf_calibrate(ctx, &spec, N, T, NULL, ds, panel, TSF_Y_F64, NULL, NULL, NULL, &cv, NULL, 0, 0.8, 0, &bad, &one, NULL) >= 0)
        return 7;
    rc = tsf_calibrate(ctx, &spec, N, T, NULL, ds, panel, TSF_Y_F64, NULL, NULL, NULL, &cv, NULL, 0, 0.8, 0, &args, &one, NULL);
    if (rc != 0) { fprintf(stderr, "tsf_calibrate: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_destroy(ctx);

    const size_t total = 2 * (2 * n * cells + n) + 3 * nlh;
    double *buf = calloc(total, sizeof(double));
    if (!buf) return 4;
    double *at = buf;
    at = put_f64(at, rule.q, n * cells); at = put_i32(at, rule.n, n * cells); at = put_i32(at, rule.status, n);
    at = put_f64(at, lo, nlh); at = put_f64(at, hi, nlh); at = put_i8(at, cell, nlh);
    at = put_f64(at, one.q, n * cells); at = put_i32(at, one.n, n * cells); at = put_i32(at, one.status, n);
    if ((size_t)(at - buf) != total) return 9;

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    return 0;
}
