/* Plain C99 caller of the serially correlated observation noise through the C-ABI (include/tsf.h):
 * tsf_residual_autocorr on a tiny aligned panel, then tsf_predict_quantiles twice on models of tests/sampler_cases.py's
 * noise-only spec (linear growth, no changepoint, no seasonality, one additive extra column shared by the series) read
 * from raw binary files -- first behind tsf_set_noise_ar with the estimate, then without a setting -- no Python in the
 * process.  Levels 0.1, 0.5, 0.9 with the running sums; 50 samples, seed 5; the default estimator arguments.
 * Usage: abi_noise_ar N H T dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64 key.i64 y.f64 fitted.f64;
 * writes dir/out.f64: phi, phi_raw, scale [N], then per call (with the setting, without) yhat [N][H], q [N][3][H],
 * cum_q [N][3][H], samples [N][H][50]; and dir/ints.i64: n_pairs, status [N] each) */
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
    const int32_t T = atoi(argv[3]);
    const char *dir = argv[4];

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
    if (tsf_ar_args_size() != (int)sizeof(tsf_ar_args) || tsf_ar_out_size() != (int)sizeof(tsf_ar_out)) return 3;

    double *theta = slurp(dir, "theta.f64", sizeof(double) * (size_t)(N * stride));
    double *ys = slurp(dir, "ys.f64", sizeof(double) * (size_t)N);
    const size_t gsz = (size_t)tsf_grid_info_size();
    char *grid = slurp(dir, "grid.bin", gsz * (size_t)N);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *extra = slurp(dir, "extra.f64", sizeof(double) * (size_t)H);
    int64_t *key = slurp(dir, "key.i64", sizeof(int64_t) * (size_t)N);
    double *y = slurp(dir, "y.f64", sizeof(double) * (size_t)(N * T));
    double *fitted = slurp(dir, "fitted.f64", sizeof(double) * (size_t)(N * T));

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t n = (size_t)N, nh = (size_t)(N * H), per_call = nh * (1 + 2 * NQ + NS), total = 3 * n + 2 * per_call;
    double *buf = calloc(total, sizeof(double));
    int64_t *ints = calloc(2 * n, sizeof(int64_t));
    int32_t *status = calloc(n, sizeof(int32_t));
    if (!buf || !ints || !status) return 4;
    tsf_ar_out est;
    est.phi = buf;
    est.phi_raw = buf + n;
    est.scale = buf + 2 * n;
    est.n_pairs = ints;
    est.status = status;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    /* refused: phi_max of 1; no pairs asked for */
    tsf_ar_args bad_args;
    bad_args.phi_max = 1.0; bad_args.min_pairs = 8; bad_args.reserved_ = 0;
    if (tsf_residual_autocorr(ctx, N, T, NULL, y, TSF_Y_F64, fitted, &bad_args, &est) >= 0) return 7;
    bad_args.phi_max = 0.95; bad_args.min_pairs = 0;
    if (tsf_residual_autocorr(ctx, N, T, NULL, y, TSF_Y_F64, fitted, &bad_args, &est) >= 0) return 7;
    int rc = tsf_residual_autocorr(ctx, N, T, NULL, y, TSF_Y_F64, fitted, NULL, &est);
    if (rc != 0) { fprintf(stderr, "tsf_residual_autocorr: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    for (size_t i = 0; i < n; ++i) ints[n + i] = status[i];

    /* refused: an autocorrelation of 1; a setting for another number of series (and the setting is gone with it) */
    const double phi0 = est.phi[0];
    est.phi[0] = 1.0;
    if (tsf_set_noise_ar(ctx, est.phi, N) >= 0) return 7;
    est.phi[0] = phi0;
    tsf_quantile_out out;
    double *at = buf + 3 * n;
    for (int call = 0; call < 3; ++call) {
        /* call 0: a setting for N - 1 series, refused by the draw; 1: the estimate; 2: no setting */
        if (call < 2) {
            rc = tsf_set_noise_ar(ctx, est.phi, call == 0 ? N - 1 : N);
            if (rc != 0) { fprintf(stderr, "tsf_set_noise_ar: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
        }
        out.yhat = at;
        out.q = out.yhat + nh;
        out.cum_q = out.q + nh * NQ;
        out.trend_q = NULL;
        out.samples = out.cum_q + nh * NQ;
        out.trend_samples = NULL;
        rc = tsf_predict_quantiles(ctx, &spec, N, H, theta, ys, (const tsf_grid_info *)grid, (int32_t)N, fut, 1, NULL, NULL,
                                   extra, key, NS, 5, NQ, levels, &out);
        if (call == 0) {
            if (rc >= 0) return 7;
            continue;
        }
        if (rc != 0) { fprintf(stderr, "tsf_predict_quantiles: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
        at += per_call;
    }
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    snprintf(path, sizeof(path), "%s/ints.i64", dir);
    f = fopen(path, "wb");
    if (!f || fwrite(ints, sizeof(int64_t), 2 * n, f) != 2 * n) return 8;
    fclose(f);
    free(buf); free(ints); free(status); free(theta); free(ys); free(grid); free(fut); free(extra); free(key); free(y);
    free(fitted);
    return 0;
}
