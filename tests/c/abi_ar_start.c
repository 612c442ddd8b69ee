/* Plain C99 caller of the conditioned start of the AR(1) noise chain through the C-ABI (include/tsf.h):
 * tsf_residual_autocorr and tsf_residual_last on a tiny aligned panel, tsf_noise_ar_mean, then tsf_predict_quantiles
 * twice on models of tests/sampler_cases.py's noise-only spec (linear growth, no changepoint, no seasonality, one
 * additive extra column shared by the series) read from raw binary files -- first behind tsf_set_noise_ar and
 * tsf_set_noise_ar_start (steps = last_gap + 1), then without a setting -- no Python in the process.  Levels 0.1, 0.5,
 * 0.9 with the running sums; 50 samples, seed 5; the default estimator arguments.
 * Usage: abi_ar_start N H T dir   (dir holds theta.f64 ys.f64 grid.bin fut.i64 extra.f64 key.i64 y.f64 fitted.f64;
 * writes dir/out.f64: phi, last_resid [N], mean [N][H], then per call (with the settings, without) yhat [N][H],
 * q [N][3][H], cum_q [N][3][H], samples [N][H][50]; and dir/ints.i32: last_gap, status of tsf_residual_last, steps [N]
 * each) */
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
    if (tsf_ar_last_out_size() != (int)sizeof(tsf_ar_last_out)) return 3;

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
    const size_t n = (size_t)N, nh = (size_t)(N * H), per_call = nh * (1 + 2 * NQ + NS), total = 2 * n + nh + 2 * per_call;
    double *buf = calloc(total, sizeof(double));
    int32_t *ints = calloc(3 * n, sizeof(int32_t));
    int32_t *est_status = calloc(n, sizeof(int32_t));
    if (!buf || !ints || !est_status) return 4;
    double *phi = buf, *last_resid = buf + n, *mean = buf + 2 * n;
    int32_t *last_gap = ints, *last_status = ints + n, *steps = ints + 2 * n;
    tsf_ar_out est;
    memset(&est, 0, sizeof(est));
    est.phi = phi;
    est.status = est_status;
    tsf_ar_last_out last;
    last.last_resid = last_resid;
    last.last_gap = last_gap;
    last.status = last_status;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    int rc = tsf_residual_autocorr(ctx, N, T, NULL, y, TSF_Y_F64, fitted, NULL, &est);
    if (rc != 0) { fprintf(stderr, "tsf_residual_autocorr: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: an output missing; a bad dtype */
    last.last_gap = NULL;
    if (tsf_residual_last(ctx, N, T, NULL, y, TSF_Y_F64, fitted, &last) >= 0) return 7;
    last.last_gap = last_gap;
    if (tsf_residual_last(ctx, N, T, NULL, y, 7, fitted, &last) >= 0) return 7;
    rc = tsf_residual_last(ctx, N, T, NULL, y, TSF_Y_F64, fitted, &last);
    if (rc != 0) { fprintf(stderr, "tsf_residual_last: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    for (size_t i = 0; i < n; ++i) {
        if (last_status[i] != TSF_AR_OK && last_status[i] != TSF_AR_NO_ROW) return 9;
        steps[i] = last_gap[i] + 1;
    }
    if (tsf_noise_ar_mean(N, phi, last_resid, steps, H, mean) != 0) return 6;

    /* refused: a start without a pending phi; a start for another number of series (and the phi is gone with it: the
     * draw behind it would be the independent one); a step count of 0 */
    if (tsf_set_noise_ar_start(ctx, last_resid, steps, N) >= 0) return 7;
    if (tsf_set_noise_ar(ctx, phi, N) != 0) return 6;
    if (tsf_set_noise_ar_start(ctx, last_resid, steps, N - 1) >= 0) return 7;
    if (tsf_set_noise_ar(ctx, phi, N) != 0) return 6;
    steps[0] = 0;
    if (tsf_set_noise_ar_start(ctx, last_resid, steps, N) >= 0) return 7;
    steps[0] = last_gap[0] + 1;

    tsf_quantile_out out;
    double *at = buf + 2 * n + nh;
    for (int call = 0; call < 2; ++call) {
        /* call 0: both settings; 1: none (the refusals above cleared what was pending) */
        if (call == 0) {
            rc = tsf_set_noise_ar(ctx, phi, N);
            if (rc == 0) rc = tsf_set_noise_ar_start(ctx, last_resid, steps, N);
            if (rc != 0) { fprintf(stderr, "tsf_set_noise_ar_start: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
        }
        out.yhat = at;
        out.q = out.yhat + nh;
        out.cum_q = out.q + nh * NQ;
        out.trend_q = NULL;
        out.samples = out.cum_q + nh * NQ;
        out.trend_samples = NULL;
        rc = tsf_predict_quantiles(ctx, &spec, N, H, theta, ys, (const tsf_grid_info *)grid, (int32_t)N, fut, 1, NULL, NULL,
                                   extra, key, NS, 5, NQ, levels, &out);
        if (rc != 0) { fprintf(stderr, "tsf_predict_quantiles: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
        at += per_call;
    }
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    snprintf(path, sizeof(path), "%s/ints.i32", dir);
    f = fopen(path, "wb");
    if (!f || fwrite(ints, sizeof(int32_t), 3 * n, f) != 3 * n) return 8;
    fclose(f);
    free(buf); free(ints); free(est_status); free(theta); free(ys); free(grid); free(fut); free(extra); free(key); free(y);
    free(fitted);
    return 0;
}
