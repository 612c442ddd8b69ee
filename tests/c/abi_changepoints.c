/* Plain C99 caller of the C-ABI that fits an aligned panel with specified changepoint dates (tsf_spec.changepoints_specified /
 * changepoint_ns, include/tsf.h), set after tsf_spec_default as a C caller would.
 * Usage: abi_changepoints N T n_cp ds.i64 y.f64 cp.i64 out.f64   (linear growth, additive weekly order 3)
 * out: N*stride theta, then N (status, n_iter, n_eval as doubles), then grid S and its n_cp t_change.
 * Then the same dates in descending order: the call must fail before any launch, with an error text. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tsf.h"

static void *slurp(const char *path, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    void *p = malloc(bytes ? bytes : 1);
    if (!f || !p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", path); exit(10); }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 8) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t T = atoi(argv[2]), n_cp = atoi(argv[3]);
    if (n_cp < 0 || n_cp > TSF_MAX_S) return 2;
    int64_t *ds = slurp(argv[4], sizeof(int64_t) * (size_t)T);
    double *y = slurp(argv[5], sizeof(double) * (size_t)(N * T));
    int64_t *cp = slurp(argv[6], sizeof(int64_t) * (size_t)n_cp);

    tsf_spec spec;
    tsf_spec_default(&spec);
    if (spec.changepoints_specified != 0) { fprintf(stderr, "default spec has changepoints_specified set\n"); return 11; }
    spec.growth = TSF_GROWTH_LINEAR;
    spec.n_seas = 1;
    spec.seas_period[0] = 7.0;
    spec.seas_order[0] = 3;
    spec.seas_prior_scale[0] = 10.0;
    spec.seas_mode[0] = TSF_MODE_ADDITIVE;
    spec.changepoints_specified = 1;
    spec.n_changepoints = n_cp;
    for (int j = 0; j < n_cp; ++j) spec.changepoint_ns[j] = cp[j];
    const int stride = tsf_theta_stride(&spec);

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed: no GPU\n"); return 3; }
    tsf_fit_out out;
    tsf_grid_info grid;
    out.theta = calloc((size_t)(N * stride), sizeof(double));
    out.y_scale = calloc((size_t)N, sizeof(double));
    out.fval = calloc((size_t)N, sizeof(double));
    out.status = calloc((size_t)N, sizeof(int32_t));
    out.n_iter = calloc((size_t)N, sizeof(int32_t));
    out.n_eval = calloc((size_t)N, sizeof(int32_t));
    out.grid = &grid;
    int rc = tsf_fit_aligned(ctx, &spec, N, T, ds, y, TSF_Y_F64, NULL, NULL, NULL, &out);
    if (rc != 0) { fprintf(stderr, "fit rc=%d: %s\n", rc, tsf_last_error(ctx)); return 4; }

    FILE *f = fopen(argv[7], "wb");
    if (!f) return 6;
    fwrite(out.theta, sizeof(double), (size_t)(N * stride), f);
    for (int64_t n = 0; n < N; ++n) {
        double t[3];
        t[0] = out.status[n]; t[1] = out.n_iter[n]; t[2] = out.n_eval[n];
        fwrite(t, sizeof(double), 3, f);
    }
    {
        double s = grid.S;
        fwrite(&s, sizeof(double), 1, f);
        fwrite(grid.t_change, sizeof(double), (size_t)n_cp, f);
    }
    fclose(f);

    if (n_cp >= 2) {
        tsf_spec bad = spec;
        for (int j = 0; j < n_cp; ++j) bad.changepoint_ns[j] = cp[n_cp - 1 - j];
        rc = tsf_fit_aligned(ctx, &bad, N, T, ds, y, TSF_Y_F64, NULL, NULL, NULL, &out);
        if (rc >= 0 || strlen(tsf_last_error(ctx)) == 0) { fprintf(stderr, "descending dates accepted (rc=%d)\n", rc); return 12; }
        printf("unsorted: rc=%d %s\n", rc, tsf_last_error(ctx));
    }
    tsf_destroy(ctx);
    printf("stride=%d S=%d T=%d\n", stride, grid.S, grid.T);
    return 0;
}
