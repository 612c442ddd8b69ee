/* Plain C99 caller of temporal reconciliation through the C-ABI (include/tsf.h): tsf_temporal_shares, then
 * tsf_predict_temporal on two models read from raw binary files -- no Python in the process.  Both tsf_specs are read
 * from files (their size checked against tsf_spec_size), so the caller picks the models.  Per-series calendars, no extra
 * columns, noise_ar on the daily side.  Levels 0.1, 0.5, 0.9; 50 samples, seed 5; every output requested; row weights
 * all 1, the period forecasts' weights in v.f64.
 * Usage: abi_temporal N H K dir   (dir holds spec.bin, p_spec.bin, w0.i32, w1.i32 [K], v.f64 [N][K], phi.f64 [N] and, for
 * the daily model and with the prefix p_ for the period model, theta.f64 ys.f64 grid.bin floor.f64 cap.f64 key.i64 and
 * ds.i64 [N][H] / [N][K]; writes dir/out.f64: share [N][H], share_total [N][K], yhat [N][H], q, cum_q [N][3][H] each,
 * total [N][K], win_q [N][3][K], samples [N][H][50], win_samples [N][K][50]) */
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

typedef struct {
    tsf_spec *spec;
    double *theta, *ys, *floor, *cap;
    tsf_grid_info *grid;
    int64_t *key, *ds;
} model;

static model load(const char *dir, const char *prefix, int64_t n, int32_t rows)
{
    model m;
    char name[64];
    snprintf(name, sizeof(name), "%sspec.bin", prefix); m.spec = slurp(dir, name, sizeof(tsf_spec));
    const size_t stride = (size_t)tsf_theta_stride(m.spec);
    snprintf(name, sizeof(name), "%stheta.f64", prefix); m.theta = slurp(dir, name, sizeof(double) * (size_t)n * stride);
    snprintf(name, sizeof(name), "%sys.f64", prefix); m.ys = slurp(dir, name, sizeof(double) * (size_t)n);
    snprintf(name, sizeof(name), "%sfloor.f64", prefix); m.floor = slurp(dir, name, sizeof(double) * (size_t)n);
    snprintf(name, sizeof(name), "%scap.f64", prefix); m.cap = slurp(dir, name, sizeof(double) * (size_t)n);
    snprintf(name, sizeof(name), "%sgrid.bin", prefix); m.grid = slurp(dir, name, sizeof(tsf_grid_info) * (size_t)n);
    snprintf(name, sizeof(name), "%skey.i64", prefix); m.key = slurp(dir, name, sizeof(int64_t) * (size_t)n);
    snprintf(name, sizeof(name), "%sds.i64", prefix); m.ds = slurp(dir, name, sizeof(int64_t) * (size_t)n * (size_t)rows);
    return m;
}

static void unload(model *m)
{
    free(m->spec); free(m->theta); free(m->ys); free(m->floor); free(m->cap); free(m->grid); free(m->key); free(m->ds);
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t H = atoi(argv[2]), K = atoi(argv[3]);
    const char *dir = argv[4];

    if (tsf_spec_size() != (int)sizeof(tsf_spec) || tsf_grid_info_size() != (int)sizeof(tsf_grid_info)) return 3;
    if (tsf_temporal_out_size() != (int)sizeof(tsf_temporal_out)) return 3;
    model d = load(dir, "", N, H), p = load(dir, "p_", N, K);
    int32_t *w0 = slurp(dir, "w0.i32", sizeof(int32_t) * (size_t)K), *w1 = slurp(dir, "w1.i32", sizeof(int32_t) * (size_t)K);
    double *v = slurp(dir, "v.f64", sizeof(double) * (size_t)(N * K));
    double *phi = slurp(dir, "phi.f64", sizeof(double) * (size_t)N);

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t nh = (size_t)(N * H), nk = (size_t)(N * K);
    const size_t total = (nh + nk) * (2 + NQ + NS) + nh * NQ;
    double *buf = calloc(total, sizeof(double));
    if (!buf) return 4;
    double *share = buf, *share_total = share + nh;
    tsf_temporal_out o;
    o.yhat = share_total + nk;
    o.q = o.yhat + nh;
    o.cum_q = o.q + nh * NQ;
    o.total = o.cum_q + nh * NQ;
    o.win_q = o.total + nk;
    o.samples = o.win_q + nk * NQ;
    o.win_samples = o.samples + nh * NS;

    /* the shares: host only, before any context exists; refused: a window that ends behind row H */
    const int32_t e0 = w1[0];
    w1[0] = H + 1;
    if (tsf_temporal_shares(N, H, K, w0, w1, NULL, v, share, share_total) != -1) return 7;
    w1[0] = e0;
    if (tsf_temporal_shares(N, H, K, w0, w1, NULL, v, share, share_total) != 0) return 6;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
#define CALL(KEY, PKEY, SHARE, NLEV, LEVELS, OUT)                                                                          \
    tsf_predict_temporal(ctx, d.spec, N, H, d.theta, d.ys, d.grid, (int32_t)N, d.ds, 0, d.floor, d.cap, NULL, KEY, phi,  \
                         p.spec, K, p.theta, p.ys, p.grid, (int32_t)N, p.ds, 0, p.floor, p.cap, NULL, PKEY, NULL, NS, 5, \
                         w0, w1, SHARE, share_total, NLEV, LEVELS, OUT)
    /* refused: no keys for the period model; a share above 1; a level outside [0, 1]; nothing wanted but yhat and total */
    if (CALL(d.key, NULL, share, NQ, levels, &o) >= 0) return 7;
    const double s0 = share[w0[0]], bad[1] = {1.5};
    share[w0[0]] = 1.25;
    if (CALL(d.key, p.key, share, NQ, levels, &o) >= 0) return 7;
    share[w0[0]] = s0;
    if (CALL(d.key, p.key, share, 1, bad, &o) >= 0) return 7;
    tsf_temporal_out none;
    memset(&none, 0, sizeof(none));
    none.yhat = o.yhat;
    none.total = o.total;
    if (CALL(d.key, p.key, share, NQ, levels, &none) >= 0) return 7;
    const int rc = CALL(d.key, p.key, share, NQ, levels, &o);
    if (rc != 0) { fprintf(stderr, "tsf_predict_temporal: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    free(buf); free(w0); free(w1); free(v); free(phi);
    unload(&d); unload(&p);
    return 0;
}
