/* Plain C99 caller of reconciliation through the C-ABI (include/tsf.h): tsf_reconcile_shares, then tsf_rollup_create,
 * tsf_rollup_add twice (series [0, N / 2) and [N / 2, N)), tsf_rollup_set_totals, tsf_rollup_reconcile,
 * tsf_rollup_reconciled_totals, tsf_rollup_free on models read from raw binary files -- no Python in the process.  The
 * tsf_spec itself is read from a file (its size checked against tsf_spec_size), so the caller picks the model.
 * Levels 0.1, 0.5, 0.9; 50 samples, seed 5; every output requested; weights all 1, the totals' weights in v.f64.
 * Usage: abi_reconcile N Gt H G dir   (dir holds spec.bin, fut.i64 and, for the members and with the prefix t_ for the
 * totals, theta.f64 ys.f64 grid.bin floor.f64 cap.f64 key.i64 group.i64; v.f64 [G]; writes dir/out.f64: share [N],
 * share_total [G], the members' yhat [N][H], q, cum_q [N][3][H] each, samples [N][H][50], then the totals' yhat [G][H],
 * q, cum_q [G][3][H] each, samples [G][H][50]) */
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
    int64_t n;
    double *theta, *ys, *floor, *cap;
    tsf_grid_info *grid;
    int64_t *key, *group;
} series;

static series load(const char *dir, const char *prefix, int64_t n, int stride)
{
    series s;
    char name[64];
    s.n = n;
    snprintf(name, sizeof(name), "%stheta.f64", prefix); s.theta = slurp(dir, name, sizeof(double) * (size_t)(n * stride));
    snprintf(name, sizeof(name), "%sys.f64", prefix); s.ys = slurp(dir, name, sizeof(double) * (size_t)n);
    snprintf(name, sizeof(name), "%sfloor.f64", prefix); s.floor = slurp(dir, name, sizeof(double) * (size_t)n);
    snprintf(name, sizeof(name), "%scap.f64", prefix); s.cap = slurp(dir, name, sizeof(double) * (size_t)n);
    snprintf(name, sizeof(name), "%sgrid.bin", prefix); s.grid = slurp(dir, name, sizeof(tsf_grid_info) * (size_t)n);
    snprintf(name, sizeof(name), "%skey.i64", prefix); s.key = slurp(dir, name, sizeof(int64_t) * (size_t)n);
    snprintf(name, sizeof(name), "%sgroup.i64", prefix); s.group = slurp(dir, name, sizeof(int64_t) * (size_t)n);
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const int64_t N = atoll(argv[1]), Gt = atoll(argv[2]);
    const int32_t H = atoi(argv[3]);
    const int64_t G = atoll(argv[4]);
    const char *dir = argv[5];

    if (tsf_spec_size() != (int)sizeof(tsf_spec) || tsf_grid_info_size() != (int)sizeof(tsf_grid_info)) return 3;
    if (tsf_reconcile_out_size() != (int)sizeof(tsf_reconcile_out)) return 3;
    tsf_spec *spec = slurp(dir, "spec.bin", sizeof(tsf_spec));
    const int stride = tsf_theta_stride(spec);
    series m = load(dir, "", N, stride), t = load(dir, "t_", Gt, stride);
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    double *v = slurp(dir, "v.f64", sizeof(double) * (size_t)G);

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t nh = (size_t)(N * H), gh = (size_t)(G * H);
    const size_t total = (size_t)(N + G) + (nh + gh) * (1 + 2 * NQ + NS);
    double *buf = calloc(total, sizeof(double));
    if (!buf) return 4;
    double *share = buf, *share_total = share + N;
    tsf_reconcile_out mo;
    mo.yhat = share_total + G;
    mo.q = mo.yhat + nh;
    mo.cum_q = mo.q + nh * NQ;
    mo.samples = mo.cum_q + nh * NQ;
    tsf_rollup_out to;
    to.yhat = mo.samples + nh * NS;
    to.count = NULL;
    to.q = to.yhat + gh;
    to.cum_q = to.q + gh * NQ;
    to.samples = to.cum_q + gh * NQ;

    /* the shares: host only, before any context exists; refused: a group index of G */
    const int64_t g0 = m.group[0];
    m.group[0] = G;
    if (tsf_reconcile_shares(N, m.group, NULL, G, v, share, share_total) != -1) return 7;
    m.group[0] = g0;
    if (tsf_reconcile_shares(N, m.group, NULL, G, v, share, share_total) != 0) return 6;

    tsf_ctx *ctx = NULL;
    tsf_rollup *r = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    if (tsf_rollup_create(ctx, G, H, fut, NS, 5, &r) != 0) { fprintf(stderr, "create: %s\n", tsf_last_error(ctx)); return 6; }
    const int64_t half = N / 2;
    int rc = tsf_rollup_add(r, spec, half, m.theta, m.ys, m.grid, (int32_t)half, m.floor, m.cap, NULL, 1, m.key, m.group);
    if (rc == 0)
        rc = tsf_rollup_add(r, spec, N - half, m.theta + half * stride, m.ys + half, m.grid + half, (int32_t)(N - half),
                            m.floor + half, m.cap + half, NULL, 1, m.key + half, m.group + half);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_add: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: reconciling before there is any total */
    if (tsf_rollup_reconcile(r, spec, N, m.theta, m.ys, m.grid, (int32_t)N, m.floor, m.cap, NULL, 1, m.key, m.group, share,
                             NQ, levels, &mo) >= 0)
        return 7;
    if (tsf_rollup_reconciled_totals(r, share_total, NQ, levels, &to) >= 0) return 7;
    rc = tsf_rollup_set_totals(r, spec, Gt, t.theta, t.ys, t.grid, (int32_t)Gt, t.floor, t.cap, NULL, 1, t.key, t.group);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_set_totals: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: a second total for a group; no keys; a share above 1; a level outside [0, 1] */
    if (tsf_rollup_set_totals(r, spec, 1, t.theta, t.ys, t.grid, 1, t.floor, t.cap, NULL, 1, t.key, t.group) >= 0) return 7;
    if (tsf_rollup_reconcile(r, spec, N, m.theta, m.ys, m.grid, (int32_t)N, m.floor, m.cap, NULL, 1, NULL, m.group, share,
                             NQ, levels, &mo) >= 0)
        return 7;
    const double s0 = share[0], bad[1] = {1.5};
    share[0] = 1.25;
    if (tsf_rollup_reconcile(r, spec, N, m.theta, m.ys, m.grid, (int32_t)N, m.floor, m.cap, NULL, 1, m.key, m.group, share,
                             NQ, levels, &mo) >= 0)
        return 7;
    share[0] = s0;
    if (tsf_rollup_reconciled_totals(r, share_total, 1, bad, &to) >= 0) return 7;
    rc = tsf_rollup_reconcile(r, spec, N, m.theta, m.ys, m.grid, (int32_t)N, m.floor, m.cap, NULL, 1, m.key, m.group, share,
                              NQ, levels, &mo);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_reconcile: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    rc = tsf_rollup_reconciled_totals(r, share_total, NQ, levels, &to);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_reconciled_totals: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_rollup_free(r);
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    free(buf); free(spec); free(fut); free(v);
    free(m.theta); free(m.ys); free(m.floor); free(m.cap); free(m.grid); free(m.key); free(m.group);
    free(t.theta); free(t.ys); free(t.floor); free(t.cap); free(t.grid); free(t.key); free(t.group);
    return 0;
}
