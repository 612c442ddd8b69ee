/* Plain C99 caller of tree reconciliation through the C-ABI (include/tsf.h): tsf_reconcile_tree_shares, then
 * tsf_rollup_create, tsf_rollup_add twice (series [0, N / 2) and [N / 2, N)), tsf_rollup_set_totals, tsf_rollup_set_tree,
 * tsf_rollup_set_node_totals per upper level, tsf_rollup_solve_tree, tsf_rollup_reconcile_tree, tsf_rollup_tree_totals per
 * level, tsf_rollup_free on models read from raw binary files -- no Python in the process.  The tsf_spec itself is read
 * from a file (its size checked against tsf_spec_size).  Levels 0.1, 0.5, 0.9; 50 samples, seed 5; every output
 * requested; no floor, no cap (a linear model).
 * Usage: abi_tree N H dir L n_1 .. n_L t_1 .. t_L   (n_k nodes and t_k fitted totals at level k; n_1 = G; dir holds
 * spec.bin, fut.i64, w.f64 [N], parent.i64 (flat), v.f64 [M] and, for the members and with the prefix t<k>_ for the totals
 * of level k, theta.f64 ys.f64 grid.bin key.i64 group.i64; writes dir/out.f64: share [N], mu [M], kappa [M], the members'
 * yhat [N][H], q, cum_q [N][3][H] each, samples [N][H][50], then per level yhat [n][H], q, cum_q [n][3][H] each,
 * samples [n][H][50]) */
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
    double *theta, *ys;
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
    snprintf(name, sizeof(name), "%sgrid.bin", prefix); s.grid = slurp(dir, name, sizeof(tsf_grid_info) * (size_t)n);
    snprintf(name, sizeof(name), "%skey.i64", prefix); s.key = slurp(dir, name, sizeof(int64_t) * (size_t)n);
    snprintf(name, sizeof(name), "%sgroup.i64", prefix); s.group = slurp(dir, name, sizeof(int64_t) * (size_t)n);
    return s;
}

static void drop(series *s) { free(s->theta); free(s->ys); free(s->grid); free(s->key); free(s->group); }

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int64_t N = atoll(argv[1]);
    const int32_t H = atoi(argv[2]);
    const char *dir = argv[3];
    const int32_t L = atoi(argv[4]);
    if (L < 2 || L > 1 + TSF_TREE_MAX_LEVELS || argc != 5 + 2 * L) return 2;
    int64_t n_nodes[1 + TSF_TREE_MAX_LEVELS], n_tot[1 + TSF_TREE_MAX_LEVELS], M = 0;
    for (int32_t k = 0; k < L; ++k) {
        n_nodes[k] = atoll(argv[5 + k]);
        n_tot[k] = atoll(argv[5 + L + k]);
        M += n_nodes[k];
    }
    const int64_t G = n_nodes[0];

    if (tsf_spec_size() != (int)sizeof(tsf_spec) || tsf_grid_info_size() != (int)sizeof(tsf_grid_info)) return 3;
    if (tsf_reconcile_out_size() != (int)sizeof(tsf_reconcile_out)) return 3;
    tsf_spec *spec = slurp(dir, "spec.bin", sizeof(tsf_spec));
    const int stride = tsf_theta_stride(spec);
    series m = load(dir, "", N, stride), t[1 + TSF_TREE_MAX_LEVELS];
    for (int32_t k = 0; k < L; ++k) {
        char prefix[16];
        snprintf(prefix, sizeof(prefix), "t%d_", k + 1);
        t[k] = load(dir, prefix, n_tot[k], stride);
    }
    int64_t *fut = slurp(dir, "fut.i64", sizeof(int64_t) * (size_t)H);
    int64_t *parent = slurp(dir, "parent.i64", sizeof(int64_t) * (size_t)(M - n_nodes[L - 1]));
    double *w = slurp(dir, "w.f64", sizeof(double) * (size_t)N);
    double *v = slurp(dir, "v.f64", sizeof(double) * (size_t)M);

    const double levels[NQ] = {0.1, 0.5, 0.9};
    const size_t per_cell = 1 + 2 * NQ + NS;
    const size_t total = (size_t)(N + 2 * M) + (size_t)((N + M) * H) * per_cell;
    double *buf = calloc(total, sizeof(double)), *e = calloc((size_t)M, sizeof(double));
    if (!buf || !e) return 4;
    double *share = buf, *mu = share + N, *kappa = mu + M, *at = kappa + M;
    tsf_reconcile_out mo;
    const size_t nh = (size_t)(N * H);
    mo.yhat = at; mo.q = mo.yhat + nh; mo.cum_q = mo.q + nh * NQ; mo.samples = mo.cum_q + nh * NQ;
    at = mo.samples + nh * NS;

    /* the shares: host only, before any context exists; refused: a parent out of range, one level too many */
    const int64_t p0 = parent[0];
    parent[0] = n_nodes[1];
    if (tsf_reconcile_tree_shares(N, m.group, w, G, L - 1, n_nodes + 1, parent, v, share, mu, e, kappa) != -1) return 7;
    parent[0] = p0;
    if (tsf_reconcile_tree_shares(N, m.group, w, G, TSF_TREE_MAX_LEVELS + 1, n_nodes + 1, parent, v, share, mu, e, kappa) != -1)
        return 7;
    if (tsf_reconcile_tree_shares(N, m.group, w, G, L - 1, n_nodes + 1, parent, v, share, mu, e, kappa) != 0) return 6;

    tsf_ctx *ctx = NULL;
    tsf_rollup *r = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }
    if (tsf_rollup_create(ctx, G, H, fut, NS, 5, &r) != 0) { fprintf(stderr, "create: %s\n", tsf_last_error(ctx)); return 6; }
    const int64_t half = N / 2;
    int rc = tsf_rollup_add(r, spec, half, m.theta, m.ys, m.grid, (int32_t)half, NULL, NULL, NULL, 1, m.key, m.group);
    if (rc == 0)
        rc = tsf_rollup_add(r, spec, N - half, m.theta + half * stride, m.ys + half, m.grid + half, (int32_t)(N - half),
                            NULL, NULL, NULL, 1, m.key + half, m.group + half);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_add: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    /* refused: everything of the tree before set_tree */
    if (tsf_rollup_solve_tree(r, mu, kappa) >= 0) return 7;
    if (tsf_rollup_set_node_totals(r, 2, spec, t[1].n, t[1].theta, t[1].ys, t[1].grid, (int32_t)t[1].n, NULL, NULL, NULL, 1,
                                   t[1].key, t[1].group) >= 0)
        return 7;
    rc = tsf_rollup_set_totals(r, spec, t[0].n, t[0].theta, t[0].ys, t[0].grid, (int32_t)t[0].n, NULL, NULL, NULL, 1, t[0].key,
                               t[0].group);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_set_totals: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    rc = tsf_rollup_set_tree(r, L - 1, n_nodes + 1, parent);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_set_tree: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    if (tsf_rollup_set_tree(r, L - 1, n_nodes + 1, parent) >= 0) return 7;        /* refused: a second tree */
    for (int32_t k = 1; k < L; ++k) {
        /* refused: level 1 (set_totals is its entry) and a level above the top */
        if (tsf_rollup_set_node_totals(r, k == 1 ? 1 : L + 1, spec, t[k].n, t[k].theta, t[k].ys, t[k].grid, (int32_t)t[k].n, NULL,
                                       NULL, NULL, 1, t[k].key, t[k].group) >= 0)
            return 7;
        rc = tsf_rollup_set_node_totals(r, k + 1, spec, t[k].n, t[k].theta, t[k].ys, t[k].grid, (int32_t)t[k].n, NULL, NULL,
                                        NULL, 1, t[k].key, t[k].group);
        if (rc != 0) { fprintf(stderr, "tsf_rollup_set_node_totals: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    }
    /* refused: a node total given twice; the reads before the solve; a kappa above 1 */
    if (tsf_rollup_set_node_totals(r, L, spec, 1, t[L - 1].theta, t[L - 1].ys, t[L - 1].grid, 1, NULL, NULL, NULL, 1,
                                   t[L - 1].key, t[L - 1].group) >= 0)
        return 7;
    tsf_rollup_out to;
    to.yhat = at; to.count = NULL; to.q = at; to.cum_q = at; to.samples = at;
    if (tsf_rollup_reconcile_tree(r, spec, N, m.theta, m.ys, m.grid, (int32_t)N, NULL, NULL, NULL, 1, m.key, m.group, share, NQ,
                                  levels, &mo) >= 0)
        return 7;
    if (tsf_rollup_tree_totals(r, 1, 0, G, NQ, levels, &to) >= 0) return 7;
    const double k0 = kappa[0];
    kappa[0] = 1.5;
    if (tsf_rollup_solve_tree(r, mu, kappa) >= 0) return 7;
    kappa[0] = k0;
    rc = tsf_rollup_solve_tree(r, mu, kappa);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_solve_tree: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    rc = tsf_rollup_reconcile_tree(r, spec, N, m.theta, m.ys, m.grid, (int32_t)N, NULL, NULL, NULL, 1, m.key, m.group, share, NQ,
                                   levels, &mo);
    if (rc != 0) { fprintf(stderr, "tsf_rollup_reconcile_tree: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    if (tsf_rollup_tree_totals(r, L + 1, 0, 1, NQ, levels, &to) >= 0) return 7;   /* refused: a level out of range */
    if (tsf_rollup_tree_totals(r, 1, 1, G, NQ, levels, &to) >= 0) return 7;       /* refused: nodes out of range */
    for (int32_t k = 0; k < L; ++k) {
        const size_t gh = (size_t)(n_nodes[k] * H);
        to.yhat = at; to.q = to.yhat + gh; to.cum_q = to.q + gh * NQ; to.samples = to.cum_q + gh * NQ;
        at = to.samples + gh * NS;
        rc = tsf_rollup_tree_totals(r, k + 1, 0, n_nodes[k], NQ, levels, &to);
        if (rc != 0) { fprintf(stderr, "tsf_rollup_tree_totals: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    }
    if (at != buf + total) return 9;
    tsf_rollup_free(r);
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(buf, sizeof(double), total, f) != total) return 8;
    fclose(f);
    free(buf); free(e); free(spec); free(fut); free(parent); free(w); free(v);
    drop(&m);
    for (int32_t k = 0; k < L; ++k) drop(&t[k]);
    return 0;
}
