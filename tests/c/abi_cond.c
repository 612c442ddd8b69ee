/* Plain C99 caller of the conditional-seasonality entry through the C-ABI (include/tsf.h, "conditional
 * seasonalities"): tsf_cond_columns for two conditional seasonalities (period 7 order 3 on condition row 0, period 1
 * order 4 on condition row 1: 14 columns) on timestamps and condition rows read from raw binary files -- no Python in
 * the process.  The columns are written INTO a larger block, as a caller's `extra` array would hold them: 2 leading
 * columns of the caller's own, a row length of rows + 5; the block is pre-filled with a marker, so the test sees that
 * nothing but the 14 x rows values was written.  Then the refused calls (each must return < 0 with a text and leave the
 * context usable), and rows = 0.
 * Usage: abi_cond rows dir   (dir holds ds.i64 [rows], cond.u8 [2][rows]; writes dir/out.f64: the block [16][rows + 5]) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tsf.h"

#define LEAD 2
#define PAD 5
#define MARK -12345.0

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

static int refused(tsf_ctx *ctx, const char *what, int rc)
{
    const char *msg = tsf_last_error(ctx);
    if (rc >= 0 || !msg || !msg[0]) { fprintf(stderr, "%s: not refused (rc=%d)\n", what, rc); return 0; }
    printf("%s: rc=%d %s\n", what, rc, msg);
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int64_t rows = atoll(argv[1]);
    const char *dir = argv[2];
    if (rows < 1) return 2;

    tsf_cond_seas cs;
    memset(&cs, 0, sizeof(cs));
    cs.n = 2;
    cs.period[0] = 7.0; cs.order[0] = 3; cs.cond[0] = 0;
    cs.period[1] = 1.0; cs.order[1] = 4; cs.cond[1] = 1;
    const int64_t C = 14, stride = rows + PAD;

    int64_t *ds = slurp(dir, "ds.i64", sizeof(int64_t) * (size_t)rows);
    uint8_t *cond = slurp(dir, "cond.u8", 2 * (size_t)rows);
    const size_t total = (size_t)((LEAD + C) * stride);
    double *block = malloc(sizeof(double) * total);
    if (!block) return 4;
    for (size_t i = 0; i < total; ++i) block[i] = MARK;
    double *cols = block + LEAD * stride;

    tsf_ctx *ctx = NULL;
    if (tsf_create(0, &ctx) != 0) { fprintf(stderr, "tsf_create failed\n"); return 5; }

    /* refused before any launch: a stride below the rows, a bad count, a bad period, a bad order, too many columns, a
     * bad condition index */
    tsf_cond_seas bad;
    if (!refused(ctx, "stride", tsf_cond_columns(ctx, &cs, rows, ds, 2, cond, cols, rows - 1))) return 7;
    bad = cs; bad.n = 0;
    if (!refused(ctx, "count0", tsf_cond_columns(ctx, &bad, rows, ds, 2, cond, cols, stride))) return 7;
    bad = cs; bad.n = TSF_MAX_SEAS + 1;
    if (!refused(ctx, "count9", tsf_cond_columns(ctx, &bad, rows, ds, 2, cond, cols, stride))) return 7;
    bad = cs; bad.period[1] = 0.0;
    if (!refused(ctx, "period", tsf_cond_columns(ctx, &bad, rows, ds, 2, cond, cols, stride))) return 7;
    bad = cs; bad.order[0] = 0;
    if (!refused(ctx, "order", tsf_cond_columns(ctx, &bad, rows, ds, 2, cond, cols, stride))) return 7;
    bad = cs; bad.order[0] = 20; bad.order[1] = 13;
    if (!refused(ctx, "columns", tsf_cond_columns(ctx, &bad, rows, ds, 2, cond, cols, stride))) return 7;
    bad = cs; bad.cond[1] = 2;
    if (!refused(ctx, "index", tsf_cond_columns(ctx, &bad, rows, ds, 2, cond, cols, stride))) return 7;
    for (size_t i = 0; i < total; ++i)
        if (block[i] != MARK) { fprintf(stderr, "a refused call wrote\n"); return 8; }

    /* rows = 0: a legal no-op (no pointer is read) */
    int rc = tsf_cond_columns(ctx, &cs, 0, NULL, 2, NULL, NULL, 0);
    if (rc != 0) { fprintf(stderr, "rows = 0: %d %s\n", rc, tsf_last_error(ctx)); return 6; }

    rc = tsf_cond_columns(ctx, &cs, rows, ds, 2, cond, cols, stride);
    if (rc != 0) { fprintf(stderr, "tsf_cond_columns: %d %s\n", rc, tsf_last_error(ctx)); return 6; }
    tsf_destroy(ctx);

    char path[4096];
    snprintf(path, sizeof(path), "%s/out.f64", dir);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(block, sizeof(double), total, f) != total) return 8;
    fclose(f);
    free(block); free(ds); free(cond);
    return 0;
}
