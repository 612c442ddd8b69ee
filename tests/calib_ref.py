"""The contracts of tsf_calibrate_rows and tsf_apply_calibration (include/tsf.h, "conformal interval calibration")
restated in numpy, operation for operation.  Not a test file: shared by tests/test_calib_ref.py (CPU: the restatement on
hand-worked cases) and tests/test_gpu_calibrate.py (the kernels against the restatement, bit for bit).

Every numpy operation on doubles below is one IEEE double operation per element (subtract, add, multiply, abs, fmax,
fmin, ceil), in the order the header writes them; every integer operation is int64; sorting moves values and rounds
nothing."""
import numpy as np

OK, NO_SCORES, TOO_LONG = 0, -40, -41      # TSF_CALIB_* (include/tsf.h)
ABS, CQR = 0, 1                             # TSF_CALIB_ABS, TSF_CALIB_CQR
MAX_ROWS = 16384                            # TSF_CALIB_MAX_ROWS


def bucket_width(horizon, n_buckets):
    return (int(horizon) + int(n_buckets) - 1) // int(n_buckets)


def calibrate_series(h, y, yhat, levels, lower=None, upper=None, mode=ABS, horizon=1, n_buckets=1, min_scores=1):
    """One series: h [m0] int64, y / yhat [m0], lower / upper [L][m0] (CQR) -> (q [B+1][L], n [B+1][L] int32, status)."""
    h = np.asarray(h, dtype=np.int64)
    y = np.asarray(y, dtype=np.float64)
    yhat = np.asarray(yhat, dtype=np.float64)
    levels = np.asarray(levels, dtype=np.float64)
    L, B, H = len(levels), int(n_buckets), int(horizon)
    q = np.full((B + 1, L), np.nan)
    cnt = np.zeros((B + 1, L), np.int32)
    if len(h) > MAX_ROWS:
        return q, cnt, TOO_LONG
    w = bucket_width(H, B)
    eligible = (h > 0) & (h <= H)
    bucket = np.minimum(np.int64(B - 1), (h - 1) // np.int64(w))       # (only read where eligible: h >= 1)
    any_pool = False
    for l in range(L):
        with np.errstate(invalid='ignore', over='ignore'):
            if mode == ABS:
                s = np.abs(y - yhat)
                live = eligible & np.isfinite(s)
            else:
                lo, hi = np.asarray(lower[l], dtype=np.float64), np.asarray(upper[l], dtype=np.float64)
                s = np.fmax(lo - y, y - hi)
                live = eligible & np.isfinite(y) & np.isfinite(lo) & np.isfinite(hi)
        for b in range(B + 1):
            a = np.sort(s[live & (bucket == b)] if b < B else s[live])
            m = len(a)
            cnt[b, l] = m
            if m < min_scores:
                continue
            k = int(np.ceil(np.float64(m + 1) * levels[l]))
            q[b, l] = a[min(k, m) - 1] + np.float64(0.0)          # (a zero comes out as +0.0)
            if b == B:
                any_pool = True
    return q, cnt, OK if any_pool else NO_SCORES


def calibrate_rows(row_off, h, y, yhat, levels, lower=None, upper=None, **kw):
    """A ragged set of rows: series n owns rows [row_off[n], row_off[n + 1]); lower / upper [L][R] ->
    dict q [N][B+1][L], n [N][B+1][L] int32, status [N] int32."""
    row_off = np.asarray(row_off, dtype=np.int64)
    N, L, B = len(row_off) - 1, len(levels), int(kw.get('n_buckets', 1))
    q, cnt, st = np.full((N, B + 1, L), np.nan), np.zeros((N, B + 1, L), np.int32), np.zeros(N, np.int32)
    for n in range(N):
        s = slice(int(row_off[n]), int(row_off[n + 1]))
        q[n], cnt[n], st[n] = calibrate_series(np.asarray(h)[s], np.asarray(y)[s], np.asarray(yhat)[s], levels,
                                               None if lower is None else np.asarray(lower)[:, s],
                                               None if upper is None else np.asarray(upper)[:, s], **kw)
    return {'q': q, 'n': cnt, 'status': st}


def mask_series(table, bad):
    """tsf_calibrate's rule for a series whose cross-validation status is not TSF_CV_OK: no table (q NaN, n 0),
    TSF_CALIB_NO_SCORES."""
    bad = np.asarray(bad, dtype=bool)
    q, cnt, st = table['q'].copy(), table['n'].copy(), table['status'].copy()
    q[bad], cnt[bad], st[bad] = np.nan, 0, NO_SCORES
    return {'q': q, 'n': cnt, 'status': st}


def apply(yhat, ds_future, origin_ns, q, n, levels, lower=None, upper=None, mode=ABS, horizon=1, n_buckets=1,
          min_scores=1):
    """yhat [N][H], ds_future [H] or [N][H], origin_ns [N], q / n [N][B+1][L], lower / upper [N][L][H] ->
    (lo, hi [N][L][H], cell [N][L][H] int8: the bucket used, B for the pooled cell, -1 for none)."""
    yhat = np.asarray(yhat, dtype=np.float64)
    N, H = yhat.shape
    L, B = len(levels), int(n_buckets)
    ds = np.broadcast_to(np.asarray(ds_future, dtype=np.int64), (N, H))
    w = bucket_width(horizon, B)
    h = ds - np.asarray(origin_ns, dtype=np.int64)[:, None]
    b = np.where(h <= 0, 0, np.minimum(np.int64(B - 1), (h - 1) // np.int64(w)))
    lo, hi = np.full((N, L, H), np.nan), np.full((N, L, H), np.nan)
    cell = np.full((N, L, H), -1, np.int8)
    rows = np.arange(N)[:, None]
    for l in range(L):
        own = n[rows, b, l] >= min_scores
        pool = (n[:, B, l] >= min_scores)[:, None] & ~own
        c = np.where(own, b, np.where(pool, B, -1))
        qq = np.where(c >= 0, q[rows, np.maximum(c, 0), l], np.nan)
        with np.errstate(invalid='ignore', over='ignore'):
            if mode == ABS:
                lo_l, hi_l = yhat - qq, yhat + qq
            else:
                lo_l = np.fmin(np.asarray(lower, dtype=np.float64)[:, l, :] - qq, yhat)
                hi_l = np.fmax(np.asarray(upper, dtype=np.float64)[:, l, :] + qq, yhat)
        none = (c < 0) | ~np.isfinite(yhat)
        lo[:, l, :], hi[:, l, :] = np.where(none, np.nan, lo_l), np.where(none, np.nan, hi_l)
        cell[:, l, :] = c
    return lo, hi, cell


def same(a, b):
    """bit for bit, NaN where and only where the other has one (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
