"""The contract of tsf_screen_rows (include/tsf.h, "outlier screening") restated in numpy, operation for operation.
Not a test file: shared by tests/test_screen_ref.py (CPU: the restatement on hand-worked cases) and
tests/test_gpu_screen.py (the kernels against the restatement, bit for bit).

Every numpy operation below is one IEEE double operation per element (subtract, add, multiply, abs, max), in the order
the header writes them; sorting moves values and rounds nothing."""
import numpy as np

OK, TOO_FEW, TOO_LONG, NONFINITE = 0, -30, -31, -32      # TSF_SCREEN_* (include/tsf.h)
MAX_ROWS = 16384                                           # TSF_SCREEN_MAX_ROWS


def screen_series(y, fitted, excluded=None, min_scale=0.0, threshold=5.0, max_share=0.05, min_rows=10):
    """One series: y [m0] (float64 / float32 / int32), fitted [m0], excluded [m0] (non-zero = removed earlier) or None ->
    dict flag [m0] uint8, resid [m0], center, scale, n_new, n_flagged, status."""
    y = np.asarray(y)
    fitted = np.asarray(fitted, dtype=np.float64)
    m0 = len(y)
    ex = np.zeros(m0, bool) if excluded is None else (np.asarray(excluded) != 0)
    with np.errstate(invalid='ignore', over='ignore'):
        r = y.astype(np.float64) - fitted
    live = ~ex
    m = int(live.sum())
    x = m0 - m
    out = {'flag': ex.astype(np.uint8), 'resid': r, 'center': np.float64(np.nan), 'scale': np.float64(np.nan),
           'n_new': 0, 'n_flagged': x, 'status': OK}
    if m0 > MAX_ROWS:
        out['status'] = TOO_LONG
    elif m < min_rows:
        out['status'] = TOO_FEW
    elif not np.all(np.isfinite(r[live])):
        out['status'] = NONFINITE
    if out['status'] != OK:
        return out
    a = np.sort(r[live])
    center = np.float64(0.5) * (a[(m - 1) // 2] + a[m // 2])
    d = np.abs(r - center)
    b = np.sort(d[live])
    mad = np.float64(0.5) * (b[(m - 1) // 2] + b[m // 2])
    scale = np.fmax(np.float64(1.4826) * mad, np.float64(min_scale))
    B = int(np.floor(np.float64(max_share) * np.float64(m0))) - x
    new = np.zeros(m0, bool)
    if B > 0:
        cut = np.fmax(np.float64(threshold) * scale, b[m - 1 - B])
        new = live & (d > cut)
    out.update(flag=(ex | new).astype(np.uint8), center=center, scale=scale, n_new=int(new.sum()),
               n_flagged=x + int(new.sum()))
    return out


def screen(y, fitted, offsets=None, excluded=None, min_scale=None, **kw):
    """A panel: y [N][T], or 1-D with offsets [N+1]; fitted / excluded in y's shape; min_scale [N] or None -> dict of
    arrays as fc.screen_rows returns them (flag, resid in y's shape; center, scale, n_new, n_flagged, status [N])."""
    y = np.asarray(y)
    fitted = np.asarray(fitted, dtype=np.float64)
    if offsets is None:
        N, T = y.shape
        offsets = np.arange(N + 1, dtype=np.int64) * T
    N = len(offsets) - 1
    yf, ff = y.reshape(-1), fitted.reshape(-1)
    ef = None if excluded is None else np.asarray(excluded).reshape(-1)
    flag, resid = np.zeros(len(yf), np.uint8), np.zeros(len(yf))
    center, scale = np.zeros(N), np.zeros(N)
    n_new, n_flagged, status = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    for n in range(N):
        s = slice(int(offsets[n]), int(offsets[n + 1]))
        o = screen_series(yf[s], ff[s], None if ef is None else ef[s], 0.0 if min_scale is None else min_scale[n], **kw)
        flag[s], resid[s] = o['flag'], o['resid']
        center[n], scale[n], n_new[n], n_flagged[n], status[n] = o['center'], o['scale'], o['n_new'], o['n_flagged'], o['status']
    return {'flag': flag.reshape(y.shape), 'resid': resid.reshape(y.shape), 'center': center, 'scale': scale,
            'n_new': n_new, 'n_flagged': n_flagged, 'status': status}


def same(a, b):
    """bit for bit, NaN where and only where the other has one (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


def cut_panel(ds, y, flag, offsets=None, extra=None):
    """The rows without a flag as a ragged panel: (offsets [N+1], ds, y, extra or None).  ds [T] with y [N][T], or ds / y
    1-D with offsets."""
    y = np.asarray(y)
    if offsets is None:
        N, T = y.shape
        ds = np.tile(np.asarray(ds), N)
        extra = None if extra is None else np.tile(np.asarray(extra), (1, N))
        offsets = np.arange(N + 1, dtype=np.int64) * T
    keep = np.asarray(flag).reshape(-1) == 0
    kept = np.add.reduceat(keep.astype(np.int64), offsets[:-1]) if len(keep) else np.zeros(len(offsets) - 1, np.int64)
    kept = np.where(np.diff(offsets) > 0, kept, 0)
    off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    return off, np.asarray(ds)[keep], y.reshape(-1)[keep], None if extra is None else np.asarray(extra)[:, keep]
