"""The contract of tsf_predict_windows / tsf_rollup_windows (include/tsf.h, "totals over row windows") restated in
numpy: the sequential window sum of every draw, then the quantile expression and the row functions of
tests/score_ref.py with a window in the place of a row.  Not a test file: shared by tests/test_window_ref.py (CPU: the
restatement against itself and the Python helpers against pandas) and tests/test_gpu_windows.py (the kernels against
the restatement, bit for bit).

Every numpy operation below is one IEEE double add per element, in the order the header writes them."""
import numpy as np

from tests import score_ref as sr


def window_sums(x, start, end):
    """x [..., H, S] -> [..., K, S]: c = x[a]; c = c + x[h] for h = a + 1 .. b - 1, per window [a, b)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape[:-2] + (len(start), x.shape[-1]))
    for k, (a, b) in enumerate(zip(start, end)):
        c = x[..., int(a), :].copy()
        for h in range(int(a) + 1, int(b)):
            c = c + x[..., h, :]
        out[..., k, :] = c
    return out


def totals(yhat, start, end):
    """yhat [N][H] -> [N][K]: the same sum of the point forecasts"""
    return window_sums(np.asarray(yhat, dtype=np.float64)[..., None], start, end)[..., 0]


def score(draws, y_win, levels, start, end):
    """draws [N][H][S], y_win [N][K] or None (NaN = not observed), levels [Q] -> dict: q [N][Q][K] and, with y_win,
    every other field of tsf_window_out but yhat and total (score_ref.score over the window sums)."""
    sums = window_sums(draws, start, end)
    if y_win is None:
        v = np.sort(sums, axis=-1)
        return {'q': np.stack([sr.quantile(v, p) for p in levels], axis=1)}
    return sr.score(sums, y_win, levels)
