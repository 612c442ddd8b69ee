"""Exact cross-validation metrics reference -- TEST INFRASTRUCTURE ONLY.

Prophet's rolling_mean_by_h as include/tsf.h states it (performance_metrics of tsf_cross_validate), in exact rational
arithmetic.  The inputs are the float64 values a call returns -- y as the kernel converts it, yhat, yhat_lower,
yhat_upper, the horizons -- and the window w = clamp(int(rolling_window * n), 1, n) rows:

  * every term is exact: (y - yhat)^2, |y - yhat|, |(y - yhat) / y| and the 0/1 coverage indicator;
  * rows are grouped by distinct horizon; every horizon whose cumulative count (ascending) reaches w gets one row: the
    whole groups of the window plus its leftmost group [gb, ge) weighted by its included share (ge - E + w) / (ge - gb),
    divided by w (E = the rows up to and including the horizon's group);
  * mape is NaN for the whole series when min |y| < 1e-8.

Besides each exact value it returns an error scale per metric row, M_win = (sum of every row of every group the window
touches, [gb, E)) / w.  Every term is >= 0, so a float64 evaluation that only adds rows the window touches -- in any
order -- is within about u (E - gb) M_win of the exact value, plus a few roundings per term and for the weight and the
division.  ``tolerance`` is TOL_C u (E - gb + 2) M_win, u = 2^-53; TOL_C is calibrated in
tests/test_cv_metrics_ref.py.  A window formed as a difference of sums over rows OUTSIDE it has no such bound.

Implementation: per series and quantity the terms are integers over one common denominator D (the lcm of the terms'
denominators), so window sums are plain integer sums and no rational is ever reduced -- the mape terms of a few
thousand rows would otherwise carry denominators of 10^5 bits through every gcd.
"""
import math

import numpy as np

U = 2.0 ** -53          # unit roundoff of float64
TOL_C = 4.0             # calibrated constant, see tests/test_cv_metrics_ref.py::test_tolerance_calibrated
MAPE_MIN_ABS_Y = 1e-8   # mape is NaN for a series with min |y| below this
METRICS = ('mse', 'mae', 'mape', 'coverage')


def window_rows(rolling_window, n):
    return min(max(int(rolling_window * n), 1), n)


def _ratio(x):
    """A finite float64 as an exact (numerator, denominator) of ints."""
    return float(x).as_integer_ratio()


class Exact:
    """One metric of one series: metric row j is num[j] / den[j], its error scale M_win scale[j] / den[j], its window
    touching rows[j] rows."""

    def __init__(self, num, scale, den, rows):
        self.num, self.scale, self.den = num, scale, den
        self.rows = np.asarray(rows, dtype=np.int64)

    def value(self):
        """The exact values correctly rounded to float64."""
        return np.array([n / d for n, d in zip(self.num, self.den)], dtype=np.float64)

    def m_win(self):
        return np.array([s / d for s, d in zip(self.scale, self.den)], dtype=np.float64)

    def err_over_tol(self, got, tol_c=TOL_C):
        """|got - exact| / (tol_c u (rows + 2) M_win) per metric row, evaluated exactly and rounded once; inf where got
        is not finite or the window's terms are all 0 and got is not."""
        tc_n, tc_d = _ratio(tol_c)
        out = np.empty(len(self.num))
        for j, (n, s, d) in enumerate(zip(self.num, self.scale, self.den)):
            g = float(got[j])
            if not math.isfinite(g):
                out[j] = math.inf
                continue
            p, q = _ratio(g)
            diff = abs(p * d - n * q)                    # |got - exact| = diff / (q d)
            lim = q * s * tc_n * (int(self.rows[j]) + 2)  # tol = lim / (q d tc_d 2^53)
            if lim == 0:
                out[j] = 0.0 if diff == 0 else math.inf
            else:
                out[j] = (diff * tc_d * 2 ** 53) / lim
        return out


def _common(terms):
    """Exact (numerator, denominator) per term -> integers over one common denominator."""
    D = 1
    for _, d in terms:
        D = D * d // math.gcd(D, d)
    return [n * (D // d) for n, d in terms], D


def _terms(y, yhat, lo, hi):
    """Exact terms per quantity, as (numerator, denominator) pairs; None for a quantity that is not defined."""
    sq, ab, pe, cv = [], [], [], []
    for i in range(len(y)):
        yn, yd = _ratio(y[i])
        hn, hd = _ratio(yhat[i])
        en, ed = yn * hd - hn * yd, yd * hd            # err = y - yhat
        sq.append((en * en, ed * ed))
        ab.append((abs(en), ed))
        if yn != 0:
            pe.append((abs(en) * yd, ed * abs(yn)))     # |err / y|
        if lo is not None:
            cv.append((1 if (y[i] >= lo[i] and y[i] <= hi[i]) else 0, 1))
    return {'mse': sq, 'mae': ab, 'mape': pe if len(pe) == len(y) else None, 'coverage': cv if lo is not None else None}


def _windows(h, w):
    """Distinct horizons (ascending) and, per metric row, its (gb, ge, E): the window [E - w, E) lies in rows
    [gb, E) of the horizon-sorted rows, its leftmost group being [gb, ge)."""
    hs, counts = np.unique(h, return_counts=True)
    ends = np.cumsum(counts)
    starts = ends - counts
    out_h, spans = [], []
    for j in range(len(hs)):
        E = int(ends[j])
        if E < w:
            continue
        k = int(np.searchsorted(ends, E - w, side='right'))     # the group holding row E - w
        out_h.append(hs[j])
        spans.append((int(starts[k]), int(ends[k]), E))
    return np.array(out_h, dtype=np.int64), spans


def rolling_mean_exact(terms, h, w):
    """Windowed means of exact terms ((num, den) per row) grouped by horizon h: (horizons, Exact)."""
    h = np.asarray(h, dtype=np.int64)
    order = np.argsort(h, kind='stable')
    nums, D = _common([terms[i] for i in order])
    P = [0]
    for x in nums:
        P.append(P[-1] + x)
    hs, spans = _windows(h[order], w)
    num, scale, den, rows = [], [], [], []
    for gb, ge, E in spans:
        g = ge - gb
        num.append((P[E] - P[ge]) * g + (ge - E + w) * (P[ge] - P[gb]))
        scale.append((P[E] - P[gb]) * g)
        den.append(D * g * w)
        rows.append(E - gb)
    return hs, Exact(num, scale, den, rows)


def cv_metrics(y, yhat, h, w, yhat_lower=None, yhat_upper=None):
    """The exact metrics of one series.  y, yhat, yhat_lower, yhat_upper: float64 [n]; h: int64 horizons [n]; w: window
    rows.  Returns {'horizon': int64 [m], 'mse' / 'mae' / 'mape' / 'coverage': Exact, or None for mape when the series'
    min |y| < 1e-8 (NaN) and for coverage without intervals}."""
    y = np.asarray(y, dtype=np.float64)
    yhat = np.asarray(yhat, dtype=np.float64)
    assert len(y) == len(yhat) == len(h) and 1 <= w <= len(y)
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(yhat))
    t = _terms(y, yhat, yhat_lower, yhat_upper)
    if not (np.min(np.abs(y)) >= MAPE_MIN_ABS_Y):
        t['mape'] = None
    out = {}
    for name in METRICS:
        if t[name] is None:
            out[name] = None
            continue
        hs, ex = rolling_mean_exact(t[name], h, w)
        out['horizon'] = hs
        out[name] = ex
    return out
