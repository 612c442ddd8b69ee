"""CPU tests of the exact cross-validation metrics reference (oracle/cv_metrics_ref.py): it equals Prophet's
rolling_mean_by_h restated literally (tests/test_cv_plan.py) where that is exact or benign, its tolerance is calibrated
on float64 emulations of sound summation orders, and the tolerance rejects the ways a metrics kernel goes wrong -- a
window formed as a difference of prefix sums, a window of w +- 1 rows, the leftmost group taken whole or weighted
wrongly, and mape's NaN threshold taken as <=.  No GPU."""
import numpy as np
import pytest

from oracle import cv_metrics_ref as ref
from tests.test_cv_plan import rolling_mean_by_h, window_rows

U = ref.U


# ---- float64 emulations of ways to evaluate the windows ------------------------------------------------------------

def _terms(y, yh, lo=None, hi=None):
    err = y - yh
    t = {'mse': err * err, 'mae': np.abs(err), 'mape': np.abs(err / y)}
    if lo is not None:
        t['coverage'] = ((y >= lo) & (y <= hi)).astype(np.float64)
    return t


def _spans(h, w):
    order = np.argsort(h, kind='stable')
    hs, spans = ref._windows(h[order], w)
    return order, hs, spans


def _seq(a):
    """Left-to-right float64 sum (np.cumsum is sequential; np.sum is pairwise)."""
    return float(np.cumsum(a)[-1]) if len(a) else 0.0


def emulate(kind, x, h, w, weight=None):
    """Windowed means of float64 terms x [n] by horizon h, evaluated in float64 as `kind` does it:
      'seq'     each window's touched rows summed left to right: whole part [ge, E), leftmost group [gb, ge);
      'groups'  each window as the sum of its touched groups' sums minus the leftmost group's excess share
                (rolling_mean_by_h's formula, sums formed afresh per window);
      'tree'    the sums as pairwise block sums (a tree over the sorted rows), a window from its O(log n) nodes;
      'prefix'  running prefix sums over all rows, a window as differences of them (cancels);
      'whole'   the leftmost group taken whole;
    weight(gb, ge, E, w) overrides the leftmost group's included share (for the kernel-bug models)."""
    order, hs, spans = _spans(h, w)
    t = x[order]
    out = np.empty(len(spans))
    if kind == 'prefix':
        P = np.concatenate([[0.0], np.cumsum(t)])
    if kind == 'groups':
        _, g_start = np.unique(h[order], return_index=True)
        g_sum = np.array([_seq(t[a:b]) for a, b in zip(g_start, list(g_start[1:]) + [len(t)])])
    if kind == 'tree':
        levels = [t]
        while len(levels[-1]) > 1:
            a = levels[-1]
            b = np.zeros((len(a) + 1) // 2)
            b += a[0::2]
            b[:len(a) // 2] += a[1::2]
            levels.append(b)

        def S(lo, hi):
            s, k = 0.0, 0
            while lo < hi:
                if lo & 1:
                    s += levels[k][lo]
                    lo += 1
                if hi & 1:
                    hi -= 1
                    s += levels[k][hi]
                lo, hi, k = lo >> 1, hi >> 1, k + 1
            return s
    for j, (gb, ge, E) in enumerate(spans):
        g = ge - gb
        inc = float(ge - E + w) if weight is None else float(weight(gb, ge, E, w))
        if kind == 'seq':
            out[j] = (_seq(t[ge:E]) + inc * _seq(t[gb:ge]) / g) / w
        elif kind == 'groups':
            kb = int(np.searchsorted(g_start, gb))
            ke = int(np.searchsorted(g_start, E))
            out[j] = (_seq(g_sum[kb:ke]) - (g - inc) * g_sum[kb] / g) / w
        elif kind == 'tree':
            out[j] = (S(ge, E) + inc * S(gb, ge) / g) / w
        elif kind == 'prefix':
            out[j] = (P[E] - P[gb] - (g - inc) * (P[ge] - P[gb]) / g) / w
        elif kind == 'whole':
            out[j] = _seq(t[gb:E]) / w
    return hs, out


def _ratios(kind, y, yh, h, w, tol_c=ref.TOL_C, lo=None, hi=None, **kw):
    """err / tol of an emulation against the reference, per metric: {name: array}."""
    r = ref.cv_metrics(y, yh, h, w, lo, hi)
    out = {}
    for name, x in _terms(y, yh, lo, hi).items():
        if r[name] is None:
            continue
        hs, got = emulate(kind, x, h, w, **kw)
        assert np.array_equal(hs, r['horizon'])
        out[name] = r[name].err_over_tol(got, tol_c)
    return out


# ---- panels -------------------------------------------------------------------------------------------------------

def aligned_horizons(C, H):
    """C folds of H daily horizons each (an aligned panel's holdout rows, fold by fold)."""
    return np.tile(np.arange(1, H + 1, dtype=np.int64), C)


def benign(rng, n_kind):
    """(y, yhat, h, lo, hi): an aligned or ragged holdout of moderate values."""
    if n_kind == 'aligned':
        C, H = int(rng.integers(1, 12)), int(rng.integers(1, 120))
        h = aligned_horizons(C, H)
    else:
        h = np.sort(rng.integers(1, 200, size=int(rng.integers(1, 600)))).astype(np.int64)
        rng.shuffle(h)
    n = len(h)
    y = np.round(np.exp(rng.normal(np.log(3e4), 1.0)) * (1 + 0.2 * rng.standard_normal(n)))
    y[y == 0] = 1.0
    yh = y + rng.normal(0, 0.05 * np.abs(y).mean() + 1, n)
    lo, hi = yh - np.abs(rng.normal(0, 0.1 * np.abs(y).mean(), n)), yh + np.abs(rng.normal(0, 0.1 * np.abs(y).mean(), n))
    return y, yh, h, lo, hi


def spike_panel():
    """The issue's panel: 9 folds x 90 daily horizons, errors N(0, 10), one error of 1e10 at horizon 1."""
    rng = np.random.default_rng(20261015)
    h = aligned_horizons(9, 90)
    y = 1e3 + np.round(rng.normal(0, 100, len(h)))
    yh = y - rng.normal(0, 10, len(h))
    yh[8 * 90] = y[8 * 90] - 1e10               # the last fold's first holdout row
    return y, yh, h


# ---- the reference against the literal restatement -----------------------------------------------------------------

def _exact_floats(x, h, w):
    return ref.rolling_mean_exact([v.as_integer_ratio() for v in np.asarray(x, np.float64)], h, w)


def test_hand_cases_exact():
    """tests/test_cv_plan.py's hand-worked cases: the reference's values are the exact ones."""
    x, h = np.array([1.0, 3.0, 2.0, 4.0, 10.0]), np.array([1, 1, 2, 2, 3])
    hs, e = _exact_floats(x, h, 1)
    assert list(hs) == [1, 2, 3] and list(e.value()) == [2.0, 3.0, 10.0]
    hs, e = _exact_floats(x, h, 3)
    assert list(hs) == [2, 3] and list(e.value()) == [8 / 3, 16 / 3]
    assert list(e.rows) == [4, 3] and list(e.m_win()) == [10 / 3, 16 / 3]
    x, h = np.array([4.0, 4.0, 8.0, 8.0, 1.0]), np.array([5, 5, 5, 5, 9])
    hs, e = _exact_floats(x, h, 4)
    assert list(hs) == [5, 9] and list(e.value()) == [6.0, 19 / 4]
    hs, e = _exact_floats(x, h, 5)
    assert list(hs) == [9] and list(e.value()) == [5.0]
    for x, h, w in (([1.0, 3.0, 2.0, 4.0, 10.0], [1, 1, 2, 2, 3], 2), ([4.0, 4.0, 8.0, 8.0, 1.0], [5, 5, 5, 5, 9], 3)):
        hs, e = _exact_floats(x, h, w)
        hl, want = rolling_mean_by_h(np.array(x), np.array(h), w)
        assert np.array_equal(hs, hl) and np.array_equal(e.value(), want)


def test_random_benign_equals_literal():
    """On random benign holdouts the literal rolling_mean_by_h agrees with the reference, metric row by metric row, for
    window sizes from 1 to n.  The literal's running sum also carries the rounding of groups that have left the window
    (it subtracts them), so its error scale is that of every row it has summed, [gb, n), not the window's own."""
    rng = np.random.default_rng(7)
    for trial in range(60):
        y, yh, h, lo, hi = benign(rng, 'aligned' if trial % 2 else 'ragged')
        w = window_rows(float(rng.choice([0.0, 0.05, 0.1, 0.33, 0.5, 1.0])), len(h))
        r = ref.cv_metrics(y, yh, h, w, lo, hi)
        order, _, spans = _spans(h, w)
        gb = np.array([s[0] for s in spans])
        for name, x in _terms(y, yh, lo, hi).items():
            hs, want = rolling_mean_by_h(x, h, w)
            assert np.array_equal(hs, r['horizon'])
            e = r[name]
            tail = np.cumsum(x[order][::-1])[::-1][gb] / w                  # S[gb, n) / w
            m = e.m_win()
            scale = np.where(m > 0, (len(h) - gb + 2) * tail / ((e.rows + 2) * np.where(m > 0, m, 1.0)), 0.0)
            assert np.all(e.err_over_tol(want) <= scale), (trial, name)


def test_mape_threshold_and_undefined():
    """mape is NaN (None here) for the whole series iff min |y| < 1e-8 -- 1e-8 itself is in; coverage only with
    intervals; a zero y makes mape NaN, not a division by zero."""
    h = np.array([1, 2, 3, 4])
    for ymin, defined in ((0.0, False), (0.99e-8, False), (1e-8, True), (1.01e-8, True), (-1e-8, True),
                          (-0.99e-8, False)):
        y = np.array([5.0, ymin, 7.0, 9.0])
        r = ref.cv_metrics(y, y + 1.0, h, 2)
        assert (r['mape'] is not None) == defined, ymin
        assert r['coverage'] is None
    y = np.array([5.0, 2.0 ** -26, 7.0, 9.0])
    r = ref.cv_metrics(y, y + 1.0, h, 1)
    assert r['mape'].value()[1] == 2.0 ** 26 and r['mse'].value().tolist() == [1.0] * 4


# ---- calibration ---------------------------------------------------------------------------------------------------

def test_tolerance_calibrated():
    """Calibration of the metrics tolerance TOL_C u (E - gb + 2) M_win (oracle/cv_metrics_ref.py) on float64 emulations
    of three sound orders -- each window's touched rows summed in sequence, the sum of its touched groups minus the
    leftmost group's excess share, and pairwise block sums of a tree -- over random benign holdouts, the spike panel
    and panels whose errors run from e^-40 to e^40.  The largest err / (u (E - gb + 2) M_win) measured is 0.66,
    the same for all three orders: w = 1 on the wide-range panels, where a squared error's two roundings meet a bound
    of (1 + 2) u.  TOL_C = 4 is the first-order bound (about one rounding per touched row, a few per term, the weight
    and the division) and leaves a factor of 6 over what was measured."""
    rng = np.random.default_rng(11)
    panels = [benign(rng, 'aligned' if i % 2 else 'ragged')[:3] for i in range(40)]
    panels.append(spike_panel())
    for i in range(10):                                        # terms over ~40 orders of magnitude
        y, yh, h, _, _ = benign(rng, 'ragged')
        yh = y - np.exp(rng.uniform(-40, 40, len(y))) * rng.choice([-1.0, 1.0], len(y))
        panels.append((y, yh, h))
    worst = {}
    for kind in ('seq', 'groups', 'tree'):
        for y, yh, h in panels:
            for rw in (0.0, 0.1, 0.5, 1.0):
                w = window_rows(rw, len(h))
                for name, r in _ratios(kind, y, yh, h, w, tol_c=1.0).items():
                    worst[kind] = max(worst.get(kind, 0.0), float(r.max()))
    assert max(worst.values()) <= ref.TOL_C / 4, worst        # headroom against the next shape
    assert max(worst.values()) >= 0.05, worst                  # the tolerance is not loose by orders of magnitude


# ---- the bound rejects the bugs -------------------------------------------------------------------------------------

def test_rejects_prefix_differences_on_spike_panel():
    """The issue's panel: prefix sums over all rows and windows as their differences lose every window after the
    spike (their mse comes out as 0 or negative); a sound order passes on the same panel."""
    y, yh, h = spike_panel()
    w = window_rows(0.1, len(h))
    bad = _ratios('prefix', y, yh, h, w)
    assert bad['mse'].max() > 1e6 and bad['mae'].max() > 1.0
    _, got = emulate('prefix', _terms(y, yh)['mse'], h, w)
    r = ref.cv_metrics(y, yh, h, w)
    exact = r['mse'].value()
    assert np.sum(np.abs(got - exact) > 0.5 * exact) >= 80      # meaningless, not slightly off
    for kind in ('seq', 'groups', 'tree'):
        assert max(v.max() for v in _ratios(kind, y, yh, h, w).values()) <= 1.0, kind


@pytest.mark.parametrize('dw', [-1, 1])
def test_rejects_window_off_by_one(dw):
    rng = np.random.default_rng(3)
    for trial in range(8):
        y, yh, h, _, _ = benign(rng, 'aligned' if trial % 2 else 'ragged')
        if len(h) < 4:
            continue
        w = window_rows(0.2, len(h))
        r = ref.cv_metrics(y, yh, h, w)
        hs, got = emulate('seq', _terms(y, yh)['mse'], h, w + dw)
        common, ia, ib = np.intersect1d(r['horizon'], hs, return_indices=True)
        assert len(common) > 0
        full = np.full(len(r['horizon']), np.nan)
        full[ia] = got[ib]
        assert np.nanmax(r['mse'].err_over_tol(full)[ia]) > 1.0, trial


def test_rejects_leftmost_group_whole_and_wrong_weight():
    """Aligned panels (groups of C rows) with w not a multiple of C: the leftmost group is partial in every window."""
    rng = np.random.default_rng(5)
    bugs = {'whole': dict(kind='whole'),
            'share + 1 row': dict(kind='seq', weight=lambda gb, ge, E, w: ge - E + w + 1),
            'excess for share': dict(kind='seq', weight=lambda gb, ge, E, w: E - gb - w),
            'share of E - w': dict(kind='seq', weight=lambda gb, ge, E, w: E - w - gb)}
    for label, kw in bugs.items():
        for trial in range(4):
            C, H = 9, 90
            y, yh, h, _, _ = benign(rng, 'aligned')
            h = aligned_horizons(C, H)
            y, yh = np.resize(y, len(h)) + 1.0, np.resize(yh, len(h))
            w = 85
            r = ref.cv_metrics(y, yh, h, w)
            for name, x in _terms(y, yh).items():
                hs, got = emulate(kw['kind'], x, h, w, weight=kw.get('weight'))
                assert r[name].err_over_tol(got).max() > 1.0, (label, name, trial)


def test_rejects_mape_threshold_le():
    """A series whose min |y| is exactly 1e-8 has a defined mape; a kernel testing <= 1e-8 returns NaN, which the
    reference's err / tol rejects (not finite)."""
    y = np.array([3.0, 1e-8, 4.0, 5.0, 6.0])
    yh = y + np.array([0.5, 1e-9, -0.25, 1.0, 2.0])
    h = np.arange(1, 6)
    r = ref.cv_metrics(y, yh, h, 2)
    assert r['mape'] is not None
    buggy = np.full(len(r['horizon']), np.nan) if np.min(np.abs(y)) <= 1e-8 else None
    assert np.all(r['mape'].err_over_tol(buggy) == np.inf)
    _, good = emulate('seq', _terms(y, yh)['mape'], h, 2)
    assert r['mape'].err_over_tol(good).max() <= 1.0


def test_exact_reference_scales_to_thousands_of_rows():
    """A 4 100-row holdout with distinct integer y (mape denominators that do not reduce) stays cheap."""
    import time
    rng = np.random.default_rng(9)
    n = 4100
    y = rng.integers(1000, 100000, n).astype(np.float64)
    yh = y + rng.normal(0, 300, n)
    h = np.arange(1, n + 1, dtype=np.int64)
    t0 = time.time()
    r = ref.cv_metrics(y, yh, h, window_rows(0.1, n))
    assert len(r['horizon']) == n - 409
    assert r['mape'].err_over_tol(emulate('tree', _terms(y, yh)['mape'], h, 410)[1]).max() <= 1.0
    assert time.time() - t0 < 60
