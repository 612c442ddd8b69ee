"""The two short cuts of cubic_interp6s (csrc/tsf_quad_kernels.h) return the bits of Stan's CubicInterp as the oracle
writes it (oracle/prophet_canon.c cubic_interp6), on every input: x1 == 1 makes the three divisions by x1^3, x1, x1^2
divisions by 1.0, and a negative c2^2 - 2 c1 c3 makes both roots NaN, which no range test admits.  Restated here in IEEE
double arithmetic (numpy float64 scalars: one rounding per operation, nothing fused) and compared on operands of a line
search's size, on a grid of special values (zeros of both signs, subnormals, huge, infinite, NaN) and on cases built to
sit at the boundary of either short cut.  No GPU: the kernels' side is tests/test_gpu_quad_line_search.py."""
import itertools

import numpy as np

F = np.float64
LO, HI = F(1e-12), F(1.0)


def _poly(x, c1, c2, c3):
    return x * (x * (x * c3 / F(3.0) + c2) / F(2.0) + c1)


def _tail(c1, c2, c3, t_s, lo, hi):
    s1 = -(c2 + t_s) / c3
    s2 = -(c2 - t_s) / c3
    min_f, min_x = _poly(lo, c1, c2, c3), lo
    tmp = _poly(hi, c1, c2, c3)
    if tmp < min_f:
        min_f, min_x = tmp, hi
    for s in (s1, s2):
        if lo < s and s < hi:
            tmp = _poly(s, c1, c2, c3)
            if tmp < min_f:
                min_f, min_x = tmp, s
    return min_x


def reference(df0, x1, f1, df1, lo=LO, hi=HI):
    """oracle/prophet_canon.c cubic_interp6, operation for operation"""
    c3 = (F(-12.0) * f1 + F(6.0) * x1 * (df0 + df1)) / (x1 * x1 * x1)
    c2 = -(F(4.0) * df0 + F(2.0) * df1) / x1 + F(6.0) * f1 / (x1 * x1)
    c1 = df0
    return _tail(c1, c2, c3, np.sqrt(c2 * c2 - F(2.0) * c1 * c3), lo, hi)


def shortcut(df0, x1, f1, df1, lo=LO, hi=HI):
    """cubic_interp6s; returns (value, which short cuts were taken)"""
    n3, n2a, n2b = F(-12.0) * f1 + F(6.0) * x1 * (df0 + df1), -(F(4.0) * df0 + F(2.0) * df1), F(6.0) * f1
    took = ''
    if x1 == F(1.0):
        c3, c2 = n3, n2a + n2b
        took += 'u'
    else:
        c3, c2 = n3 / (x1 * x1 * x1), n2a / x1 + n2b / (x1 * x1)
    c1 = df0
    disc = c2 * c2 - F(2.0) * c1 * c3
    if disc < F(0.0):
        return (hi if _poly(hi, c1, c2, c3) < _poly(lo, c1, c2, c3) else lo), took + 'n'
    return _tail(c1, c2, c3, np.sqrt(disc), lo, hi), took


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.array([a]).view(np.int64)[0] == np.array([b]).view(np.int64)[0]


def _check(cases):
    seen = {'': 0, 'u': 0, 'n': 0, 'un': 0}
    with np.errstate(all='ignore'):
        for df0, x1, f1, df1 in cases:
            args = (F(df0), F(x1), F(f1), F(df1))
            got, took = shortcut(*args)
            assert _same(got, reference(*args)), (args, got, reference(*args), took)
            seen[took] += 1
    return seen


def test_operands_of_a_line_search():
    """slopes and decreases of the sizes a fit sees, previous steps 1 and not 1: every combination of short cuts is taken
    thousands of times"""
    rng = np.random.default_rng(20260417)
    n = 40000
    df0 = -np.exp(rng.uniform(-12, 6, n))
    df1 = df0 * np.exp(rng.normal(0, 2, n)) * np.where(rng.uniform(size=n) < 0.15, -1.0, 1.0)
    x1 = np.where(rng.uniform(size=n) < 0.6, 1.0, np.exp(rng.uniform(-6, 3, n)))
    f1 = x1 * df0 * rng.uniform(-0.5, 2.0, n)
    seen = _check(zip(df0, x1, f1, df1))
    assert min(seen.values()) > 1000, seen


def test_special_values():
    vals = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-12, 0.5, -0.5, 1.0, -1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53,
            3.0, -7.25, 1e150, -1e150, 1e300, -1e300, np.inf, -np.inf, np.nan]
    seen = _check(itertools.product(vals, repeat=4))
    assert seen['u'] > 10000 and seen['n'] > 100 and seen['un'] > 10, seen


def test_at_the_boundary_of_the_short_cuts():
    """c2^2 - 2 c1 c3 at zero and one rounding either side of it, and x1 one ulp either side of 1.  At x1 = 1,
    c3 = -12 f1 + 6 (df0 + df1) and c2 = -(4 df0 + 2 df1) + 6 f1: the discriminant is a parabola in f1 that opens upwards;
    from its lowest point, where it is negative in these cases, f1 is bisected up to the sign change."""
    cases = []
    rng = np.random.default_rng(7)
    with np.errstate(all='ignore'):
        for _ in range(2000):
            df0, df1 = -np.exp(rng.uniform(-3, 3)), -np.exp(rng.uniform(-3, 3))

            def disc(f1):
                c3 = F(-12.0) * F(f1) + F(6.0) * (F(df0) + F(df1))
                c2 = -(F(4.0) * F(df0) + F(2.0) * F(df1)) + F(6.0) * F(f1)
                return c2 * c2 - F(2.0) * F(df0) * c3
            a = -(4.0 * df0 + 2.0 * df1)
            lo, hi = -(12.0 * a + 24.0 * df0) / 72.0, 1e3        # the parabola's lowest point; far up it is positive
            if not (disc(lo) < 0 and disc(hi) > 0):
                continue
            for _ in range(80):
                mid = 0.5 * (lo + hi)
                if disc(mid) < 0:
                    lo = mid
                else:
                    hi = mid
            for f1 in (lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)):
                for x1 in (1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)):
                    cases.append((df0, x1, f1, df1))
    seen = _check(cases)
    assert seen['un'] > 500 and seen['u'] > 500 and seen['n'] + seen[''] > 1000, seen
