"""Reference statements for conditional seasonalities (include/tsf.h "conditional seasonalities") -- TEST
INFRASTRUCTURE ONLY.  `columns` is the literal fbprophet statement (fourier_series, then
make_all_seasonality_features' `features[~df[condition_name]] = 0`), restated from recall of fbprophet 0.5;
`canonical_columns` the canonical oracle's values of the same seasonality (the bits the library must produce) times
the mask; `extended_columns` the same statement in extended precision and `rounding_bound` the distance the number
format allows between the two double-precision ones; `season_flip_panel` the inputs of the "it models what it says" test."""
import numpy as np

from tests import helpers

DAY_NS = 86400 * 10 ** 9


def columns(ds_ns, period, order, mask):
    """[rows][2 * order]: sin / cos of 2 pi h t / period (t in days since the epoch), h = 1 .. order, in fbprophet's
    column order [sin 1, cos 1, sin 2, ...]; the rows where mask is false are 0."""
    t = np.asarray(ds_ns, dtype=np.int64).astype(np.float64) / 1e9 / 86400.0
    out = np.column_stack([fun(2.0 * (h + 1) * np.pi * t / period) for h in range(order) for fun in (np.sin, np.cos)])
    out[~np.asarray(mask, dtype=bool)] = 0.0
    return out


def extended_columns(ds_ns, period, order, mask):
    """[rows][2 * order]: `columns` evaluated in numpy's longdouble (64-bit mantissa on x86-64) from the integer
    timestamps -- what both double-precision statements are measured against."""
    ld = np.longdouble
    t = np.asarray(ds_ns, dtype=np.int64).astype(ld) / ld(10 ** 9) / ld(86400)
    pi = ld('3.14159265358979323846264338327950288')
    out = np.column_stack([fun(2 * ld(h + 1) * pi * t / ld(period)) for h in range(order) for fun in (np.sin, np.cos)])
    out[~np.asarray(mask, dtype=bool)] = 0.0
    return out


def rounding_bound(ds_ns, period, order):
    """Worst-case |literal - canonical| from the number format alone, u = 2^-53, X = max |2 pi order t / period|:
      * literal: the argument 2.0 * h * pi * t / period carries pi's own representation error (0.35 u), the two
        roundings of t = ns / 1e9 / 86400 and three of the products and the quotient: relative error < 6 u, so the
        argument is off by < 6 u X and sin / cos (Lipschitz 1) by that plus numpy's own < 1 ulp (u);
      * canonical: the first harmonic's argument 2 pi t / period is built with the same count of roundings (< 6 u
        relative); harmonic h of the recurrence is sin / cos of h times that argument, so its error is < 6 u X again,
        plus the recipe's 2 ulp (tsf_detmath.h: < 3 u) carried through a three-term recurrence whose rounding and
        starting errors grow at most like h^2 (< 3 u (h^2 + 2) together).
    Sum: 12 u X + 3 u (order^2 + 3).  A wrong harmonic, sign or column order is an error of order 1."""
    u = 2.0 ** -53
    t_max = float(np.abs(np.asarray(ds_ns, dtype=np.int64)).max()) / 1e9 / 86400.0
    X = 2.0 * np.pi * order * t_max / period
    return 12.0 * u * X + 3.0 * u * (order * order + 3)


def canonical_columns(ds_ns, period, order, mask):
    """[2 * order][rows]: the canonical oracle's design values of an UNCONDITIONAL seasonality of this period and order
    (oracle/canon_lib.design through helpers.canonical_fourier) where mask is true, +0.0 where it is false."""
    X = helpers.canonical_fourier(np.asarray(ds_ns, dtype=np.int64).astype('datetime64[ns]'), period, order)
    return np.where(np.asarray(mask, dtype=bool)[None, :], X.T, 0.0)


def season_flip_panel(N=3, T=210, seed=7):
    """(ds, y [N][T], in_season [T]): daily series on a gentle linear trend whose weekly pattern FLIPS SIGN between the
    season (every other block of five weeks) and the rest, with light noise: one weekly seasonality fits the average of
    the two patterns -- nearly nothing --, an in-season / off-season pair fits both."""
    rng = np.random.RandomState(seed)
    ds = (np.datetime64('2019-01-07', 'ns').astype(np.int64) + DAY_NS * np.arange(T)).astype(np.int64)   # a Monday
    day = np.arange(T)
    in_season = (day // 35) % 2 == 0
    week = np.array([3.0, 1.0, -2.0, -4.0, 0.0, 2.5, -0.5])
    y = np.zeros((N, T))
    for n in range(N):
        amp = 4.0 + n
        y[n] = 100.0 + 10.0 * n + 0.05 * (n + 1) * day + amp * week[day % 7] * np.where(in_season, 1.0, -1.0) \
            + 0.2 * rng.standard_normal(T)
    return ds, y, in_season
