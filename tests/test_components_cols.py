"""CPU tests of the forecast decomposition's host side: forecaster.component_columns against tables written out by
hand from fbprophet 0.5's regressor_column_matrix / add_group_component (column j of the design matrix belongs to the
component named before its '_delim_'; holidays, extra_regressors_<mode> and <mode>_terms group columns; pandas.crosstab
sorts the components by name; additive_terms / multiplicative_terms are appended empty when no column has their mode;
the 'zeros' placeholder is dropped), and the column layout of Components.frame (fbprophet 0.5's predict())."""
import numpy as np

from time_series_spark_amd import forecaster as fc

YEARLY = {'name': 'yearly', 'period': 365.25, 'fourier_order': 10}
WEEKLY = {'name': 'weekly', 'period': 7, 'fourier_order': 3}


def bits(*cols):
    m = 0
    for c in cols:
        m |= 1 << c
    return m


def span(a, b):
    return bits(*range(a, b))


def test_default_model_additive():
    spec = fc.ModelSpec(seasonalities=[YEARLY, WEEKLY])          # yearly: columns 0-19, weekly: 20-25
    assert fc.component_columns(spec) == [
        ('additive_terms', span(0, 26), 1),
        ('weekly', span(20, 26), 1),
        ('yearly', span(0, 20), 1),
        ('multiplicative_terms', 0, 0),
    ]


def test_default_model_multiplicative():
    spec = fc.ModelSpec(seasonality_mode='multiplicative', seasonalities=[YEARLY, WEEKLY])
    assert fc.component_columns(spec) == [
        ('multiplicative_terms', span(0, 26), 0),
        ('weekly', span(20, 26), 0),
        ('yearly', span(0, 20), 0),
        ('additive_terms', 0, 1),
    ]


def _holiday_spec(mode):
    holidays = [{'holiday': 'xmas', 'ds': ['2020-12-25', '2021-12-25'], 'lower_window': -1, 'upper_window': 1},
                {'holiday': 'easter', 'ds': ['2021-04-04']}]
    # the modeler's layout: holiday indicator columns first among the extras, sorted by name, in the model's mode
    extra = [{'name': n, 'prior_scale': 10.0, 'mode': mode}
             for n in ('easter_delim_+0', 'xmas_delim_+0', 'xmas_delim_+1', 'xmas_delim_-1')]
    return fc.ModelSpec(seasonality_mode=mode, seasonalities=[WEEKLY], extra=extra, holidays=holidays)


def test_two_holidays_with_windows():
    # weekly: columns 0-5; easter_delim_+0: 6; xmas_delim_+0, +1, -1: 7, 8, 9
    assert fc.component_columns(_holiday_spec('additive')) == [
        ('additive_terms', span(0, 10), 1),
        ('easter', bits(6), 1),
        ('holidays', span(6, 10), 1),
        ('weekly', span(0, 6), 1),
        ('xmas', bits(7, 8, 9), 1),
        ('multiplicative_terms', 0, 0),
    ]
    assert fc.component_columns(_holiday_spec('multiplicative')) == [
        ('easter', bits(6), 0),
        ('holidays', span(6, 10), 0),
        ('multiplicative_terms', span(0, 10), 0),
        ('weekly', span(0, 6), 0),
        ('xmas', bits(7, 8, 9), 0),
        ('additive_terms', 0, 1),
    ]


def test_regressors_of_both_modes():
    spec = fc.ModelSpec(seasonalities=[WEEKLY],
                        extra=[{'name': 'temp', 'mode': 'additive'}, {'name': 'promo', 'mode': 'multiplicative'},
                               {'name': 'rain', 'mode': 'additive'}])
    # weekly 0-5, temp 6, promo 7, rain 8
    assert fc.component_columns(spec) == [
        ('additive_terms', span(0, 7) | bits(8), 1),
        ('extra_regressors_additive', bits(6, 8), 1),
        ('extra_regressors_multiplicative', bits(7), 0),
        ('multiplicative_terms', bits(7), 0),
        ('promo', bits(7), 0),
        ('rain', bits(8), 1),
        ('temp', bits(6), 1),
        ('weekly', span(0, 6), 1),
    ]


def test_holidays_and_a_regressor():
    spec = _holiday_spec('additive')
    spec.extra.append({'name': 'temp', 'mode': 'multiplicative'})       # column 10
    assert fc.component_columns(spec) == [
        ('additive_terms', span(0, 10), 1),
        ('easter', bits(6), 1),
        ('extra_regressors_multiplicative', bits(10), 0),
        ('holidays', span(6, 10), 1),
        ('multiplicative_terms', bits(10), 0),
        ('temp', bits(10), 0),
        ('weekly', span(0, 6), 1),
        ('xmas', bits(7, 8, 9), 1),
    ]


def test_zeros_placeholder():
    # fbprophet's model without any seasonality: one column of zeros, no component of its own
    spec = fc.ModelSpec(seasonalities=[], extra=[{'name': 'zeros', 'prior_scale': 1.0, 'mode': 'additive'}])
    assert fc.component_columns(spec) == [('additive_terms', bits(0), 1), ('multiplicative_terms', 0, 0)]


def test_name_ordering():
    # crosstab's order is the names' sort order: upper case before lower case, '_' after upper-case letters
    seas = [{'name': 'monthly', 'period': 30.5, 'fourier_order': 2},                    # 0-3
            {'name': 'Quarterly', 'period': 91.3, 'fourier_order': 1},                  # 4-5
            {'name': 'b_mult', 'period': 3.5, 'fourier_order': 1, 'mode': 'multiplicative'},   # 6-7
            {'name': 'zz', 'period': 2.0, 'fourier_order': 1}]                          # 8-9
    spec = fc.ModelSpec(seasonalities=seas, extra=[{'name': 'A_reg', 'mode': 'additive'}])   # 10
    assert [n for n, _, _ in fc.component_columns(spec)] == [
        'A_reg', 'Quarterly', 'additive_terms', 'b_mult', 'extra_regressors_additive', 'monthly',
        'multiplicative_terms', 'zz']
    got = {n: (m, s) for n, m, s in fc.component_columns(spec)}
    assert got['additive_terms'] == (span(0, 6) | bits(8, 9, 10), 1)
    assert got['multiplicative_terms'] == (bits(6, 7), 0) and got['b_mult'] == (bits(6, 7), 0)


def _components(spec, names, N=2, H=5, intervals=False):
    rng = np.random.default_rng(1)
    arr = lambda: rng.normal(size=(N, H))                       # noqa: E731
    comp = rng.normal(size=(N, len(names), H))
    iv = [arr() for _ in range(4)] if intervals else [None] * 4
    return fc.Components(spec, names, arr(), arr(), comp, *iv, floor=np.array([0.5, -1.0]),
                         cap=np.array([9.0, 7.0]))


def _want(growth, intervals, names):
    cols = ['ds', 'trend'] + (['cap', 'floor'] if growth == 'logistic' else [])
    if intervals:
        cols += ['yhat_lower', 'yhat_upper', 'trend_lower', 'trend_upper']
    for n in names:
        cols += [n, n + '_lower', n + '_upper']
    return cols + ['yhat']


def test_frame_layout():
    ds = np.datetime64('2021-01-01', 'ns').astype(np.int64) + 86400 * 10 ** 9 * np.arange(5)
    for growth in ('linear', 'logistic'):
        spec = fc.ModelSpec(growth=growth, seasonalities=[WEEKLY])
        names = [n for n, _, _ in fc.component_columns(spec)]
        for intervals in (False, True):
            c = _components(spec, names, intervals=intervals)
            df = c.frame(1, ds)
            assert list(df.columns) == _want(growth, intervals, names), (growth, intervals)
            assert len(df) == 5 and df['ds'].dtype == np.dtype('datetime64[ns]')
            assert (df['ds'].values.view(np.int64) == ds).all()
            assert np.array_equal(df['yhat'].values, c.yhat[1]) and np.array_equal(df['trend'].values, c.trend[1])
            for n in names:
                v = c.terms[n][1]
                assert np.array_equal(df[n].values, v) and np.array_equal(df[n + '_lower'].values, v)
                assert np.array_equal(df[n + '_upper'].values, v)
            if intervals:
                assert np.array_equal(df['trend_lower'].values, c.trend_lower[1])
                assert np.array_equal(df['yhat_upper'].values, c.yhat_upper[1])
            if growth == 'logistic':
                assert (df['cap'] == 7.0).all() and (df['floor'] == -1.0).all()
                df2 = c.frame(0, ds.astype('datetime64[ns]'), cap=3.0, floor=0.0)
                assert (df2['cap'] == 3.0).all() and (df2['floor'] == 0.0).all()


def test_terms_are_views_of_one_array():
    spec = fc.ModelSpec(seasonalities=[YEARLY, WEEKLY])
    names = [n for n, _, _ in fc.component_columns(spec)]
    c = _components(spec, names)
    for i, n in enumerate(names):
        assert np.shares_memory(c.terms[n], c.comp) and np.array_equal(c.terms[n], c.comp[:, i, :])
