"""GPU tests of the `_dev` forecast entries (tsf_predict_intervals_dev, tsf_predict_components_dev,
tsf_predict_quantiles_dev, tsf_score_actuals_dev) called the way include/tsf.h means them to be called: every input and
output in device memory (torch tensors), on a caller stream that is not the default one.

What pins them: the host entry of the same name on the same arguments, bit for bit.  The host entries are pinned to the
oracle and to each other by tests/test_gpu_forecast.py, test_gpu_components.py, test_gpu_quantiles.py and
test_gpu_scores.py; their several-chunk runs pin the chunk loop, so the shapes here are the two small interval cases of
tests/forecast_cases.py (per-series and shared future grids, logistic growth with a floor, linear growth with extra
columns) with 3 samples: a sample count that is not the padded sort width."""
import ctypes

import numpy as np
import pytest
# at collection, before anything loads libtsf_amd.so (as in bench.py): a torch wheel carries a HIP runtime of its own,
# and the library binds to the runtime that is loaded first -- loaded after the library, torch would start a second
# runtime in the process and see no GPU
import torch

from tests import forecast_cases as fcs

pytestmark = pytest.mark.gpu

N_SAMPLES = 3
WIDTH = 0.8
SEED = 23
LEVELS = np.array([0.1, 0.9])
NAMES = ['iv65', 'iv129']


@pytest.fixture(scope='module')
def env(built):
    from time_series_spark_amd import _lib, forecaster as fc
    if _lib.load().tsf_device_count() < 1:
        pytest.fail('no GPU visible: GPU tests of the _dev entries cannot run (product has no CPU fallback)')
    return fc, _lib, torch


class Call(object):
    """One case's forecast inputs on the host and on the device, and the two ways to run an entry on them."""

    def __init__(self, env, name, keyed):
        self.fc, self.lib, self.torch = env
        self.L = self.lib.load()
        self.ctx = self.fc.get_context()
        c = self.c = fcs.make(name)
        self.cs = c.spec.to_c()
        key = np.arange(c.N, dtype=np.int64) * 6151 + 11 if keyed else None
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)    # noqa: E731
        self.host = dict(theta=f64(c.theta), y_scale=f64(c.y_scale),
                         grid=np.ascontiguousarray(c.grid, dtype=self.lib.GRID_DTYPE).view(np.uint8),
                         fut=np.ascontiguousarray(c.fut, dtype=np.int64), floor=f64(c.floor), cap=f64(c.cap),
                         extra=f64(c.extra), key=key)
        self.dev = {k: self.to_dev(v) for k, v in self.host.items()}

    def to_dev(self, a):
        return None if a is None else self.torch.from_numpy(a).cuda()

    def out_dev(self, like):
        """a device output of the host output's shape, filled with what no entry writes"""
        t = self.torch.from_numpy(like).cuda()
        return t.fill_(-7 if like.dtype.kind == 'i' else float('nan'))

    def head(self, a):
        """the arguments every forecast entry starts with, from host arrays or device tensors"""
        return [self.ctx.handle, ctypes.byref(self.cs), self.c.N, self.c.H, ptr(a['theta']), ptr(a['y_scale']),
                ptr(a['grid']), len(self.c.grid), ptr(a['fut']), int(self.c.shared), ptr(a['floor']), ptr(a['cap']),
                ptr(a['extra'])]

    def run(self, entry, host_args, dev_args):
        """the host entry, then the _dev entry on a stream of its own; the outputs are the callers'"""
        self.ctx.check(getattr(self.L, entry)(*host_args))
        self.torch.cuda.synchronize()                   # the device inputs and output fills are on the default stream
        st = self.torch.cuda.Stream()
        assert st.cuda_stream != 0
        self.ctx.check(getattr(self.L, entry + '_dev')(*(dev_args + [ctypes.c_void_p(st.cuda_stream)])))
        st.synchronize()


def ptr(a):
    if a is None:
        return None
    return a.data_ptr() if hasattr(a, 'data_ptr') else a.ctypes.data


def same(dev, host):
    got = dev.cpu().numpy()
    assert got.shape == host.shape and got.dtype == host.dtype
    if host.dtype == np.float64:
        return np.array_equal(got.view(np.int64), host.view(np.int64))
    return np.array_equal(got, host)


@pytest.mark.parametrize('keyed', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_intervals_dev(env, name, keyed):
    k = Call(env, name, keyed)
    c = k.c
    host = [np.zeros((c.N, c.H)) for _ in range(3)]
    dev = [k.out_dev(a) for a in host]
    tail = [N_SAMPLES, WIDTH, SEED]
    k.run('tsf_predict_intervals', k.head(k.host) + [ptr(k.host['key'])] + tail + [ptr(a) for a in host],
          k.head(k.dev) + [ptr(k.dev['key'])] + tail + [ptr(a) for a in dev])
    for what, d, h in zip(('yhat', 'yhat_lower', 'yhat_upper'), dev, host):
        assert same(d, h), what
    assert (host[1] <= host[2]).all() and (host[1] < host[2]).any()


@pytest.mark.parametrize('keyed', [True, False])
@pytest.mark.parametrize('n_samples', [0, N_SAMPLES])
@pytest.mark.parametrize('name', NAMES)
def test_components_dev(env, name, n_samples, keyed):
    k = Call(env, name, keyed)
    c = k.c
    cols = k.fc.component_columns(c.spec)
    C = len(cols)
    assert C > 0 and any(m for _, m, _ in cols)
    masks = np.array([int(m) for _, m, _ in cols], dtype=np.uint64)         # host data in both entries
    scaled = np.array([int(s) for _, _, s in cols], dtype=np.int32)
    names = ['yhat', 'trend', 'comp'] + (['yhat_lower', 'yhat_upper', 'trend_lower', 'trend_upper'] if n_samples else [])
    host = [np.zeros((c.N, C, c.H) if w == 'comp' else (c.N, c.H)) for w in names]
    dev = [k.out_dev(a) for a in host]
    pad = [None] * (7 - len(names))
    mid = [C, masks.ctypes.data, scaled.ctypes.data]
    tail = [n_samples, WIDTH, SEED]
    k.run('tsf_predict_components', k.head(k.host) + mid + [ptr(k.host['key'])] + tail + [ptr(a) for a in host] + pad,
          k.head(k.dev) + mid + [ptr(k.dev['key'])] + tail + [ptr(a) for a in dev] + pad)
    for what, d, h in zip(names, dev, host):
        assert same(d, h), what
    assert host[2].any()


@pytest.mark.parametrize('keyed', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_quantiles_dev(env, name, keyed):
    k = Call(env, name, keyed)
    c = k.c
    Q = len(LEVELS)
    host = {w: np.zeros((c.N, Q, c.H)) for w in ('q', 'cum_q', 'trend_q')}
    host.update({w: np.zeros((c.N, c.H, N_SAMPLES)) for w in ('samples', 'trend_samples')})
    host['yhat'] = np.zeros((c.N, c.H))
    dev = {w: k.out_dev(a) for w, a in host.items()}
    ho = k.lib.TsfQuantileOut(**{w: ptr(a) for w, a in host.items()})
    do = k.lib.TsfQuantileOut(**{w: ptr(a) for w, a in dev.items()})
    tail = [N_SAMPLES, SEED, Q, LEVELS.ctypes.data]
    k.run('tsf_predict_quantiles', k.head(k.host) + [ptr(k.host['key'])] + tail + [ctypes.byref(ho)],
          k.head(k.dev) + [ptr(k.dev['key'])] + tail + [ctypes.byref(do)])
    for w in host:
        assert same(dev[w], host[w]), w
    assert host['samples'].std(axis=-1).all()


@pytest.mark.parametrize('keyed', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_score_actuals_dev(env, name, keyed):
    k = Call(env, name, keyed)
    c = k.c
    Q = len(LEVELS)
    yhat = k.fc.predict(c.spec, c.theta, c.y_scale, c.grid, c.fut, floor=c.floor, cap=c.cap, extra_future=c.extra)
    y = yhat * (1.0 + 0.1 * np.random.default_rng(4).normal(size=yhat.shape))
    y[0, 5:9] = np.nan                                                      # not observed
    host = {w: np.zeros((c.N, c.H)) for w in ('yhat', 'pit', 'crps')}
    host.update({w: np.zeros((c.N, Q, c.H)) for w in ('q', 'pinball')})
    host.update(n_obs=np.zeros(c.N, np.int32), mean_crps=np.zeros(c.N), mean_pinball=np.zeros((c.N, Q)),
                coverage=np.zeros((c.N, Q)))
    dev = {w: k.out_dev(a) for w, a in host.items()}
    ho = k.lib.TsfScoreOut(**{w: ptr(a) for w, a in host.items()})
    do = k.lib.TsfScoreOut(**{w: ptr(a) for w, a in dev.items()})
    d_y = k.to_dev(y)
    tail = [Q, LEVELS.ctypes.data]
    k.run('tsf_score_actuals', k.head(k.host) + [ptr(k.host['key']), N_SAMPLES, SEED, ptr(y)] + tail + [ctypes.byref(ho)],
          k.head(k.dev) + [ptr(k.dev['key']), N_SAMPLES, SEED, ptr(d_y)] + tail + [ctypes.byref(do)])
    for w in host:
        assert same(dev[w], host[w]), w
    assert same(dev['yhat'], yhat) and host['n_obs'].tolist() == [c.H - 4] + [c.H] * (c.N - 1)
