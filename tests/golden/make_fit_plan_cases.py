"""Writes tests/golden/fit_plan_cases.npz: inputs of tsf_fit_plan (include/tsf_dev.h) and the plan it returns for each,
as integer columns.  tests/test_fit_plan.py replays every record and compares every field exactly, so the fixture pins
which route a call takes -- which no GPU test can see, results being route-independent by design.

    python tests/golden/make_fit_plan_cases.py          # needs the built library; no GPU

The committed file was generated when the decision was first moved out of the fit driver, expression for expression,
before anything in it was rewritten.  Regenerate it only with a change that MEANS to move a route or a threshold, and
say so in that change.

MODELS, spec_for and the column names are shared with the test (it imports this module)."""
import functools
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from time_series_spark_amd import _lib  # noqa: E402

OUT = os.path.join(HERE, 'fit_plan_cases.npz')
DAY_NS = 86400 * 10 ** 9
MAX_T = 1048576                 # TSF_MAX_T
NEWTON_BELOW_T = 100            # TSF_NEWTON_BELOW_T
SP_MAX_ROWS = 127 * 64          # SP_MAX_NT row steps of 64 lanes
Y10, W3, D4, Y8 = (365.25, 10), (7.0, 3), (1.0, 4), (365.25, 8)
ADD, MUL = _lib.MODE_ADDITIVE, _lib.MODE_MULTIPLICATIVE

# name, growth, changepoints, history, [(period, order, mode)], extras, their mode, changepoints at given dates
MODELS = [
    ('y10_w3', 0, 25, 5, [Y10 + (ADD,), W3 + (ADD,)], 0, ADD, False),           # the bench model: KP 28
    ('w3', 0, 25, 5, [W3 + (ADD,)], 0, ADD, False),                             # KP 8
    ('w3_d4', 0, 25, 5, [W3 + (ADD,), D4 + (ADD,)], 0, ADD, False),             # KP 16
    ('y10_w3_x2', 0, 25, 5, [Y10 + (ADD,), W3 + (ADD,)], 2, ADD, False),        # harmonic, K != harm_kf
    ('y10_w3_x32', 0, 25, 5, [Y10 + (ADD,), W3 + (ADD,)], 32, ADD, False),      # + 30 indicators: KP 64, sparse candidate
    ('y8', 0, 25, 5, [Y8 + (ADD,)], 0, ADD, False),                             # no compiled expansion
    ('y10_w3_mul', 0, 25, 5, [Y10 + (MUL,), W3 + (MUL,)], 0, MUL, False),
    ('y10_w3_mixed', 0, 25, 5, [Y10 + (ADD,), W3 + (MUL,)], 0, ADD, False),
    ('y10_w3_logistic', 1, 25, 5, [Y10 + (ADD,), W3 + (ADD,)], 0, ADD, False),
    ('y10_w3_cp60', 0, 60, 5, [Y10 + (ADD,), W3 + (ADD,)], 0, ADD, False),      # two parameters per lane
    ('y10_w3_hist7', 0, 25, 7, [Y10 + (ADD,), W3 + (ADD,)], 0, ADD, False),
    ('y10_w3_cp_dates', 0, 25, 5, [Y10 + (ADD,), W3 + (ADD,)], 0, ADD, True),
    ('y10_w3_x32_logistic_mul', 1, 25, 5, [Y10 + (MUL,), W3 + (MUL,)], 32, MUL, False),   # cfg4's model
]

IN_I32 = ['model', 'algorithm', 'eval_form', 'residual_kernel', 'converge', 'coop_after', 'aligned', 'Tm', 'call', 'classes',
          'n_cu']
IN_I64 = ['N', 'n_distinct', 'lat_step', 'lat_U', 'mem_avail']
IN_COLS = IN_I32 + IN_I64                       # + 'opt': [records][len(_lib.OPTIONS)]


@functools.lru_cache(maxsize=None)
def spec_for(model, algorithm, eval_form, residual_kernel, converge, coop_after):
    _, growth, n_cp, history, seas, n_extra, extra_mode, dates = MODELS[model]
    s = _lib.default_spec()
    s.growth, s.n_changepoints, s.history = growth, n_cp, history
    s.n_seas, s.n_extra = len(seas), n_extra
    for i, (period, order, mode) in enumerate(seas):
        s.seas_period[i], s.seas_order[i], s.seas_mode[i], s.seas_prior_scale[i] = period, order, mode, 10.0
    for e in range(n_extra):
        s.extra_mode[e], s.extra_prior_scale[e] = extra_mode, 10.0
    if dates:
        s.changepoints_specified = 1
        for j in range(n_cp):
            s.changepoint_ns[j] = (j + 1) * 20 * DAY_NS
    s.algorithm, s.eval_form, s.residual_kernel, s.converge, s.coop_after = algorithm, eval_form, residual_kernel, converge, coop_after
    return s


def run_record(rec, opt):
    """(rc, plan fields) of one record: rec maps IN_COLS to integers, opt is the full option vector."""
    spec = spec_for(*(rec[k] for k in ('model', 'algorithm', 'eval_form', 'residual_kernel', 'converge', 'coop_after')))
    return _lib.fit_plan(spec, rec['N'], rec['Tm'], rec['aligned'], rec['call'], rec['classes'], rec['n_distinct'],
                         rec['lat_step'], rec['lat_U'], list(opt), rec['n_cu'], rec['mem_avail'])


# ---- the cases ---------------------------------------------------------------------------------------------------

ALGOS, FORMS, KERNELS, CONVERGE, AFTER = range(3), range(3), range(4), range(2), (-1, 0)
LENGTHS = sorted({0, 1, 2, NEWTON_BELOW_T - 1, NEWTON_BELOW_T, NEWTON_BELOW_T + 1, 130, 730, 767, 768, 769, 1023, 1024, 1025,
                  4095, 4096, 4097, SP_MAX_ROWS - 1, SP_MAX_ROWS, SP_MAX_ROWS + 1, MAX_T - 1, MAX_T, MAX_T + 1})
BIG_N = 3000000                 # 730 rows on 28 columns: 516 GB of design tables, past the 256 MB and the 32 GB rules
COUNTS = (1, 3, 1000, 100000, BIG_N)
# (option, value): every switch the plan reads at each documented value, one at a time; () = all defaults
OPTION_SETS = [(), ('harm', 0), ('harm', 1), ('harm', 2), ('lattice', 0), ('lattice', 1), ('sparse_extra', 0), ('sparse_extra', 2),
               ('fit_grouped', 0), ('gram_share', 0), ('quad_raw_y', 0)]
MEMS = (-1, 1 << 40, 1 << 28)   # unknown, ample, two fifths of it below any table the memory rule looks at


def panel(kind, N, nd=None):
    """aligned / a grid per series / shared calendars / lattice / lattice with shared calendars"""
    p = dict(aligned=0, classes=0, n_distinct=0, lat_step=0, lat_U=0)
    if kind == 'aligned':
        p['aligned'] = 1
    if kind in ('shared', 'lattice_shared'):
        p['classes'], p['n_distinct'] = 1, (max(N // 4, 1) if nd is None else nd)
    if kind in ('lattice', 'lattice_shared'):
        p['lat_step'], p['lat_U'] = DAY_NS, 1100
    return p


PANELS = ('aligned', 'series', 'shared', 'lattice', 'lattice_shared')


def cases():
    base = dict(algorithm=0, eval_form=0, residual_kernel=0, converge=0, coop_after=-1, call=0, n_cu=256, mem_avail=-1, N=1000,
                Tm=730)
    models = range(len(MODELS))

    def rec(opt=(), **kw):
        r = dict(base)
        r.update(panel(kw.pop('panel', 'aligned'), kw.get('N', base['N']), kw.pop('nd', None)))
        r.update(kw)
        return r, opt

    # every spec switch against every other, fits
    for m, al, ef, rk, cv, ca in itertools.product(models, ALGOS, FORMS, KERNELS, CONVERGE, AFTER):
        for pn, T in itertools.product(('aligned', 'series', 'shared', 'lattice'), (40, 730)):
            yield rec(model=m, algorithm=al, eval_form=ef, residual_kernel=rk, converge=cv, coop_after=ca, panel=pn, Tm=T)
    # the two evaluation calls
    for m, al, ef, rk, cv, call in itertools.product(models, (0, 2), FORMS, KERNELS, CONVERGE, (1, 2)):
        for pn, T in itertools.product(('aligned', 'series'), (40, 730)):
            yield rec(model=m, algorithm=al, eval_form=ef, residual_kernel=rk, converge=cv, call=call, panel=pn, Tm=T)
    # lengths: every threshold and one either side
    for m, T, al, rk, ef, pn in itertools.product(models, LENGTHS, ALGOS, (0, 2, 3), (0, 1), ('aligned', 'series', 'lattice')):
        yield rec(model=m, Tm=T, algorithm=al, residual_kernel=rk, eval_form=ef, panel=pn)
    # series counts, device size, memory
    for m, N, pn, T, ef, cu, mem in itertools.product(models, COUNTS, PANELS, (40, 730, 1500), (0, 1), (256, 8), MEMS):
        yield rec(model=m, N=N, panel=pn, Tm=T, eval_form=ef, n_cu=cu, mem_avail=mem)
    # shared calendars either side of 2 * n_distinct <= N and of the 64 MB table rule (730 rows: 12 steps of 64 lanes
    # on 64 / 28 / 16 / 8 columns hold 170.7 / 390.1 / 682.7 / 1365.3 grids in 64 MB)
    for m, pn, ef in itertools.product(models, ('shared', 'lattice_shared'), (0, 1)):
        for N, nd in [(3000, 1500), (3000, 1501), (3000, 2999), (3000, 3000), (3, 1), (3, 2)] + \
                [(100000, v) for v in (170, 171, 390, 391, 682, 683, 1365, 1366, 50000, 50001)]:
            yield rec(model=m, panel=pn, eval_form=ef, N=N, nd=nd)
    # the context's route switches, one at a time
    for m, o, pn, T, ef, cv in itertools.product(models, OPTION_SETS, PANELS, (40, 730, 1500), (0, 1), CONVERGE):
        yield rec(opt=o, model=m, panel=pn, Tm=T, eval_form=ef, converge=cv)
    for m, o, call in itertools.product(models, OPTION_SETS, (1, 2)):
        yield rec(opt=o, model=m, call=call)


def main():
    n_opt = len(_lib.OPTIONS)
    rows = set()
    for r, o in cases():
        opt = [-1] * n_opt
        if o:
            opt[_lib.OPTIONS.index(o[0])] = o[1]
        rows.add(tuple(r[k] for k in IN_COLS) + tuple(opt))
    rows = sorted(rows)
    out = {k: [] for k in ['rc'] + _lib.PLAN_FIELDS}
    for row in rows:
        rc, plan = run_record(dict(zip(IN_COLS, row)), row[len(IN_COLS):])
        out['rc'].append(rc)
        for f in _lib.PLAN_FIELDS:
            out[f].append(plan[f])
    arr = np.array(rows, dtype=np.int64)
    cols = {'in_' + k: arr[:, i].astype(np.int32 if k in IN_I32 else np.int64) for i, k in enumerate(IN_COLS)}
    cols['in_opt'] = arr[:, len(IN_COLS):].astype(np.int32)
    for k, v in out.items():
        cols['out_' + k] = np.array(v, dtype=np.int64 if k in ('n_grids', 'lat_U', 'quad_pre') else np.int32)
    np.savez_compressed(OUT, **cols)
    print('%d records -> %s (%d bytes)' % (len(rows), OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
