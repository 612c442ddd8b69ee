"""The model-input reader and the packer's statistics, restated in plain Python from their contract in include/tsf.h
("model-input reader", "host-side panel packing") -- not from the C++.  Timestamps are Python ints, so nothing here can
wrap; files are bytes, so any input can be classified.  tests/test_host_sanitize.py compares the native reader and packer
with this, bit for bit.

    read_ref(files, layout, series_id)   -> dict(rc, err_file, err_line, malformed, sid, did, ds, y)
    pack_ref(sid, did, ds, y)            -> dict(identity, ksid, kdid, off, ds, y, span, min_dt, y_max, flags)
"""
import re
import zlib

import numpy as np

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
TS_MIN, TS_MAX = INT64_MIN + 1, INT64_MAX       # 1677-09-21T00:12:43.145224193 .. 2262-04-11T23:47:16.854775807 (INT64_MIN = NaT)
E_OPEN, E_PARSE = -10, -11
DAY_NS = 86400 * 10 ** 9

BLANK, BAD = 'blank', 'bad'


# ---- files ---------------------------------------------------------------------------------------------------------

def inflate_all(raw):
    """Concatenated gzip / zlib members as one file; None = corrupt or truncated."""
    out = []
    while True:
        d = zlib.decompressobj(47)
        try:
            out.append(d.decompress(raw))
        except zlib.error:
            return None
        if not d.eof:
            return None
        raw = d.unused_data
        if not raw:
            return b''.join(out)


def file_bytes(raw, name=''):
    """What the reader parses for a file holding `raw`: gzip by its magic under any name, zlib only as `.deflate`."""
    if len(raw) >= 2 and raw[:2] == b'\x1f\x8b':
        return inflate_all(raw)
    if len(raw) >= 2 and name.endswith('.deflate') and raw[0] == 0x78 and ((raw[0] << 8) | raw[1]) % 31 == 0:
        return inflate_all(raw)
    return raw


# ---- fields --------------------------------------------------------------------------------------------------------

def trim(f):
    f = f.lstrip(b' \t').rstrip(b' \t\r')
    if len(f) >= 2 and f[:1] == b'"' and f[-1:] == b'"':
        f = f[1:-1]
    return f


_INT = re.compile(rb'[+-]?[0-9]{1,18}')
_TS = re.compile(rb'([0-9]{4})-([0-9]{2})-([0-9]{2})(?:[ T]([0-9]{2}):([0-9]{2})(?::([0-9]{2})(?:\.([0-9]+))?)?Z?)?')
_DEC = re.compile(rb'[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?')
_HEX = re.compile(rb'[+-]?0[xX](?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)(?:[pP][+-]?[0-9]+)?')
_NAN = re.compile(rb'[+-]?[nN][aA][nN](?:\([0-9A-Za-z_]*\))?')
_MDAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def parse_int(f):
    f = trim(f)
    return int(f) if _INT.fullmatch(f) else None


def _leap(y):
    return (y % 4 == 0 and y % 100 != 0) or y % 400 == 0


def days_from_epoch(y, m, d):
    """Days from 1970-01-01 of a proleptic Gregorian date, y >= 1, counted year by year."""
    y1 = y - 1
    before = y1 * 365 + y1 // 4 - y1 // 100 + y1 // 400                      # days before Jan 1 of year y, from 0001-01-01
    before += sum(_MDAYS[:m - 1]) + (1 if m > 2 and _leap(y) else 0) + (d - 1)
    return before - 719162                                                  # 1970-01-01 is day 719 162 after 0001-01-01


def parse_timestamp(f):
    m = _TS.fullmatch(trim(f))
    if not m:
        return None
    Y, M, D = int(m.group(1)), int(m.group(2)), int(m.group(3))
    h, mi, s = (int(m.group(k)) if m.group(k) else 0 for k in (4, 5, 6))
    frac = int((m.group(7) or b'0')[:9].ljust(9, b'0'))                       # digits after the ninth are dropped
    if not (1 <= M <= 12 and 1 <= D <= _MDAYS[M - 1] + (1 if M == 2 and _leap(Y) else 0)):
        return None
    if h > 23 or mi > 59 or s > 59:
        return None
    if Y < 1:
        return None                                                         # (year 0000: far outside int64 ns anyway)
    v = days_from_epoch(Y, M, D) * DAY_NS + ((h * 60 + mi) * 60 + s) * 10 ** 9 + frac
    return v if TS_MIN <= v <= TS_MAX else None


def parse_quantity(f):
    f = trim(f)
    if not f:
        return float('nan')                                                 # null
    iv = parse_int(f)
    if iv is not None:
        return float(iv)
    # C strtod, the whole field: white space first, then a decimal or hexadecimal literal or "nan"
    g = f.lstrip(b' \t\n\v\f\r')
    try:
        if _DEC.fullmatch(g):
            v = float(g.decode('ascii'))
        elif _HEX.fullmatch(g):
            v = float.fromhex(g.decode('ascii'))
        elif _NAN.fullmatch(g):
            return float('nan')
        else:
            return None
    except OverflowError:
        return None
    return None if v in (float('inf'), float('-inf')) else v


_PARSE = {'s': parse_int, 'd': parse_int, 't': parse_timestamp, 'q': parse_quantity}


def parse_line(line, cols, sid_const=0):
    """One line without its '\\n': BLANK, BAD, or (sid, did, ds, y)."""
    line = line.rstrip(b'\r ')
    if not line:
        return BLANK
    vals = {'s': sid_const}
    rest = line
    for k, c in enumerate(cols):
        if k == len(cols) - 1:
            field, rest = rest, None                    # the last column takes the rest of the line
        else:
            field, sep, rest = rest.partition(b',')
            if not sep:
                return BAD                              # too few fields
        if c == 'x':
            continue
        v = _PARSE[c](field)
        if v is None:
            return BAD
        vals[c] = v
    return vals['s'], vals['d'], vals['t'], vals['q']


def classify(data, cols, sid_const=0):
    """Every line of a file's bytes, in order (an unterminated last line counts; nothing after a final '\\n')."""
    lines = data.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    return [parse_line(ln, cols, sid_const) for ln in lines]


def read_ref(files, layout, series_id=None):
    """files: the bytes the reader parses per file (file_bytes), None = corrupt stream, False = cannot be read."""
    permissive = layout.endswith('?')
    cols = layout.rstrip('?')
    out = dict(rc=0, err_file=-1, err_line=0, malformed=0)
    rows = []
    for i, data in enumerate(files):                    # every file is opened before any is parsed
        if data is None or data is False:
            return dict(rc=E_OPEN, err_file=i, err_line=-1 if data is None else 0, malformed=-1, rows=[])
    for i, data in enumerate(files):
        for ln, r in enumerate(classify(data, cols, series_id[i] if series_id is not None else 0), 1):
            if r is BLANK:
                continue
            if r is BAD:
                if not permissive:
                    return dict(rc=E_PARSE, err_file=i, err_line=ln, malformed=-1, rows=[])
                out['malformed'] += 1
                continue
            rows.append(r)
    out['rows'] = rows
    return out


def columns(rows):
    sid = np.array([r[0] for r in rows], dtype=np.int64)
    did = np.array([r[1] for r in rows], dtype=np.int64)
    ds = np.array([r[2] for r in rows], dtype=np.int64)
    y = np.array([r[3] for r in rows], dtype=np.float64)
    return sid, did, ds, y


# ---- packer --------------------------------------------------------------------------------------------------------

def _sat(v):
    return min(v, INT64_MAX)


def pack_ref(sid, did, ds, y):
    """The order contract and the per-series statistics of tsf_pack_rows / tsf_pack_fetch / tsf_pack_flags."""
    sid, did, ds = (np.asarray(a).astype(np.int64) for a in (sid, did, ds))
    y = np.asarray(y).astype(np.float64)
    keep = ~np.isnan(y)
    same = (sid[1:] == sid[:-1]) & (did[1:] == did[:-1])
    key_down = (sid[1:] < sid[:-1]) | ((sid[1:] == sid[:-1]) & (did[1:] < did[:-1]))
    identity = bool(keep.all() and not key_down.any() and not (same & (ds[1:] < ds[:-1])).any())
    idx = np.flatnonzero(keep)
    order = idx[np.lexsort((ds[idx], did[idx], sid[idx]))]                   # stable: ties stay in input order
    s, d, t, v = sid[order], did[order], ds[order], y[order]
    starts = np.flatnonzero(np.r_[True, (s[1:] != s[:-1]) | (d[1:] != d[:-1])]) if len(s) else np.zeros(0, np.int64)
    off = np.r_[starts, len(s)].astype(np.int64)
    NS = len(starts)
    span, min_dt, y_max = [], [], []
    aligned = NS > 0
    for k in range(NS):
        a, b = int(off[k]), int(off[k + 1])
        tt = [int(x) for x in t[a:b]]
        span.append(_sat(tt[-1] - tt[0]))
        gaps = [_sat(q - p) for p, q in zip(tt, tt[1:]) if q > p]
        min_dt.append(min(gaps) if gaps else -1)
        y_max.append(v[a:b][int(np.argmax(v[a:b]))])                         # the first of the largest
        aligned = aligned and np.array_equal(t[a:b], t[off[0]:off[1]])
    whole = (v >= -2147483648.0) & (v <= 2147483647.0) & (v == np.trunc(v))
    flags = np.array([aligned, bool(np.isinf(v).any()), NS > 0 and bool(whole.all()), bool((t == INT64_MIN).any())],
                     dtype=np.int32)
    return dict(identity=int(identity), ksid=s[starts] if NS else s[:0], kdid=d[starts] if NS else d[:0], off=off, ds=t, y=v,
                span=np.array(span, dtype=np.int64), min_dt=np.array(min_dt, dtype=np.int64),
                y_max=np.array(y_max, dtype=np.float64), flags=flags)
