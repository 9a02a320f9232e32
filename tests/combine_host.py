"""TEST INFRASTRUCTURE: what the reader-operator tests share -- the golden (tests/golden/c38_reader_ops.npz, written by
tools/gen_golden_reader_ops.py from the reference), this project's readers over the golden's fields with the table of expressions
the generator evaluated, and ctypes access to the evaluator of opendrift_amd/csrc/odr_combine.hip.h compiled for the host
(combine_host.cpp)."""
import ctypes as C
import os
from datetime import datetime, timedelta

import numpy as np

from host_build import host_lib
from opendrift_amd import _abi, readers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c38_reader_ops.npz')
T0 = datetime(2020, 1, 1)
WIND = ['x_wind', 'y_wind']
CURRENT = ['x_sea_water_velocity', 'y_sea_water_velocity']
_dp, _bp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_float)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def golden_readers(g):
    """a, b, c, d, [ts0, ts1]: the generator's reference_readers() as this project's readers."""
    times = [T0 + timedelta(seconds=float(s)) for s in g['seconds']]
    a = readers.GridReader(g['a_x'], g['a_y'], times, {v: g['a_' + v] for v in WIND + CURRENT}, name='a')
    b = readers.GridReader(g['b_x'], g['b_y'], times, {v: g['b_' + v] for v in WIND + CURRENT}, proj4=str(g['proj4_b']), name='b')
    d = readers.GridReader(g['d_x'], g['d_y'], times, {v: g['d_' + v] for v in CURRENT}, z=g['d_z'], name='d')
    c = readers.ConstantReader(dict(zip([str(n) for n in g['constant_names']], [float(v) for v in g['constant_values']])))
    ts = [readers.TimeseriesReader({'time': [T0 + timedelta(seconds=float(s)) for s in g['ts%d_seconds' % k]], 'lon': float(g['ts%d_lon' % k]),
                                    'lat': float(g['ts%d_lat' % k]), 'x_wind': g['ts%d_x_wind' % k], 'y_wind': g['ts%d_y_wind' % k]})
          for k in range(2)]
    return a, b, c, d, ts


def cases(g):
    """name -> (expression, variables): tools/gen_golden_reader_ops.py:cases over this project's readers."""
    a, b, c, d, ts = golden_readers(g)
    std = [float(s) for s in g['std']]
    return {
        'a+b': (a + b, WIND + CURRENT),
        '(a+b)/2': ((a + b) / 2, WIND + CURRENT),
        '(a+b)+c': ((a + b) + c, WIND + CURRENT),
        '2.5*a': (2.5 * a, WIND + CURRENT),
        '0.9*a': (0.9 * a, WIND),
        'a-3': (a - 3, WIND + CURRENT),
        'filter(a)+b': (a.filter_vars(WIND) + b, WIND),
        'c+a': (c + a, WIND + CURRENT),
        'a+d': (a + d, CURRENT),
        '0.9*d': (0.9 * d, CURRENT),
        '(a+b)+(c+a)': ((a + b) + (c + a), WIND),
        'gauss1': (a.combine_gaussian(ts[0], std[0]), WIND),
        'gauss1b': (a.combine_gaussian(ts[1], std[1]), WIND),
    }


CASE_NAMES = ['a+b', '(a+b)/2', '(a+b)+c', '2.5*a', '0.9*a', 'a-3', 'filter(a)+b', 'c+a', 'a+d', '0.9*d', '(a+b)+(c+a)', 'gauss1', 'gauss1b']


def _lib():
    return host_lib('combine_host', ('odr_combine.hip.h', 'odr_geodinv.hip.h', 'odr_geodesic.hip.h'), flags=('-O1', '-ffp-contract=off', '-w'))


def run_program(ops, values, f32, lon=None, lat=None, uniform=None):
    """The host build of comb_program over leaves given as rows of `values` ([leaf][n]) with their dtype class f32[leaf]:
    (float64 results, their class).  ops: (kind, index, (d0, d1, d2)).  ValueError with the reason for a refused program."""
    values = np.ascontiguousarray(np.atleast_2d(values), np.float64)
    n = values.shape[1]
    flat = np.ascontiguousarray([[k, i, *(tuple(d) + (0.0,) * 3)[:3]] for k, i, d in ops], np.float64)
    cls = np.ascontiguousarray(f32, np.uint8)
    uni = np.zeros(_abi.COMBINE_MAX_UNIFORM) if uniform is None else np.ascontiguousarray(list(uniform) + [0.0] * (_abi.COMBINE_MAX_UNIFORM - len(uniform)), np.float64)
    lon = np.zeros(n) if lon is None else np.ascontiguousarray(lon, np.float64)
    lat = np.zeros(n) if lat is None else np.ascontiguousarray(lat, np.float64)
    out, out_cls, why = np.empty(n), np.empty(n, np.uint8), C.create_string_buffer(128)
    rc = _lib().combh_run(len(ops), flat.ctypes.data_as(_dp), len(values), C.c_longlong(n), values.ctypes.data_as(_dp), cls.ctypes.data_as(_bp),
                          uni.ctypes.data_as(_dp), lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp), out.ctypes.data_as(_dp),
                          out_cls.ctypes.data_as(_bp), why)
    if rc:
        raise ValueError(why.value.decode())
    return out, out_cls.astype(bool)


def gauss_weight(lon, lat, lon_c, lat_c, std):
    """(weight, distance) of the host build of comb_gauss_weight / geod_inverse."""
    lon, lat = np.ascontiguousarray(lon, np.float64), np.ascontiguousarray(lat, np.float64)
    f, d = np.empty(len(lon)), np.empty(len(lon))
    _lib().combh_gauss_weight(C.c_longlong(len(lon)), lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp), C.c_double(lon_c), C.c_double(lat_c),
                              C.c_double(std), f.ctypes.data_as(_dp), d.ctypes.data_as(_dp))
    return f, d


def take(val, cur, first):
    val, cur = np.ascontiguousarray(val, np.float32), np.ascontiguousarray(cur, np.float32)
    out = np.empty(len(val), np.uint8)
    _lib().combh_take(C.c_longlong(len(val)), val.ctypes.data_as(_fp), cur.ctypes.data_as(_fp), C.c_int(int(first)), out.ctypes.data_as(_bp))
    return out.astype(bool)
