"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c38_reader_ops.npz from the REFERENCE ITSELF.

The reference's own operator classes (opendrift/readers/operators/: ops.py, numops.py, readerops.py, filter.py), imported through
oracle/refshim.py, answer every query recorded here; the leaves are the reference's reader_constant, reader_timeseries and the
in-memory StructuredReader of oracle/gen_golden.py.

WHAT THE REFERENCE DOES (asserted below, so that the golden cannot drift from these findings):
  * grammar: T + T is readerops.Combined, a BaseReader (it nests); number o T is numops.Combined, no BaseReader and without
    operators; r1 - r2, r1 + 2 * r2, 2 * (3 * r1) and (2 * r1) + 1 are TypeErrors; a variable outside the intersection is an
    AssertionError;
  * readerops.Combined.get_variables_interpolated calls its operands WITHOUT rotate_to_proj, so the vector pairs of a projected
    (polar-stereographic) operand are NOT rotated to east / north: the sum holds the components along the grid's own axes, and a
    2-D block level stays float32 (asserted: the operand's un-rotated values give the sum bit for bit, the rotated ones do not);
  * dtype: 2-D block levels give float32, between two time levels too -- when the reader covers EVERY position of the call; a
    reader that misses one position hands its values out in a masked float64 array (np.ma.masked_all, variables.py:840-858); a
    3-D variable, a constant and a timeseries reader give float64.  float32 + float32 is a float32 sum.  number o float32 is a
    FLOAT64 operation: the operand is a np.ma.MaskedArray, whose arithmetic turns the python number into a 0-d float64 array
    before NumPy's promotion sees it (asserted: 0.9 * a is the float32 cast of the float64 product, not the float32 product);
  * combine_gaussian stops at `assert isinstance(np.broadcast_arrays(lon, lat), list)` under a NumPy whose broadcast_arrays returns a
    tuple; this process gives np.broadcast_arrays a wrapper that returns a list, and nothing else is changed.  With that the blend
    with ONE measurement reader runs.  The blend with a LIST of measurement readers hands Geod.inv arrays of shape (N, n), which the
    stand-in for pyproj behind oracle/refshim.py returns flattened; making that path run would take more than the one line, so the
    list form is not recorded here and readers.CombinedReader refuses it.

Contents:
  1  direct get_variables_interpolated results of thirteen expressions over: `a` a latlong grid of 6 x 5 nodes with NaN (land) cells in
     its current; `b` a polar-stereographic grid that covers part of the positions; `d` a latlong grid whose current has three z
     levels; `c` a constant reader; two timeseries readers with a position.  Two time levels, the call between them.
     Two sets of 321 positions: inside every grid, and over a box that a and b cover in part.  The Gaussian blend with one
     measurement reader, at two centres.
  2  two runs of the reference's OceanDrift with the priority list [combined, wind, current] of the gallery example
     example_reader_operators.py: Euler with constant + gridded wind, runge-kutta4 with tide + background currents; 40 elements,
     10 steps of 10 minutes over three hourly levels.
  3  the rejected expressions and the AssertionError, as a list of names.

    python tools/gen_golden_reader_ops.py
"""
import os
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as gg  # noqa: E402  (installs the shim)
import pyproj  # noqa: E402  (the shim's)
from opendrift.readers import reader_constant, reader_timeseries  # noqa: E402
from opendrift.readers.basereader import BaseReader  # noqa: E402
from opendrift_amd import synthetic as synth  # noqa: E402

_broadcast_arrays = np.broadcast_arrays
np.broadcast_arrays = lambda *a, **k: list(_broadcast_arrays(*a, **k))      # the one version-dependent line of ops.py

WIND = ['x_wind', 'y_wind']
CURRENT = ['x_sea_water_velocity', 'y_sea_water_velocity']
NQ = 321
CALL_SECONDS = 1200      # between the first two levels
CONSTANT = {'x_wind': 10.0, 'y_wind': 0.5, 'x_sea_water_velocity': 0.1, 'y_sea_water_velocity': -0.05}
TS = [dict(lon=4.5, lat=60.0, seconds=[0, 1800, 3600], x_wind=[3.0, 4.0, 5.0], y_wind=[-1.0, -2.0, -3.0]),
      dict(lon=4.8, lat=60.2, seconds=[0, 1800, 3600], x_wind=[-6.0, -7.0, -8.0], y_wind=[2.5, 3.5, 4.5])]
STD = [12000.0, 7000.0]


def fields():
    """The grids and their arrays: small integers / 64, exact in float32."""
    rng = np.random.default_rng(38)

    def arr(*shape):
        return (rng.integers(-64, 65, shape) / 64.0).astype(np.float32)
    f = dict(seconds=np.array([0.0, 3600.0, 7200.0]))
    f['a_x'], f['a_y'] = 4.0 + 0.2 * np.arange(6), 59.6 + 0.2 * np.arange(5)
    for v in WIND + CURRENT:
        f['a_' + v] = arr(3, 5, 6)
    for v in CURRENT:      # land: no current
        f['a_' + v][:, 1, 1] = np.nan
        f['a_' + v][:, 3, 4] = np.nan
    xc, yc = pyproj.Proj(synth.NORKYST_PROJ4)(4.7, 60.1)
    f['b_x'], f['b_y'] = np.round(xc) + 8000.0 * np.arange(-3, 3), np.round(yc) + 8000.0 * np.arange(-2, 3)
    for v in WIND + CURRENT:
        f['b_' + v] = arr(3, 5, 6)
    f['d_x'], f['d_y'], f['d_z'] = 3.8 + 0.3 * np.arange(6), 59.4 + 0.3 * np.arange(5), np.array([0.0, -10.0, -20.0])
    for v in CURRENT:
        f['d_' + v] = arr(3, 3, 5, 6)
    return f


def reference_readers(f):
    times = [gg.T0 + timedelta(seconds=float(s)) for s in f['seconds']]
    a = gg.GridReader('+proj=latlong', f['a_x'], f['a_y'], times, {v: f['a_' + v] for v in WIND + CURRENT}, name='a')
    b = gg.GridReader(synth.NORKYST_PROJ4, f['b_x'], f['b_y'], times, {v: f['b_' + v] for v in WIND + CURRENT}, name='b')
    d = gg.GridReader('+proj=latlong', f['d_x'], f['d_y'], times, {v: f['d_' + v] for v in CURRENT}, z=f['d_z'], name='d')
    c = reader_constant.Reader(dict(CONSTANT))
    ts = [reader_timeseries.Reader({'time': [gg.T0 + timedelta(seconds=s) for s in m['seconds']], 'lon': m['lon'], 'lat': m['lat'],
                                    'x_wind': list(m['x_wind']), 'y_wind': list(m['y_wind'])}) for m in TS]
    return a, b, c, d, ts


def cases(a, b, c, d, ts):
    """name -> (expression, variables).  The same table, over this project's readers, is tests/combine_host.py:cases."""
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
        'gauss1': (a.combine_gaussian(ts[0], STD[0]), WIND),
        'gauss1b': (a.combine_gaussian(ts[1], STD[1]), WIND),
    }


def filled32(a):
    """The float32 cast of environment.py:695, NaN where the array is masked or not finite."""
    return np.ma.filled(np.ma.masked_invalid(np.ma.asarray(a).astype(np.float64)), np.nan).astype(np.float32)


def part1(f):
    a, b, c, d, ts = reference_readers(f)
    rng = np.random.default_rng(381)
    t = gg.T0 + timedelta(seconds=CALL_SECONDS)
    out = dict(call_seconds=CALL_SECONDS)
    # two sets of positions: 'in' inside a, b and d (every reader covers every position: 2-D levels stay float32), and 'all' over
    # a wider box (b and a cover part of it: their arrays arrive as masked float64)
    sets = {'in': (rng.uniform(4.55, 4.85, NQ), rng.uniform(60.02, 60.18, NQ)), 'all': (rng.uniform(3.9, 5.1, NQ), rng.uniform(59.5, 60.5, NQ))}
    sets['all'][0][:4], sets['all'][1][:4] = [4.5, 4.8, 4.2, 4.0], [60.0, 60.2, 59.8, 59.6]      # the measurement points, a land node, a corner
    z = -np.round(rng.uniform(0, 18, NQ) * 4) / 4
    out['q_z'] = z
    names, dtypes = [], []
    for tag, (lon, lat) in sets.items():
        out['q_%s_lon' % tag], out['q_%s_lat' % tag] = lon, lat
        for name, (expr, variables) in cases(a, b, c, d, ts).items():
            env, prof = expr.get_variables_interpolated(variables, time=t, lon=lon, lat=lat, z=z)
            assert prof is None
            for v in variables:
                out['r_%s_%s_%s' % (tag, name, v)] = filled32(env[v])
                names.append('%s %s %s' % (tag, name, v))
                dtypes.append(str(np.ma.asarray(env[v]).dtype))
            print(tag, name, {v: str(np.ma.asarray(env[v]).dtype) for v in variables},
                  'finite', int(np.isfinite(out['r_%s_%s_%s' % (tag, name, variables[0])]).sum()), 'of', NQ)
    out['case_variable'], out['case_dtype'] = np.array(names), np.array(dtypes)
    # the findings
    dt = dict(zip(names, dtypes))
    for name in ('a+b', 'filter(a)+b'):
        assert dt['in %s x_wind' % name] == 'float32' and dt['all %s x_wind' % name] == 'float64', name
    for name, v in (('2.5*a', 'x_wind'), ('0.9*a', 'x_wind'), ('a-3', 'x_wind'), ('(a+b)/2', 'x_wind'), ('c+a', 'x_wind'), ('a+d', CURRENT[0]), ('0.9*d', CURRENT[0]), ('gauss1', 'x_wind'), ('(a+b)+c', 'x_wind')):
        assert dt['in %s %s' % (name, v)] == 'float64', name
    assert all(np.isfinite(out[k]).all() for k in out if k.startswith('r_in_'))
    # number o float32 MaskedArray is a float64 operation: not the float32 product
    lon, lat = sets['in']
    own, _ = a.get_variables_interpolated(WIND, time=t, lon=lon, lat=lat, z=z)
    assert isinstance(own['x_wind'], np.ma.MaskedArray) and own['x_wind'].dtype == np.float32
    assert np.array_equal(out['r_in_0.9*a_x_wind'], (0.9 * np.asarray(own['x_wind'], np.float64)).astype(np.float32))
    assert (out['r_in_0.9*a_x_wind'] != np.float32(0.9) * np.asarray(own['x_wind'])).sum() > 10
    # the operands are not rotated
    latlong = pyproj.Proj('+proj=latlong')
    plain, _ = b.get_variables_interpolated(WIND, time=t, lon=lon, lat=lat, z=z)
    rotated, _ = b.get_variables_interpolated(WIND, time=t, lon=lon, lat=lat, z=z, rotate_to_proj=latlong)
    assert np.array_equal(np.asarray(own['x_wind']) + np.asarray(plain['x_wind']), out['r_in_a+b_x_wind'])
    assert np.abs(filled32(np.asarray(own['x_wind']) + np.asarray(rotated['x_wind'])) - out['r_in_a+b_x_wind']).max() > 0.01
    both = np.isfinite(out['r_all_a+b_x_wind'])
    assert 0.1 * NQ < both.sum() < 0.8 * NQ, both.sum()      # b covers part of the wide box
    assert np.isfinite(out['r_all_2.5*a_x_wind']).sum() > both.sum() and not np.isfinite(out['r_all_2.5*a_x_wind']).all()
    # the distances behind the Gaussian weights
    geod = pyproj.Geod(ellps='WGS84')
    for tag, (lon, lat) in sets.items():
        for k, m in enumerate(TS):
            out['gauss_distance_%s_%d' % (tag, k)] = np.asarray(geod.inv(lon, lat, m['lon'] * np.ones(NQ), m['lat'] * np.ones(NQ))[2])
    return out


def part2(f):
    a, b, c, d, ts = reference_readers(f)
    rng = np.random.default_rng(382)
    n, steps, dt = 40, 10, 600.0
    lon, lat = rng.uniform(4.3, 4.7, n), rng.uniform(59.85, 60.15, n)
    lon, lat = np.float32(lon).astype(np.float64), np.float32(lat).astype(np.float64)      # (the elements hold float32 at the start)
    out = dict(run_dt=dt, run_steps=steps, run_wdf=0.03)
    times = [gg.T0 + timedelta(seconds=float(s)) for s in f['seconds']]

    # Euler: constant extra wind on a gridded wind, then the wind reader, then the current (example_reader_operators.py)
    onshore = reader_constant.Reader({'x_wind': 10.0, 'y_wind': 0.0})
    wind = gg.GridReader('+proj=latlong', f['d_x'], f['d_y'], times, {v: 8 * f['a_' + v] for v in WIND}, name='wind')
    current = gg.GridReader('+proj=latlong', f['d_x'], f['d_y'], times, {v: f['b_' + v] for v in CURRENT}, name='current')
    o = gg._base('euler')
    o.add_reader([onshore + wind, wind, current])
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:stokes_drift', False)
    np.random.seed(0)
    o.seed_elements(lon=lon, lat=lat, time=gg.T0, wind_drift_factor=0.03)
    res, _ = gg._run(o, dt, steps)
    assert not o.env.discarded_readers and (res['status'] == 0).all()
    plain = gg._base('euler')      # the same run without the combined reader must end elsewhere
    plain.add_reader([wind, current])
    plain.set_config('environment:constant:land_binary_mask', 0)
    plain.set_config('drift:stokes_drift', False)
    np.random.seed(0)
    plain.seed_elements(lon=lon, lat=lat, time=gg.T0, wind_drift_factor=0.03)
    res0, _ = gg._run(plain, dt, steps)
    assert np.abs(res['lon'][-1] - res0['lon'][-1]).min() > 0.01
    out.update({'run_euler_' + k: v for k, v in res.items()})

    # runge-kutta4: tide + background currents, then the background alone
    tide = gg.GridReader('+proj=latlong', f['a_x'] - 0.3, f['a_y'] - 0.1, times, {v: 0.5 * f['b_' + v] for v in CURRENT}, name='tide')
    background = gg.GridReader('+proj=latlong', f['d_x'], f['d_y'], times, {v: f['a_' + v][:, ::-1, ::-1].copy() for v in WIND + CURRENT},
                               name='background')
    o = gg._base('runge-kutta4')
    o.add_reader([tide + background, background])
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:stokes_drift', False)
    np.random.seed(0)
    o.seed_elements(lon=lon, lat=lat, time=gg.T0, wind_drift_factor=0.0)
    res, _ = gg._run(o, dt, steps)
    assert not o.env.discarded_readers and (res['status'] == 0).all()
    moved = np.hypot(res['lon'][-1] - res['lon'][0], res['lat'][-1] - res['lat'][0])
    print('rk4 run moved', moved.min(), '..', moved.max(), 'deg')
    out.update({'run_rk4_' + k: v for k, v in res.items()})
    out['run_lon'], out['run_lat'] = lon, lat
    return out


def part3(f):
    a, b, c, d, ts = reference_readers(f)
    rejected = []
    for name, make in (('r1 - r2', lambda: a - b), ('r1 + 2 * r2', lambda: a + 2 * b), ('2 * (3 * r1)', lambda: 2 * (3 * a)),
                       ('(2 * r1) + 1', lambda: (2 * a) + 1)):
        try:
            make()
        except TypeError:
            rejected.append(name)
    assert len(rejected) == 4, rejected
    assert isinstance(a + b, BaseReader) and isinstance((a + b) + a, BaseReader) and not isinstance(2 * a, BaseReader)
    r = c.exclude_vars(['x_wind']) + a
    try:
        r.get_variables_interpolated(['x_wind'], time=gg.T0, lon=np.array([4.5]), lat=np.array([60.0]), z=np.array([0.0]))
        raise SystemExit('the reference accepted a variable outside the intersection')
    except AssertionError:
        rejected.append('variable outside the intersection: AssertionError')
    filtered = set((a.filter_vars(WIND) + b).variables)      # (the reference's BaseReader adds what it can derive: wind_speed)
    assert (a + b).name == 'Combined(a | b)' and set(WIND) <= filtered and not filtered & set(CURRENT)
    return dict(rejected=np.array(rejected), name_a_plus_b=(a + b).name)


def main():
    f = fields()
    out = dict(f)
    out.update(constant_names=np.array(list(CONSTANT)), constant_values=np.array(list(CONSTANT.values())), std=np.array(STD),
               proj4_b=synth.NORKYST_PROJ4)
    for k, m in enumerate(TS):
        out.update({'ts%d_%s' % (k, key): np.asarray(val, np.float64) for key, val in m.items()})
    out.update(part1(f))
    out.update(part2(f))
    out.update(part3(f))
    path = os.path.join(gg.GOLD, 'c38_reader_ops.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 1 << 20


if __name__ == '__main__':
    main()
