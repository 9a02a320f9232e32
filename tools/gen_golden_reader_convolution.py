"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c41_reader_convolution.npz from the REFERENCE ITSELF.

StructuredReader.set_convolution_kernel / __convolve_block__ (readers/basereader/structured.py:163-192, applied at :278-306) of the
reference, imported through oracle/refshim.py, on the in-memory StructuredReader of oracle/gen_golden.py; SciPy does the arithmetic.

Contents:
  a  raw blocks and what the reference's __convolve_block__ makes of them, per case `name`: a_<name>_kernel (the argument of
     set_convolution_kernel: a 0-d int N, or the weights), a_<name>_vars, a_<name>_raw_<variable>, a_<name>_out_<variable>.  Box
     kernels N = 2, 3, 4, 5 and an asymmetric 3 x 5 kernel with one zero weight; 2-D and 3-D float32 variables; in every variable two
     NaN cells and a cell of 1e10 next to one of 9.99e9; grids one less than, equal to and one more than the device's tile edge
     (TILE = 32, csrc/odr_convolve.hip.h CONV_T) along y and x; ny = 2 with N = 5; nz = 2 with N = 3; a 3-D variable of one layer.
  b  get_variables_interpolated of a reader with convolve = 3: 300 positions between two time levels, 2-D and 3-D variables with NaN
     (land) cells, and the profile of sea_water_temperature.
  c  two runs of the reference's OceanDrift (euler, runge-kutta4) on a convolved current and wind: 40 elements, 12 steps of 10 minutes
     over three hourly levels.

Asserted here, so that the file cannot hide a failure: convolved and raw fields differ by more than 1e-3 of the raw field's range on
at least half of the cells; somewhere a convolved value lies beyond the 1e9 mask and somewhere a smeared fill value lies below it; a
NaN under the zero weight does not spread; the trajectories of (c) end more than 100 x the comparison bound (1e-7 deg,
tests/test_gpu_parity.py) from those of the same run without the kernel.

    python tools/gen_golden_reader_convolution.py
"""
import os
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as gg  # noqa: E402  (installs the shim)

TILE = 32
BOUND = 1e-7
U, V, W = 'x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity'
XW, YW = 'x_wind', 'y_wind'
DEPTH, LAND, TEMP = 'sea_floor_depth_below_sea_level', 'land_binary_mask', 'sea_water_temperature'
ASYM = np.array([[0.05, 0.1, 0.2, -0.05, 0.02],
                 [0.1, 0.25, 0.0, 0.07, 0.03],
                 [0.01, 0.04, 0.11, 0.06, 0.01]])      # not normalised (sum 1.0 is a coincidence the reference does not need): one zero
# name -> (kernel argument, ny, nx, {variable: layers; 0 = a 2-D array})
CASES = {
    'n2': (2, TILE - 1, TILE + 1, {XW: 0, LAND: 0, U: 3}),
    'n3': (3, TILE, TILE, {DEPTH: 0, V: 2}),
    'n4': (4, TILE + 1, TILE - 1, {XW: 0, TEMP: 1, W: 3}),
    'n5': (5, 2, 40, {YW: 0, U: 4}),
    'k35': (ASYM, TILE + 1, 2 * TILE + 1, {XW: 0, DEPTH: 0, U: 3}),
}


def reader_of(arrays, ny, nx, z=None, times=None, name='r'):
    x, y = 4.0 + 0.05 * np.arange(nx), 59.0 + 0.05 * np.arange(ny)
    return gg.GridReader('+proj=latlong', x, y, times or [gg.T0], arrays, z=z, name=name)


def spoil(a, rng):
    """Two NaN cells, a cell of 1e10 and one of 9.99e9 next to it, in the last two axes' plane of layer 0 (and of the last layer)."""
    ny, nx = a.shape[-2:]
    plane = a.reshape((-1, ny, nx))
    for k in {0, plane.shape[0] - 1}:
        cells = rng.choice(ny * nx - 1, 3, replace=False)
        plane[k].flat[cells[0]] = np.nan
        plane[k].flat[cells[1]] = np.nan
        plane[k].flat[cells[2]] = 1e10
        plane[k].flat[cells[2] + 1] = 9.99e9
    return a


def part_a():
    rng = np.random.default_rng(41)
    out = dict(a_cases=np.array(list(CASES)), tile=TILE)
    beyond = below = 0
    for name, (conv, ny, nx, variables) in CASES.items():
        raw = {}
        for v, nz in variables.items():
            shape = (ny, nx) if nz == 0 else (nz, ny, nx)
            a = (rng.integers(0, 2, shape) if v == LAND else rng.normal(size=shape) * 3 + (100 if v == DEPTH else 0)).astype(np.float32)
            raw[v] = a if v == LAND else spoil(a, rng)
        r = reader_of({v: a[None] for v, a in raw.items()}, ny, nx, z=np.array([0.0, -5.0]))
        r.set_convolution_kernel(conv)
        env = r.get_variables(list(variables), gg.T0)
        env = r.__convolve_block__(env)
        out['a_%s_kernel' % name] = np.asarray(conv)
        out['a_%s_vars' % name] = np.array(list(variables))
        for v in variables:
            c = env[v]
            assert c.dtype == np.float32 and c.shape == raw[v].shape, (name, v, c.dtype, c.shape)
            out['a_%s_raw_%s' % (name, v)], out['a_%s_out_%s' % (name, v)] = raw[v], c
            ok = np.isfinite(raw[v]) & (np.abs(raw[v]) < 1e9)
            span = raw[v][ok].max() - raw[v][ok].min()
            with np.errstate(invalid='ignore'):
                differs = np.abs(c - raw[v]) > 1e-3 * span
                beyond += int((np.abs(c) > 1e9).sum())
                below += int(((np.abs(c) > 1e6) & (np.abs(c) <= 1e9)).sum())
            print(name, v, c.shape, 'cells that differ: %d of %d' % (differs[ok].sum(), ok.sum()), 'NaN', int(np.isnan(c).sum()))
            assert differs[ok].sum() >= 0.5 * ok.sum(), (name, v)
            assert np.isnan(c).sum() > np.isnan(raw[v]).sum() or v == LAND      # a NaN spreads over its footprint
    assert beyond > 0 and below > 0, (beyond, below)
    # a NaN under the zero weight stays where it is
    a = np.ones((9, 9), np.float32)
    a[4, 4] = np.nan
    r = reader_of({XW: a[None]}, 9, 9)
    r.set_convolution_kernel(ASYM)
    c = r.__convolve_block__(r.get_variables([XW], gg.T0))[XW]
    assert np.isnan(c).sum() == ASYM.size - 1, np.isnan(c).sum()
    out['a_zero_raw'], out['a_zero_out'] = a, c
    return out


def filled32(a):
    return np.ma.filled(np.ma.masked_invalid(np.ma.asarray(a).astype(np.float64)), np.nan).astype(np.float32)


def part_b():
    rng = np.random.default_rng(412)
    ny, nx, nz, n = 24, 26, 4, 300
    z = np.array([0.0, -10.0, -20.0, -40.0])
    seconds = np.array([0.0, 3600.0])
    times = [gg.T0 + timedelta(seconds=float(s)) for s in seconds]
    arrays = {U: rng.normal(size=(2, nz, ny, nx)), V: rng.normal(size=(2, nz, ny, nx)), TEMP: 8 + rng.normal(size=(2, nz, ny, nx)),
              XW: 5 * rng.normal(size=(2, ny, nx)), YW: 5 * rng.normal(size=(2, ny, nx))}
    arrays = {v: a.astype(np.float32) for v, a in arrays.items()}
    for v in (U, V):      # land: no current
        arrays[v][:, :, 10:13, 20:22] = np.nan
        arrays[v][:, :, 18, 5] = np.nan
    r = reader_of(arrays, ny, nx, z=z, times=times, name='conv_b')
    r.set_convolution_kernel(3)
    lon, lat = rng.uniform(r.x[3], r.x[-4], n), rng.uniform(r.y[3], r.y[-4], n)
    zq = -np.round(rng.uniform(0, 35, n) * 4) / 4
    zq[:20] = 0.0
    call = 1500.0
    variables = [U, V, TEMP, XW, YW]
    env, prof = r.get_variables_interpolated(variables, profiles=[TEMP], profiles_depth=30.0, time=gg.T0 + timedelta(seconds=call),
                                             lon=lon, lat=lat, z=zq)
    out = dict(b_x=r.x, b_y=r.y, b_z=z, b_seconds=seconds, b_call_seconds=call, b_lon=lon, b_lat=lat, b_zq=zq, b_vars=np.array(variables))
    for v in variables:
        out['b_field_' + v] = arrays[v]
        out['b_env_' + v] = filled32(env[v])
        print('b', v, 'finite', int(np.isfinite(out['b_env_' + v]).sum()), 'of', n)
        assert np.isfinite(out['b_env_' + v]).all()
    out['b_profile_z'] = np.asarray(prof['z'], np.float64)
    out['b_profile_' + TEMP] = filled32(prof[TEMP])
    print('b profile', out['b_profile_' + TEMP].shape, out['b_profile_z'])
    plain = reader_of(arrays, ny, nx, z=z, times=times, name='plain_b')
    env0, _ = plain.get_variables_interpolated(variables, time=gg.T0 + timedelta(seconds=call), lon=lon, lat=lat, z=zq)
    for v in variables:
        assert (np.abs(filled32(env0[v]) - out['b_env_' + v]) > 1e-3).sum() > n // 2, v
    return out


def part_c():
    rng = np.random.default_rng(413)
    ny, nx, n, steps, dt = 30, 34, 40, 12, 600.0
    seconds = np.array([0.0, 3600.0, 7200.0])
    times = [gg.T0 + timedelta(seconds=float(s)) for s in seconds]
    cur = {v: (0.6 * rng.normal(size=(3, ny, nx))).astype(np.float32) for v in (U, V)}
    wind = {v: (8 * rng.normal(size=(3, ny, nx))).astype(np.float32) for v in (XW, YW)}
    x, y = 4.0 + 0.05 * np.arange(nx), 59.0 + 0.05 * np.arange(ny)
    lon, lat = rng.uniform(x[8], x[-9], n), rng.uniform(y[8], y[-9], n)
    lon, lat = np.float32(lon).astype(np.float64), np.float32(lat).astype(np.float64)      # (the elements hold float32 at the start)
    out = dict(c_x=x, c_y=y, c_seconds=seconds, c_dt=dt, c_steps=steps, c_wdf=0.03, c_lon=lon, c_lat=lat, c_kernel=3)
    out.update({'c_field_' + v: a for v, a in {**cur, **wind}.items()})
    for scheme, tag in (('euler', 'euler'), ('runge-kutta4', 'rk4')):
        ends = []
        for conv in (3, None):
            rc = reader_of(cur, ny, nx, times=times, name='current')
            rw = reader_of(wind, ny, nx, times=times, name='wind')
            rc.set_convolution_kernel(conv)
            rw.set_convolution_kernel(conv)
            o = gg._base(scheme)
            o.add_reader([rc, rw])
            o.set_config('environment:constant:land_binary_mask', 0)
            o.set_config('drift:stokes_drift', False)
            np.random.seed(0)
            o.seed_elements(lon=lon, lat=lat, time=gg.T0, wind_drift_factor=0.03)
            res, _ = gg._run(o, dt, steps)
            assert not o.env.discarded_readers and (res['status'] == 0).all()
            ends.append(res)
            if conv is not None:
                out.update({'c_%s_%s' % (tag, k): a for k, a in res.items()})
        apart = np.hypot(ends[0]['lon'][-1] - ends[1]['lon'][-1], ends[0]['lat'][-1] - ends[1]['lat'][-1])
        print(scheme, 'convolved and plain runs end %.2e .. %.2e deg apart' % (apart.min(), apart.max()))
        assert apart.min() > 100 * BOUND, apart.min()
    return out


def main():
    out = {}
    out.update(part_a())
    out.update(part_b())
    out.update(part_c())
    path = os.path.join(gg.GOLD, 'c41_reader_convolution.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 400 << 10


if __name__ == '__main__':
    main()
