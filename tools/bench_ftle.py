#!/usr/bin/env python
"""FTLE maps on one MI355X: odr_ftle_map and the whole OpenDriftSimulation.calculate_ftle at 4000 x 2000 cells of the double gyre
(the reference's example_double_gyre_LCS.py stops at 100 x 50), against the reference's loop restated with NumPy on the same
machine on a grid small enough to finish.

    python tools/bench_ftle.py [--nx NX] [--ny NY] [--repeats R] [--numpy-nx NX] [--numpy-ny NY] [--skip-model] [--skip-numpy]

One JSON line each:
  map     `kernel_ms` the device time of the two launches (events around them), `call_ms` the whole synchronous call from host
          arrays (upload of lon / lat, launches, download of the float32 map), `call_device_inputs_ms` the same with lon / lat
          already on the device; medians of R calls after a warm-up call.  Traffic of the launches: 8 B read and 16 B written per
          element, then 16 B read (each displacement once, its neighbours from the cache) and 4 B written per cell.
  numpy   `numpy_s` the reference's physics_methods.ftle -- np.gradient, then a Python double loop with np.dot and
          np.linalg.eigvals per cell -- on --numpy-nx x --numpy-ny cells of the same field, and what that is per cell.
  model   `wall_s` of calculate_ftle with the example's parameters (runge-kutta4, time_step 0.5 s, duration 15 s) on NX x NY cells,
          both runs, their seeding and both maps included; `runs_s` the part spent in the two clones (seeding, run(), release);
          `device_GB_at_end_of_run` the device memory in use when a run has finished and nothing is released yet (hipMemGetInfo,
          whole device, minus what was in use before the first clone).
"""
import argparse
import json
import os
import sys
import time
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_loop(X, Y, delta, duration):
    """physics_methods.ftle (models/physics_methods.py:458-484), restated"""
    nx, ny = X.shape
    J = np.empty([nx, ny, 2, 2], np.float32)
    FTLE = np.empty([nx, ny], np.float32)
    dx, dy = np.gradient(X), np.gradient(Y)
    J[:, :, 0, 0] = dx[0] / (2 * delta)
    J[:, :, 1, 0] = dy[0] / (2 * delta)
    J[:, :, 0, 1] = dx[1] / (2 * delta)
    J[:, :, 1, 1] = dy[1] / (2 * delta)
    for i in range(nx):
        for j in range(ny):
            D = np.dot(np.transpose(J[i, j]), J[i, j])
            lamda = np.linalg.eigvals(D)
            FTLE[i, j] = np.log(np.sqrt(max(lamda))) / np.abs(duration)
    return FTLE


def moved_grid(proj, nx, ny, delta):
    """float32 lon / lat [ny, nx] of the grid moved by a smooth folded map of the gyre's box, and its axes"""
    xs, ys = np.arange(nx) * delta, np.arange(ny) * delta
    X, Y = np.meshgrid(xs, ys)
    bx = X + 0.3 * np.sin(np.pi * X) * np.cos(np.pi * Y) + 0.05 * np.sin(7 * X + 3 * Y)
    by = Y - 0.3 * np.cos(np.pi * X) * np.sin(np.pi * Y) + 0.05 * np.cos(5 * X - 4 * Y)
    lon, lat = proj(bx, by, inverse=True)
    return xs, ys, np.ascontiguousarray(lon, np.float32), np.ascontiguousarray(lat, np.float32)


def hip_mem_info():
    """() -> (free, total) bytes of the current device from the HIP runtime the library has loaded; None when it cannot be asked"""
    import ctypes as C
    try:      # the very file the process has mapped
        path = next(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line)
        hip = C.CDLL(path)
    except (OSError, StopIteration):
        return None

    def ask():
        free, total = C.c_size_t(), C.c_size_t()
        return (free.value, total.value) if hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 else (0, 0)
    return ask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=4000)
    ap.add_argument('--ny', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--numpy-nx', type=int, default=200)
    ap.add_argument('--numpy-ny', type=int, default=100)
    ap.add_argument('--skip-model', action='store_true')
    ap.add_argument('--skip-numpy', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.device import Context
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.readers import DoubleGyreReader
    reader = DoubleGyreReader(epsilon=.25, omega=0.628, A=.1)
    delta, T = 2.0 / a.nx, 15.0
    ctx = Context(device=0, seed=0)
    mem_info = hip_mem_info()
    xs, ys, lon, lat = moved_grid(reader.proj, a.nx, a.ny, delta)
    n = a.nx * a.ny
    P = ctx.particles(n)      # its float32 environment slots hold the device copies of lon / lat
    P.append(np.zeros(n), np.zeros(n))
    P.env_upload(0, lon.ravel())
    P.env_upload(1, lat.ravel())
    ctx.sync()
    ptr = [P.device_ptr('env:0'), P.device_ptr('env:1')]

    def timed(lo, la):
        kernel, call = [], []
        for r in range(a.repeats + 1):      # the first call warms up
            t0 = time.perf_counter()
            out = ctx.ftle_map(reader.proj.params, xs, ys, delta, T, lo, la)
            call.append(1e3 * (time.perf_counter() - t0))
            kernel.append(ctx.ftle_last_kernel_ms())
        return out, round(float(np.median(kernel[1:])), 4), round(float(np.median(call[1:])), 2)

    res = dict(what='map', nx=a.nx, ny=a.ny)
    out, res['kernel_ms'], res['call_ms'] = timed(lon, lat)
    out2, res['kernel_device_inputs_ms'], res['call_device_inputs_ms'] = timed(*ptr)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    res['kernel_cells_per_s'] = round(n / (1e-3 * res['kernel_ms']), 0)
    res['kernel_GB_per_s'] = round(44.0 * n / (1e-3 * res['kernel_ms']) / 1e9, 1)      # 24 B + 20 B per cell, see above
    res['finite_cells'] = int(np.isfinite(out).sum())
    print(json.dumps(res), flush=True)
    P.close()
    if not a.skip_numpy:
        sx, sy = max(1, a.nx // a.numpy_nx), max(1, a.ny // a.numpy_ny)
        X, Y = np.meshgrid(xs[::sx][:a.numpy_nx], ys[::sy][:a.numpy_ny])
        bx, by = reader.proj(lon[::sy, ::sx][:a.numpy_ny, :a.numpy_nx].astype(np.float64), lat[::sy, ::sx][:a.numpy_ny, :a.numpy_nx].astype(np.float64))
        t0 = time.perf_counter()
        with np.errstate(divide='ignore', invalid='ignore'):
            ref = reference_loop(bx - X, by - Y, delta * sx, T)
        s = time.perf_counter() - t0
        print(json.dumps(dict(what='numpy', nx=X.shape[1], ny=X.shape[0], numpy_s=round(s, 3), numpy_us_per_cell=round(1e6 * s / ref.size, 2),
                              extrapolated_to_full_grid_s=round(s / ref.size * n, 1),
                              full_grid_over_call=round(s / ref.size * n / (1e-3 * res['call_ms']), 0))), flush=True)
    ctx.close()
    if not a.skip_model:
        o = OceanDrift(loglevel=50)
        o.set_config('environment:fallback:land_binary_mask', 0)
        o.set_config('drift:advection_scheme', 'runge-kutta4')
        o.add_reader(reader)
        runs, in_use = [], []
        inner, inner_clone = o._ftle_trajectories, o.clone
        base = (lambda m: m[1] - m[0])(mem_info()) if mem_info else 0

        def clone():
            c = inner_clone()
            release = c._release_device

            def measured_release():
                if mem_info:
                    free, total = mem_info()
                    in_use.append(round((total - free - base) / 1e9, 2))
                release()
            c._release_device = measured_release
            return c
        o.clone = clone

        def trajectories(*args):
            t0 = time.perf_counter()
            out = inner(*args)
            runs.append(time.perf_counter() - t0)
            return out
        o._ftle_trajectories = trajectories
        t0 = time.perf_counter()
        lcs = o.calculate_ftle(time=reader.initial_time + timedelta(seconds=3), time_step=timedelta(seconds=.5),
                               duration=timedelta(seconds=T), delta=delta)
        wall = time.perf_counter() - t0
        print(json.dumps(dict(what='model', nx=lcs['lon'].shape[1], ny=lcs['lon'].shape[0], wall_s=round(wall, 2),
                              runs_s=[round(r, 2) for r in runs], device_GB_at_end_of_run=in_use, masked=[int(np.ma.getmaskarray(lcs[k]).sum()) for k in ('RLCS', 'ALCS')],
                              rlcs_range=[float(lcs['RLCS'].min()), float(lcs['RLCS'].max())])), flush=True)


if __name__ == '__main__':
    main()
