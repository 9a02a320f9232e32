#!/usr/bin/env python
"""SedimentDrift.run() through the model API at C3 size on one MI355X, next to OceanDrift.run() on the same fields in the same
call (machines differ by several per cent: only same-call numbers compare).  C3 fields (1024 x 1024 x 12 lon / lat / z block:
current, vertical velocity, diffusivity, land mask) with a shallow sea floor of 4 - 34 m; 10 M elements sinking at
0.5 - 20 mm/s, RK4 + vertical mixing (60 s sub-steps) + vertical advection, device RNG.

    python tools/bench_sedimentdrift.py [--particles N] [--steps K] [--small] [--only sediment|ocean|mixing]

One JSON line:
  steady ms per step (the loop body after the first step) of both models -- OceanDrift takes run()'s fused lane and the static
  C3 launches, SedimentDrift the call-by-call lane with the run-time mixing kernel (sea-floor action ODR_SEAFLOOR_SETTLE) and
  its resuspension launch;
  the run-time mixing kernel (odr_vmix, host clock around a synchronised launch, best of five) on the same elements with the
  sea-floor action 1 (lift) and 4 (settle);
  k_resuspend's memory yardstick: about 12 B per element (u, v, moving in; z and moving only where an element is settled) at
  the 6.3 TB/s DESIGN.md quotes for a streaming kernel -- an ESTIMATE.  The kernel's own time comes from a
  `rocprofv3 --kernel-trace --stats -- python tools/bench_sedimentdrift.py --only sediment` run (k_resuspend).
"""
import argparse
import json
import os
import sys
import time
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12
RESUSPEND_KERNEL_BYTES = 12
NAMES = ['x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity', 'ocean_vertical_diffusivity',
         'sea_floor_depth_below_sea_level', 'land_binary_mask']


def fields(small):
    from opendrift_amd import synthetic as synth
    nx, ny, nz = (128, 96, 8) if small else (1024, 1024, 12)
    g = synth.grid3d(nx=nx, ny=ny, nz=nz, nt=3, seed=0)
    X, Y = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
    depth = (4 + 30 * (0.5 + 0.5 * np.sin(2 * X + 1.0) * np.cos(1.5 * Y))).astype(np.float32)
    g['sea_floor_depth_below_sea_level'] = np.broadcast_to(depth, (3, ny, nx)).copy()
    return g


def seeds(g, n):
    rng = np.random.default_rng(0)
    lon = rng.uniform(g['x'][8], g['x'][int(0.9 * len(g['x']))], n)
    lat = rng.uniform(g['y'][8], g['y'][-9], n)
    tv = -np.exp(rng.uniform(np.log(0.0005), np.log(0.02), n)).astype(np.float32)
    return lon, lat, -rng.uniform(0.5, 3.5, n), tv


def run(cls, g, n, steps):
    t0 = datetime(2020, 1, 1)
    times = [t0 + timedelta(seconds=float(t)) for t in g['t']]
    from opendrift_amd import readers
    o = cls(loglevel=50, seed=0)
    o.add_reader(readers.GridReader(g['x'], g['y'], times, {k: g[k] for k in NAMES}, z=g['z']))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('drift:vertical_mixing', True)
    o.set_config('vertical_mixing:timestep', 60)
    o.set_config('general:coastline_action', 'previous')
    lon, lat, z, tv = seeds(g, n)
    o.seed_elements(lon=lon, lat=lat, z=z, time=t0, terminal_velocity=tv)
    o.run(time_step=600, steps=steps, time_step_output=600 * steps, export_variables=['lon', 'lat', 'z', 'status'])
    o.ctx.sync()
    e = o.elements
    out = {'steady_ms_per_step': o.timing['steady_ms_per_step'], 'main_loop_s': o.timing['main_loop_s'],
           'active_at_end': int(o.num_elements_active()), 'share_settled': float((e.moving == 0).mean()), 'z_mean': float(e.z.mean()),
           'host_phases_ms_per_step': o.timing['host_phases_ms_per_step']}
    del o
    return out


def mixing(g, n):
    """odr_vmix with the run-time configuration (ODR_NO_VMIX_SPEC=1: the kernel a settle action takes) on the same elements, sea
    floor in reach, with the sea-floor actions lift and settle: ms per launch, best of five."""
    from opendrift_amd.device import Context
    os.environ['ODR_NO_VMIX_SPEC'] = '1'
    ctx = Context(seed=0)
    sid = ctx.add_grid(g['x'], g['y'], z=g['z'])
    for k in range(3):
        ctx.upload_block(sid, k, float(g['t'][k]), {nm: g[nm][k] for nm in NAMES})
    for nm in NAMES:
        ctx.bind(nm, [sid], 10000.0 if nm == 'sea_floor_depth_below_sea_level' else 0.0)
    ctx.bind('sea_surface_height', [], 0.0)
    lon, lat, z, tv = seeds(g, n)
    out = {}
    for action in ('lift_to_seafloor', 'settle'):
        P = ctx.particles(n)
        P.append(lon, lat, z=z, terminal_velocity=tv)
        P.env_sample(['x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity', 'sea_floor_depth_below_sea_level',
                      'sea_surface_height'], 0.0)
        P.store_previous()
        ctx.set_seafloor_action(action)
        best = np.inf
        for k in range(5):
            P.upload(z=z, moving=np.ones(n, np.int32))
            ctx.sync()
            t = time.perf_counter()
            P.vmix(0.0, 600.0, 60.0, step=k)
            ctx.sync()
            best = min(best, 1e3 * (time.perf_counter() - t))
        d = P.download()
        out[action] = {'ms_per_launch': best, 'share_on_the_floor': float((d['z'] <= -3.9).mean()), 'share_settled': float((d['moving'] == 0).mean())}
        P.close()
    ctx.set_seafloor_action('lift_to_seafloor')
    ctx.close()
    del os.environ['ODR_NO_VMIX_SPEC']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=10_000_000)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--small', action='store_true', help='small fields (a rehearsal, not a measurement)')
    ap.add_argument('--only', choices=['sediment', 'ocean', 'mixing'], default=None)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.sedimentdrift import SedimentDrift
    g = fields(a.small)
    res = {'metric': 'steady ms per step of run() (model API, whole loop body)', 'particles': a.particles, 'steps': a.steps,
           'resuspend_kernel_yardstick_ms': 1e3 * RESUSPEND_KERNEL_BYTES * a.particles / HBM_ACHIEVABLE}
    # the model under test runs second: whatever the first run() of a process pays once is not charged to it
    if a.only in (None, 'ocean'):
        res['OceanDrift'] = run(OceanDrift, g, a.particles, a.steps)
    if a.only in (None, 'sediment'):
        res['SedimentDrift'] = run(SedimentDrift, g, a.particles, a.steps)
    if a.only in (None, 'mixing'):
        res['run_time_mixing_kernel'] = mixing(g, a.particles)
    if a.only is None:
        res['value'] = res['SedimentDrift']['steady_ms_per_step']
        res['unit'] = 'ms/step'
        res['ratio_to_OceanDrift'] = res['SedimentDrift']['steady_ms_per_step'] / res['OceanDrift']['steady_ms_per_step']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
