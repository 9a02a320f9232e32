#!/usr/bin/env python
"""LarvalFish.run() through the model API at C3 size on one MI355X, next to OceanDrift.run() on the same fields in the same
call (machines differ by several per cent: only same-call numbers compare).  C3 fields (1024 x 1024 x 12 lon / lat / z block:
current, vertical velocity, diffusivity, depth, land mask) plus float32 temperature and salinity, stratified in z with a
horizontal wave; 10 M elements -- half larvae of 0.08 - 50 mg, half eggs, a tenth of them about to hatch --, RK4 + vertical
mixing (60 s sub-steps), device RNG.

    python tools/bench_larvalfish.py [--particles N] [--steps K] [--small] [--only larval|ocean]

One JSON line: steady ms per step (the loop body after the first step) of both models.  OceanDrift takes run()'s fused lane,
LarvalFish the call-by-call lane with its three launches (k_larval_update, k_egg_terminal_velocity, k_larval_migrate); the
kernels' own times come from a `rocprofv3 --kernel-trace --stats -- python tools/bench_larvalfish.py --only larval` run.
k_larval_update moves 20 B per element (200 MB at 10 M elements, 0.032 ms at 6.3 TB/s), k_larval_migrate 4 B per egg and 24 B
per larva (at most 240 MB, 0.038 ms).
"""
import argparse
import json
import os
import sys
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12
UPDATE_KERNEL_BYTES, MIGRATE_KERNEL_BYTES = 20, 24


def fields(small):
    from opendrift_amd import synthetic as synth
    nx, ny, nz = (128, 96, 8) if small else (1024, 1024, 12)
    g = synth.grid3d(nx=nx, ny=ny, nz=nz, nt=3, seed=0)
    X, Y = np.meshgrid(np.linspace(0, 1, nx, dtype=np.float32), np.linspace(0, 1, ny, dtype=np.float32))
    wave_t = np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y)
    wave_s = 0.5 * np.sin(3 * X + 2 * Y)
    T = np.empty(g['x_sea_water_velocity'].shape, np.float32)
    S = np.empty_like(T)
    for it in range(T.shape[0]):
        for k in range(nz):
            T[it, k] = 4 + 8 * np.exp(g['z'][k] / 50.0) + wave_t
            S[it, k] = 35 - 3 * np.exp(g['z'][k] / 30.0) + wave_s
    g['sea_water_temperature'], g['sea_water_salinity'] = T, S
    return g


def run(cls, g, n, steps):
    t0 = datetime(2020, 1, 1)
    times = [t0 + timedelta(seconds=float(t)) for t in g['t']]
    from opendrift_amd import readers
    names = ['x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity', 'ocean_vertical_diffusivity',
             'sea_floor_depth_below_sea_level', 'land_binary_mask', 'sea_water_temperature', 'sea_water_salinity']
    o = cls(loglevel=50, seed=0)
    o.add_reader(readers.GridReader(g['x'], g['y'], times, {k: g[k] for k in names if k in cls.required_variables}, z=g['z']))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('drift:vertical_mixing', True)
    o.set_config('vertical_mixing:timestep', 60)
    o.set_config('general:coastline_action', 'previous')
    rng = np.random.default_rng(0)
    lon = rng.uniform(g['x'][8], g['x'][int(0.9 * len(g['x']))], n)
    lat = rng.uniform(g['y'][8], g['y'][-9], n)
    kw = {}
    if 'weight' in getattr(cls, 'aux_properties', []):
        larva = np.arange(n) % 2 == 0
        kw = dict(diameter=rng.uniform(0.001, 0.0018, n).astype(np.float32),
                  neutral_buoyancy_salinity=rng.uniform(30, 36, n).astype(np.float32), hatched=larva.astype(np.float32),
                  weight=np.where(larva, np.exp(rng.uniform(np.log(0.08), np.log(50.0), n)), 0.08).astype(np.float32),
                  stage_fraction=np.where(larva, 1.0, np.where(np.arange(n) % 20 == 1, rng.uniform(0.997, 1.0, n),
                                                               rng.uniform(0.0, 0.9, n))).astype(np.float32))
    o.seed_elements(lon=lon, lat=lat, z=-rng.uniform(0, 50, n), time=t0, **kw)
    o.run(time_step=600, steps=steps, time_step_output=600 * steps, export_variables=['lon', 'lat', 'z', 'status'])
    o.ctx.sync()
    e = o.elements
    out = {'steady_ms_per_step': o.timing['steady_ms_per_step'], 'main_loop_s': o.timing['main_loop_s'],
           'active_at_end': int(o.num_elements_active()), 'share_at_surface': float((e.z == 0).mean()), 'z_mean': float(e.z.mean()),
           'host_phases_ms_per_step': o.timing['host_phases_ms_per_step']}
    if kw:
        out['terminal_velocity_range'] = [float(e.terminal_velocity.min()), float(e.terminal_velocity.max())]
        out['share_hatched'] = float((e.hatched == 1).mean())
        out['weight_range'] = [float(e.weight.min()), float(e.weight.max())]
    del o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--particles', type=int, default=10_000_000)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--small', action='store_true', help='small fields (a rehearsal, not a measurement)')
    ap.add_argument('--only', choices=['larval', 'ocean'], default=None)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.larvalfish import LarvalFish
    g = fields(a.small)
    res = {'metric': 'steady ms per step of run() (model API, whole loop body)', 'particles': a.particles, 'steps': a.steps,
           'update_kernel_yardstick_ms': 1e3 * UPDATE_KERNEL_BYTES * a.particles / HBM_ACHIEVABLE,
           'migrate_kernel_yardstick_ms': 1e3 * MIGRATE_KERNEL_BYTES * a.particles / HBM_ACHIEVABLE}
    # the model under test runs second: whatever the first run() of a process pays once is not charged to it
    if a.only != 'larval':
        res['OceanDrift'] = run(OceanDrift, g, a.particles, a.steps)
    if a.only != 'ocean':
        res['LarvalFish'] = run(LarvalFish, g, a.particles, a.steps)
    if a.only is None:
        res['value'] = res['LarvalFish']['steady_ms_per_step']
        res['unit'] = 'ms/step'
        res['ratio_to_OceanDrift'] = res['LarvalFish']['steady_ms_per_step'] / res['OceanDrift']['steady_ms_per_step']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
