#!/usr/bin/env python
"""Milliseconds per odr_oil_weather call -- the reduction for the call-wide decisions plus the fused launch -- at 10 M elements of a
16-component oil on one MI355X, next to the HBM bytes the call moves and the time that traffic alone would take; and one step of
OpenOil.run() with and without weathering.

    python tools/bench_openoil_weathering.py [--n 10000000] [--ncomp 16] [--calls 5] [--windows 3] [--model-particles 2000000]

Arms, each with every element at the surface and with a third of them there (evaporation acts at z == 0 only):
    weather_ms        evaporation + emulsification + dispersion, the reference's defaults
    properties_ms     the reduction and the property update alone: no row is touched
    nothing_ms        no process: the reduction plus a launch that reads and writes the records (an upper bound for the reduction)
Bytes per element of weather_ms: the record read (112 B) and nine of its values written (72 B), the row of mass_components read twice
under evaporation and written once (the second read hits the cache: counted once), id, z, age and three environment values
(28 B), two float32 properties written (8 B).  Each figure is a window of `calls` back-to-back calls between two device events,
divided by `calls`; the arms alternate within a round; round 0 warms up.  The state is reset in front of every window.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0        # MI355X peak; what the traffic alone would take is bytes / this


def oil_of(ncomp):
    bp = np.linspace(350., 900., ncomp)
    return dict(mass_fraction=(np.ones(ncomp) / ncomp).tolist(), boiling_point=bp.tolist(), molecular_weight=(0.4 * bp - 60).tolist(),
                density=870., density_k=0.7, viscosity=2e-5, viscosity_B=2500., bullwinkle_fraction=0.1, bullwinkle_time=None,
                emulsion_water_fraction_max=0.7, oil_water_interfacial_tension=0.025)


def launches(a):
    from opendrift_amd import _abi
    from opendrift_amd.device import Context
    n, oil = a.n, oil_of(a.ncomp)
    rng = np.random.default_rng(0)
    ctx = Context(device=0, seed=0)
    P = ctx.particles(n)
    P.append(np.linspace(4, 5, n), np.full(n, 60.0))
    P.increase_age(900.)
    P.env_upload('x_wind', rng.uniform(2, 15, n).astype(np.float32))
    P.env_upload('y_wind', np.zeros(n, np.float32))
    P.env_upload('sea_water_temperature', rng.uniform(2, 20, n).astype(np.float32))
    for k in (1, 2):
        P.set_property(k, np.zeros(n, np.float32))
    P.weathering_setup(oil, n)
    mass = np.full(n, 10.0)
    out = {}
    for tag, share in (('all_surface', 1.0), ('third_surface', 1 / 3)):
        z = np.where(rng.uniform(size=n) < share, 0.0, -5.0)
        P.upload(z=z)
        arms = {'weather_ms': ['properties', 'evaporation', 'emulsification', 'dispersion'], 'properties_ms': ['properties'], 'nothing_ms': []}
        res = {k: [] for k in arms}
        for r in range(a.windows + 1):
            for k, which in arms.items():
                P.weathering_seed(0, mass, oil['mass_fraction'], 872.2, 2.2e-5)       # the same state in front of every window
                ctx.sync()
                ctx.timer_begin()
                for _ in range(a.calls):
                    P.oil_weather(900., which)
                ms = ctx.timer_end() / a.calls
                if r:
                    res[k].append(round(ms, 4))
        stride = (a.ncomp + 1) & ~1
        per_element = 112 + 72 + 28 + 8 + 16 * stride      # (dispersion scales the rows of the submerged elements too)
        res['bytes_per_element'] = round(per_element, 1)
        res['traffic_alone_ms'] = round(per_element * n / HBM_GBS / 1e6, 4)
        res['double_exponentials_per_call'] = int(2 * a.ncomp * n * share + 3 * n)
        out[tag] = res
    P.close()
    ctx.close()
    return out


def model_step(a, weathering):
    from opendrift_amd import readers, synthetic as synth
    from opendrift_amd.openoil import OpenOil
    from opendrift_amd.projection import stere_polar_inverse
    g = synth.grid_stere(nt=12)
    t0 = datetime(2020, 1, 1)
    times = [t0 + timedelta(seconds=float(t)) for t in g['t']]
    names = [k for k in g if k not in ('x', 'y', 't')]
    o = OpenOil(loglevel=50, seed=0, **({'weathering_model': 'noaa'} if weathering else {}))
    o.add_reader(readers.GridReader(g['x'], g['y'], times, {k: g[k] for k in names}, proj4=synth.NORKYST_PROJ4))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('environment:constant:horizontal_diffusivity', 10)
    o.set_config('general:coastline_action', 'stranding')
    n = a.model_particles
    rng = np.random.default_rng(0)
    x = rng.uniform(g['x'][8], g['x'][int(0.9 * len(g['x']))], n)
    y = rng.uniform(g['y'][8], g['y'][-9], n)
    lon, lat = stere_polar_inverse(x, y, **synth.NORKYST_PROJ)
    oil = oil_of(a.ncomp) if weathering else {'density': 900.0, 'viscosity': 0.005, 'oil_water_interfacial_tension': 0.03}
    o.seed_elements(lon=lon, lat=lat, z=0.0, time=t0, number=n, oil_type=oil)
    t = time.perf_counter()
    o.run(time_step=900, steps=a.model_steps, time_step_output=900 * a.model_steps, export_variables=['lon', 'lat', 'z', 'status'])
    o.ctx.sync()
    el = time.perf_counter() - t
    steady = getattr(o, 'timing', {})
    b = o.get_oil_budget() if weathering else None
    o.P.close()
    return dict(ms_per_step_including_setup=round(1e3 * el / a.model_steps, 3), timing={k: v for k, v in steady.items() if not isinstance(v, dict)},
                mass_total_relative_drift=None if b is None else float(abs(b['mass_total'][-1] / b['mass_total'][0] - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10_000_000)
    ap.add_argument('--ncomp', type=int, default=16)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--model-particles', type=int, default=2_000_000)
    ap.add_argument('--model-steps', type=int, default=8)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    out = dict(n=a.n, ncomp=a.ncomp, calls_per_window=a.calls, launches=launches(a))
    if a.model_particles:
        out['model'] = dict(particles=a.model_particles, steps=a.model_steps, without_weathering=model_step(a, False),
                            with_weathering=model_step(a, True))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
