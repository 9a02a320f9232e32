"""Milliseconds per odr_ship_drift call (ShipDrift.update of every element: one launch) at 1 M ships on C29-shaped input -- the
environment and the hulls of tools/gen_golden_shipdrift.py case (b), tiled -- with ONE class and with 1 000 classes (the golden's
eight class tables repeated: 1 000 x 784 B of table, an index per element that changes from element to element), and next to them
the odr_leeway call (Leeway.update, config C5's kernel) on a set of the same size for scale:

    python tools/bench_shipdrift.py [--n 1000000] [--calls 20] [--windows 5]

Each figure is a window of `calls` back-to-back calls between two device events, divided by `calls`; the three arms alternate
within a round and the rounds are repeated, so that the spread is visible; every arm is warmed up first.  The per-kernel time
comes from the library's own timeline: `rocprofv3 --kernel-trace --stats -- python tools/bench_shipdrift.py` in a run of its own
(k_ship_drift, k_leeway).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opendrift_amd.device import Context  # noqa: E402

DT = 3600.0
TM02 = 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'
# the environment and the float32 properties of a ship, in slot order
ENV = ('x_sea_water_velocity', 'y_sea_water_velocity', 'x_wind', 'y_wind', 'sea_surface_wave_stokes_drift_x_velocity',
       'sea_surface_wave_stokes_drift_y_velocity', 'sea_surface_wave_significant_height', TM02)
PROPS = ('length', 'height', 'draft', 'beam', 'wind_drag_coeff', 'water_drag_coeff')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    a = ap.parse_args()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'c29_shipdrift.npz'))
    m = g['b_orientation'][1] >= 0
    reps = -(-a.n // int(m.sum()))
    tile = lambda v: np.ascontiguousarray(np.tile(v[m], reps)[:a.n])      # noqa: E731
    ctx = Context(device=0, seed=0)
    ctx.slot_aliases[TM02] = 13      # Tm02 in the peak period's slot, as ShipDrift's own context has it
    lon, lat = tile(g['b_lon'][1]), tile(g['b_lat'][1])
    P = ctx.particles(a.n)
    P.append(lon, lat, z=np.zeros(a.n))
    for k in ENV:
        P.env_upload(k, tile(g['b_env_' + k][1]))
    P.env_upload('land_binary_mask', np.zeros(a.n, np.float32))
    for slot, k in enumerate(PROPS):
        P.set_property(slot, tile(g['b_' + k][1]))
    P.set_property(6, tile(g['b_orientation'][1]).astype(np.float32))
    tables = {1: P.ship_table(g['b_class_table'][:1]), 1000: P.ship_table(np.tile(g['b_class_table'], (125, 1, 1)))}
    index = {1: np.zeros(a.n, np.float32), 1000: (np.arange(a.n) % 1000).astype(np.float32)}
    # Leeway on a set of its own: the same wind and current, the coefficients of one object class (plausible values: the
    # reference's table is not read here), orientation alternating
    L = ctx.particles(a.n)
    L.append(lon, lat, z=np.zeros(a.n))
    for k in ENV[:4]:
        L.env_upload(k, tile(g['b_env_' + k][1]))
    for slot, v in enumerate((0.96, 0.54, 0.0, 0.5, 0.1, 0.1, 0.04)):
        L.set_property(slot, np.full(a.n, v, np.float32))
    L.set_property(7, (np.arange(a.n) % 2).astype(np.float32))
    L.set_property(8, np.zeros(a.n, np.float32))

    def ship(k):
        def call(step):
            P.ship_drift(DT, tables[k], hs_mode=0, tp_mode=0, wave_dir_from_stokes=True, check_classes=False)
        return call

    def window(call):
        ctx.timer_begin()
        for s in range(a.calls):
            call(s)
        return ctx.timer_end() / a.calls

    arms = {'ship_drift_1_class_ms': ship(1), 'ship_drift_1000_classes_ms': ship(1000), 'leeway_ms': lambda s: L.leeway(DT, step=s)}
    out = {k: [] for k in arms}
    for r in range(a.windows + 1):      # round 0 warms every arm up
        for k, call in arms.items():
            if k.startswith('ship'):
                P.set_property(7, index[1 if '1_class' in k else 1000])
                P.upload(lon=lon, lat=lat)      # every window starts from the same positions
            ms = window(call)
            if r:
                out[k].append(round(ms, 4))
    print(json.dumps(dict(n=a.n, calls_per_window=a.calls, **out)))
    for t in tables.values():
        t.close()
    P.close()
    L.close()
    ctx.close()


if __name__ == '__main__':
    main()
