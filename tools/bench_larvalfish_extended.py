#!/usr/bin/env python
"""The three launches of LarvalFishExtended on one MI355X: odr_larvalx_hatch, odr_larvalx_behave (mode dvm and mode depth) and
odr_solar_elevation, 1 M elements spread over 30 W - 30 E, 55 - 80 N at 11:30 UTC on 10 January (about half of them in daylight),
half of them larvae, z between the surface and a sea floor of 20 - 320 m.

    python tools/bench_larvalfish_extended.py [--n N] [--calls K] [--windows W]

One JSON line: ms per call, the mean over a window of K back-to-back calls between two events on the stream, W windows after a
warm-up window; every window starts from the same z and stage_fraction.  Traffic per element: the hatch launch reads hatched and,
for an egg, reads and writes stage_fraction (4 - 12 B); the behaviour launch in mode dvm reads hatched, depth, lon, lat and z and
writes z (4 + 4 + 8 + 8 + 8 + 8 = 40 B for an element that moves, 4 B for an egg in the larva case; 44 B with the hatched store
of the hatch launch counted in); the elevation call writes 8 B per element, reads 16 B and then copies the result to the host,
which its time includes.  The yardstick next to each time is that traffic at the 6.3 TB/s a streaming kernel reaches.
"""
import argparse
import json
import os
import sys
from datetime import datetime

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--windows', type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.device import Context
    from opendrift_amd.oceandrift import solar_time_scalars
    n = a.n
    rng = np.random.default_rng(0)
    lon, lat = rng.uniform(-30, 30, n), rng.uniform(55, 80, n)
    depth = (20 + 300 * (lat - 55) / 25).astype(np.float32)
    z = -rng.uniform(0, 1, n) * depth
    hatched = (np.arange(n) % 2).astype(np.float32)
    stage = rng.uniform(0, 0.5, n).astype(np.float32)
    solar = solar_time_scalars(datetime(2020, 1, 10, 11, 30))
    ctx = Context(device=0, seed=0)
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    P.env_upload('sea_floor_depth_below_sea_level', depth)
    P.set_property(0, stage)
    P.set_property(1, hatched)
    inc = (1800.0 / 86400) / 2.0 / a.calls / 100      # (no egg hatches during the measurement)
    arms = {
        'hatch_ms': lambda: P.larvalx_hatch(inc, 0, 1),
        'behave_dvm_larva_ms': lambda: P.larvalx_behave('dvm', 1800.0, 0.003, (-5.0, 1.0), (-25.0, 2.5), solar, hatched_slot=1),
        'behave_dvm_all_ms': lambda: P.larvalx_behave('dvm', 1800.0, 0.003, (-5.0, 1.0), (-25.0, 2.5), solar, active_only_hatched=False),
        'behave_depth_all_ms': lambda: P.larvalx_behave('depth', 1800.0, 0.003, (-10.0, 1.0), active_only_hatched=False),
        'behave_depth_all_float32_z_ms': lambda: P.larvalx_behave('depth', 1800.0, 0.003, (-10.0, 1.0), active_only_hatched=False, z_is_float32=True),
        'solar_elevation_with_download_ms': lambda: P.solar_elevation(*solar),
    }
    bytes_per_element = {'hatch_ms': 4 + 8 * 0.5, 'behave_dvm_larva_ms': 4 + 36 * 0.5, 'behave_dvm_all_ms': 36, 'behave_depth_all_ms': 20,
                         'behave_depth_all_float32_z_ms': 20, 'solar_elevation_with_download_ms': 24}
    out = {k: [] for k in arms}
    for r in range(a.windows + 1):      # round 0 warms every arm up
        for k, call in arms.items():
            P.upload(z=z)
            P.set_property(0, stage)
            ctx.timer_begin()
            for _ in range(a.calls):
                call()
            ms = ctx.timer_end() / a.calls
            if r:
                out[k].append(round(ms, 4))
    res = dict(n=n, calls_per_window=a.calls, share_in_daylight=float((P.solar_elevation(*solar) > 0).mean()), **out)
    res['yardstick_ms'] = {k: round(1e3 * b * n / HBM_ACHIEVABLE, 5) for k, b in bytes_per_element.items()}
    print(json.dumps(res))
    P.close()
    ctx.close()


if __name__ == '__main__':
    main()
