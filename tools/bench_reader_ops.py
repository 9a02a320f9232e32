"""Times the reader-operator launch on the device (odr_combined_sample: the front door k_combined_front and k_combined_sample) against the floor a
separate-launch design would pay: two plain odr_env_sample calls of the same operands.

Two 3-D latlong grids (u, v on nz levels), elements drawn over the overlap of the two, sorted by cell as a run's elements are after
the spatial re-sort; one JSON line per measurement, the median of the repeats after a warm-up.

    python tools/bench_reader_ops.py --elements 10000000
"""
import argparse
import json
import os
import sys
from datetime import datetime, timedelta

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opendrift_amd import readers  # noqa: E402
from opendrift_amd.device import Context  # noqa: E402

U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
T0 = datetime(2020, 1, 1)


def grid(name, nx, ny, nz, x0, seed):
    rng = np.random.default_rng(seed)
    times = [T0, T0 + timedelta(hours=1)]
    arrays = {v: rng.standard_normal((2, nz, ny, nx)).astype(np.float32) for v in (U, V)}
    return readers.GridReader(x0 + 0.01 * np.arange(nx), 58.0 + 0.01 * np.arange(ny), times, arrays, z=-5.0 * np.arange(nz), name=name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--elements', type=int, default=10_000_000)
    ap.add_argument('--nx', type=int, default=400)
    ap.add_argument('--ny', type=int, default=300)
    ap.add_argument('--nz', type=int, default=12)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    ctx = Context(device=0, seed=0)
    ga, gb = grid('a', a.nx, a.ny, a.nz, 3.0, 1), grid('b', a.nx, a.ny, a.nz, 3.5, 2)
    ts = readers.TimeseriesReader({'time': [T0, T0 + timedelta(hours=1)], U: [0.5, 0.6], V: [-0.1, -0.2], 'lon': 5.0, 'lat': 59.5})
    rng = np.random.default_rng(0)
    n = a.elements
    lon, lat = rng.uniform(3.6, 6.9, n), rng.uniform(58.1, 60.9, n)      # inside both grids
    order = np.argsort((np.floor((lat - 58.0) / 0.04) * 1024 + np.floor((lon - 3.0) / 0.04)).astype(np.int64), kind='stable')
    P = ctx.particles(n)
    P.append(lon[order], lat[order], z=-rng.uniform(0, 50, n))
    t = T0 + timedelta(minutes=20)
    for name, expr in (('a + b', ga + gb), ('(a + b) / 2', (ga + gb) / 2), ('a.combine_gaussian(ts, 50 km)', ga.combine_gaussian(ts, 50000.0))):
        b = readers.DeviceReaderBinding(ctx, expr, variables=[U, V])
        ms = []
        for r in range(a.repeats + 1):      # the first call warms up (and uploads the leaves' levels)
            b.sample_combined(P, [U, V], [True, True], t)
            ms.append(ctx.combined_last_kernel_ms())
        u = P.env_download(U)
        print(json.dumps(dict(what='odr_combined_sample', expression=name, elements=n, variables=2, levels=a.nz,
                              kernels_ms=round(float(np.median(ms[1:])), 3), finite=int(np.isfinite(u).sum()))), flush=True)
        leaves = [lb for _, lb, _ in b.leaves]
    # the floor of a design with one launch per operand: odr_env_sample of a, then of b (the sum would be a third pass)
    total = 0.0
    for lb in leaves[:1] + [readers.DeviceReaderBinding(ctx, gb, variables=[U, V])]:
        lb.ensure_levels(t, t, times=[t])
        for v in (U, V):
            ctx.bind(v, [lb.sid], None)
        ms = []
        for r in range(a.repeats + 1):
            ctx.timer_begin()
            P.env_sample([U, V], readers._epoch(t))
            ms.append(ctx.timer_end())
        total += float(np.median(ms[1:]))
        print(json.dumps(dict(what='odr_env_sample', reader=lb.reader.name, elements=n, variables=2, kernel_ms=round(float(np.median(ms[1:])), 3))), flush=True)
    print(json.dumps(dict(what='two plain odr_env_sample calls', kernel_ms=round(total, 3))), flush=True)
    P.close()
    ctx.close()


if __name__ == '__main__':
    main()
