#!/usr/bin/env python
"""Trajectory lengths on one MI355X: odr_trajectory_lengths at 10 M trajectories x 100 output times (990 M inverse geodesics), the
size get_trajectory_lengths meets after a full-size run.

    python tools/bench_trajectory_lengths.py [--n N] [--times T] [--repeats R] [--host-check K]

The cloud: drifters at 0.05 .. 2 m/s (hourly intervals of 0.2 .. 7 km, float32 positions), a fifth of the trajectories seeded late and
a fifth deactivated early (NaN heads and tails).  One JSON line: `kernel_ms` the device time of the launches (events around them,
summed over the slabs), `call_ms` the whole synchronous call -- upload in slabs, launches, download -- each the median of R calls
after a warm-up call, for
  totals_device_inputs   lon / lat already on the device (torch tensors), total_length alone comes back: 8 B per trajectory
  totals                 host lon / lat, total_length alone
  segments               host lon / lat, distances and speeds too: 16 B per interval leave the device and cross the bounce buffer
Kernel traffic per interval: 8 B read (lon, lat, float32, each position read once per tile plus one column of overlap in 65), 8 B
written (16 B with speeds), 8 B read again by the totals.  The first K trajectories are compared with the host build of the header
bit for bit before anything is reported.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def cloud(n, nt, rng, chunk=1 << 20):
    lon, lat = np.empty((n, nt), np.float32), np.empty((n, nt), np.float32)
    t = np.arange(nt)[None, :]
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        speed = rng.uniform(0.05, 2.0, (m, 1)).astype(np.float32) * 3600.0 / 111.2e3      # degrees of latitude per interval
        az = np.cumsum(rng.standard_normal((m, nt), dtype=np.float32) * 0.3, 1) + rng.uniform(0, 6.28, (m, 1)).astype(np.float32)
        la0 = rng.uniform(55, 70, (m, 1))
        la = la0 + np.cumsum(speed * np.cos(az), 1)
        lo = rng.uniform(-10, 30, (m, 1)) + np.cumsum(speed * np.sin(az), 1) / np.cos(np.radians(la0))
        first = np.where(rng.uniform(size=m) < 0.2, rng.integers(0, nt, m), 0)[:, None]
        last = np.where(rng.uniform(size=m) < 0.2, rng.integers(0, nt, m), nt)[:, None]
        gone = (t < first) | (t >= last)
        lo[gone] = np.nan
        la[gone] = np.nan
        lon[a:a + m], lat[a:a + m] = lo, la
    return lon, lat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000000)
    ap.add_argument('--times', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--host-check', type=int, default=2000)
    a = ap.parse_args()
    import torch
    torch.cuda.init()      # before the library opens the device: asked afterwards, torch's own runtime reports no GPU
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.device import Context
    import geodinv_host as gh
    ctx = Context(device=0, seed=0)
    lon, lat = cloud(a.n, a.times, np.random.default_rng(0))
    dt = 3600.0

    def timed(inputs, segments, shape=None):
        kernel, call = [], []
        for r in range(a.repeats + 1):      # the first call warms up
            t0 = time.perf_counter()
            out = ctx.trajectory_lengths(*inputs, dt, segments=segments, shape=shape)
            call.append(1e3 * (time.perf_counter() - t0))
            kernel.append(ctx.trajectory_lengths_last_kernel_ms())
        return out, round(float(np.median(kernel[1:])), 3), round(float(np.median(call[1:])), 2)

    res = dict(n_trajectories=a.n, n_times=a.times, intervals=a.n * (a.times - 1))
    k = min(a.host_check, a.n)
    want = gh.trajectory_lengths(lon[:k], lat[:k], dt)
    dev = [torch.from_numpy(v).to('cuda:0') for v in (lon, lat)]
    torch.cuda.synchronize()
    total, res['totals_device_inputs_kernel_ms'], res['totals_device_inputs_call_ms'] = timed([v.data_ptr() for v in dev], False, lon.shape)
    assert np.array_equal(total[:k], want[0]), 'the device totals differ from the host build'
    del dev
    torch.cuda.empty_cache()
    total, res['totals_kernel_ms'], res['totals_call_ms'] = timed((lon, lat), False)
    assert np.array_equal(total[:k], want[0])
    out, res['segments_kernel_ms'], res['segments_call_ms'] = timed((lon, lat), True)
    assert all(np.array_equal(o[..., :k], w) for o, w in zip(out, want)), 'the device segments differ from the host build'
    res['kernel_intervals_per_s'] = round(res['intervals'] / (1e-3 * res['totals_device_inputs_kernel_ms']), 0)
    res['mean_total_length_km'] = round(float(total.mean()) / 1e3, 3)
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
