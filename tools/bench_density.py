#!/usr/bin/env python
"""Density maps on one MI355X against np.histogram2d on the same arrays on the same machine: odr_density_map at 1 M trajectories x
24 output times into 347 x 442 bins, for a plume-shaped cloud (half of the elements within a few bins of the release point, the
rest spread out) and for a uniform cloud; a fifth of the entries NaN, 40 % at the surface, 10 % stranded.

    python tools/bench_density.py [--n N] [--times T] [--repeats R] [--skip-numpy]

One JSON line per cloud: `kernel_ms` the device time of the launches (events around them, summed over the slabs), `call_ms` the whole
synchronous call from host arrays (upload in slabs, launches, download of the three float64 maps), `call_device_inputs_ms` the same
with the five inputs already on the device, each the median of R calls after a warm-up call; `weighted_*` the same with a weight
(float64 atomic adds); `numpy_s` the reference's loop -- three np.histogram2d per output time -- once.  The counts are compared with
NumPy's before anything is reported.  Traffic of the kernel: 16 B read per entry (20 B with a weight) and at most three 4-B (8-B)
atomic adds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRANDED = 2


def cloud(kind, n, nt, rng):
    shape = (n, nt)
    if kind == 'plume':
        core = rng.uniform(size=(n, 1)) < 0.5
        drift = np.arange(nt)[None, :] * 0.002
        lon = np.where(core, rng.normal(4.9, 0.003, shape), rng.normal(4.9, 0.05, shape)) + drift
        lat = np.where(core, rng.normal(60.1, 0.002, shape), rng.normal(60.1, 0.03, shape)) + drift / 2
    else:
        lon, lat = rng.uniform(4.65, 5.15, shape), rng.uniform(59.95, 60.25, shape)
    z = -rng.uniform(0.1, 30.0, shape)
    z[rng.uniform(size=shape) < 0.4] = 0.0
    status = np.zeros(shape)
    stranded = rng.uniform(size=shape) < 0.1
    status[stranded], z[stranded] = STRANDED, 0.0
    weight = rng.uniform(0.05, 3.0, shape)
    late = np.arange(nt)[None, :] < np.where(rng.uniform(size=n) < 0.4, rng.integers(0, nt, n), 0)[:, None]
    out = [lon, lat, z, status, weight]
    for a in out:
        a[late] = np.nan
    return [np.ascontiguousarray(a, np.float32) for a in out]


def numpy_maps(lon, lat, z, status, bins):
    """the reference's loop (basemodel/__init__.py:4110-4144)"""
    lon, lat, z, status = lon.T.copy(), lat.T.copy(), z.T, status.T
    lon_sub, lat_sub, lon_str, lat_str = lon.copy(), lat.copy(), lon.copy(), lat.copy()
    lon_sub[z >= 0] = 1000
    lat_sub[z >= 0] = 1000
    lon[z < 0] = 1000
    lat[z < 0] = 1000
    lon_str[status != STRANDED] = 1000
    lat_str[status != STRANDED] = 1000
    H = np.zeros((lon.shape[0], len(bins[0]) - 1, len(bins[1]) - 1))
    Hsub, Hstr = H.copy(), H.copy()
    for i in range(lon.shape[0]):
        H[i] = np.histogram2d(lon[i], lat[i], bins=bins)[0]
        Hsub[i] = np.histogram2d(lon_sub[i], lat_sub[i], bins=bins)[0]
        Hstr[i] = np.histogram2d(lon_str[i], lat_str[i], bins=bins)[0]
    return H, Hsub, Hstr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--times', type=int, default=24)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--skip-numpy', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.device import Context
    ctx = Context(device=0, seed=0)
    bins = (np.arange(348) * (0.5 / 347) + 4.65, np.arange(443) * (0.3 / 442) + 59.95)
    n_entries = a.n * a.times
    P = ctx.particles(n_entries)      # its float32 environment slots hold the device copies of the inputs
    P.append(np.zeros(n_entries), np.zeros(n_entries))
    for kind in ('plume', 'uniform'):
        arr = cloud(kind, a.n, a.times, np.random.default_rng(0))
        for k in range(5):
            P.env_upload(k, arr[k].ravel())
        ctx.sync()
        ptr = [P.device_ptr('env:%d' % k) for k in range(5)]

        def timed(inputs, weight, shape=None):
            kernel, call = [], []
            for r in range(a.repeats + 1):      # the first call warms up
                t0 = time.perf_counter()
                out = ctx.density_map(*inputs, bins[0], bins[1], weight=weight, stranded_code=STRANDED, shape=shape)
                call.append(1e3 * (time.perf_counter() - t0))
                kernel.append(ctx.density_last_kernel_ms())
            return out, round(float(np.median(kernel[1:])), 4), round(float(np.median(call[1:])), 2)

        res = dict(cloud=kind, n_trajectories=a.n, n_times=a.times, bins=[len(bins[0]) - 1, len(bins[1]) - 1])
        out, res['kernel_ms'], res['call_ms'] = timed(arr[:4], None)
        _, res['kernel_device_inputs_ms'], res['call_device_inputs_ms'] = timed(ptr[:4], None, arr[0].shape)
        _, res['weighted_kernel_ms'], res['weighted_call_ms'] = timed(arr[:4], arr[4])
        res['largest_bin'] = float(out[0].max())
        res['entries_counted'] = [float(h.sum()) for h in out]
        res['kernel_entries_per_s'] = round(n_entries / (1e-3 * res['kernel_ms']), 0)
        if not a.skip_numpy:
            t0 = time.perf_counter()
            want = numpy_maps(*arr[:4], bins)
            res['numpy_s'] = round(time.perf_counter() - t0, 3)
            assert all(np.array_equal(h, w) for h, w in zip(out, want)), 'the device maps differ from np.histogram2d'
            res['numpy_over_call'] = round(1e3 * res['numpy_s'] / res['call_ms'], 1)
            res['numpy_over_kernel'] = round(1e3 * res['numpy_s'] / res['kernel_ms'], 1)
        print(json.dumps(res), flush=True)
    P.close()
    ctx.close()


if __name__ == '__main__':
    main()
