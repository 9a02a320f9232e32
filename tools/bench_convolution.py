"""Measures the convolution pass of the level preparation (StructuredReader.set_convolution_kernel; csrc/odr_convolve.hip.h) on the
GPU, all in one process:

  1  the preparation of one C3-sized time level (u, v, w, K at 1024 x 1024 x 12, sea floor depth and land mask: 210 MB) that already
     lies in device memory, without a kernel, with N = 3 and with N = 9 -- odr_block_upload_device, host clock around a call that ends
     in a stream synchronisation, the three variants in turn; next to it the time the pass's own traffic would take: one read and
     one write of the level at the 6.3 TB/s a streaming kernel reaches on this GPU;
  2  a run of OceanDrift on the same reader with the asynchronous level upload, without a kernel and with N = 3 and N = 9: the host
     time the run waited for a prefetched level (the binding's stall_s) and the run's wall time.

    python tools/bench_convolution.py [--small] [--reps 10] [--elements 200000]

prints one JSON line."""
import argparse
import json
import os
import sys
import time
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_BYTES_PER_S = 6.3e12


def prepare_times(fields, reps):
    import torch
    from opendrift_amd.device import Context
    g, names = fields['g'], fields['names']
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k][0])).cuda() for k in names}      # (torch first: it brings its own runtime)
    torch.cuda.synchronize()
    ctx = Context(0, seed=0)
    sid = ctx.add_grid(g['x'], g['y'], z=fields['z'])
    ptrs = {k: int(t.data_ptr()) for k, t in dev.items()}
    nzv = {k: (g[k].shape[1] if g[k].ndim == 4 else 1) for k in names}
    level_bytes = sum(t.numel() * 4 for t in dev.values())
    variants = [('none', None), ('N=3', 3), ('N=9', 9)]
    samples = {tag: [] for tag, _ in variants}
    from opendrift_amd import readers
    for rep in range(reps + 2):
        for tag, n in variants:
            ctx.set_convolution(sid, None if n is None else readers.convolution_weights(n))
            ctx.sync()
            t0 = time.perf_counter()
            ctx.upload_block_device(sid, rep % 3, 0.0, ptrs, nzv)      # copy into the staging memory + preparation + commit; synchronous
            ctx.sync()
            if rep >= 2:
                samples[tag].append(time.perf_counter() - t0)
    ctx.close()
    out = dict(level_bytes=level_bytes, traffic_ms=1e3 * 2 * level_bytes / STREAM_BYTES_PER_S)
    for tag, s in samples.items():
        out['prepare_ms ' + tag] = dict(median=1e3 * float(np.median(s)), min=1e3 * float(np.min(s)), max=1e3 * float(np.max(s)))
    base = out['prepare_ms none']['median']
    for tag in ('N=3', 'N=9'):
        out['pass_ms ' + tag] = out['prepare_ms ' + tag]['median'] - base
    return out


def run_stalls(fields, elements):
    from opendrift_amd import readers
    from opendrift_amd.oceandrift import OceanDrift
    g, names = fields['g'], fields['names']
    T0 = datetime(2020, 1, 1)
    times = [T0 + timedelta(seconds=float(t)) for t in g['t']]
    rng = np.random.default_rng(0)
    lon = rng.uniform(g['x'][8], g['x'][int(0.9 * len(g['x']))], elements)
    lat = rng.uniform(g['y'][8], g['y'][-9], elements)
    out = {}
    for tag, n in (('none', None), ('N=3', 3), ('N=9', 9), ('none again', None)):
        r = readers.GridReader(g['x'], g['y'], times, {k: np.ascontiguousarray(g[k]) for k in names}, z=fields['z'])
        r.set_convolution_kernel(n)
        o = OceanDrift(loglevel=50, seed=0)
        o.add_reader(r)
        o.set_config('drift:advection_scheme', 'runge-kutta4')
        o.set_config('general:coastline_action', 'previous')
        o.seed_elements(lon=lon, lat=lat, z=-rng.uniform(0, 30, elements), time=T0)
        steps = int((g['t'][-1] - g['t'][0]) // 600) - 1
        t0 = time.perf_counter()
        o.run(time_step=600, steps=steps)
        wall = time.perf_counter() - t0
        out[tag] = dict(stall_s=float(o.timing['reader_level_stall_s']), run_s=wall, steps=steps,
                        levels=sum(len(b.slots) for b in o.readers.values()))
        del o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--small', action='store_true', help='a 128 x 96 x 8 level: a rehearsal of the script, not a measurement')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--elements', type=int, default=200000)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    fields = bench.make_fields('c3', small=a.small)
    res = dict(tool='bench_convolution', small=a.small, reps=a.reps, prepare=prepare_times(fields, a.reps), runs=run_stalls(fields, a.elements))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
