#!/usr/bin/env python
"""Land mask from coastline polygons on one MI355X (csrc/odr_shape.hip.h): the index build, the bare query odr_shape_contains and the
whole odr_shape_sample launch, next to the path they replace -- the host-evaluated lane: positions downloaded, the same predicate
on the host (matplotlib's Path.contains_points per ring behind a bounding-box prefilter, at most 16 threads), values uploaded.

    python tools/bench_shape.py [--edges 1000000] [--queries 10000000] [--repeats 3] [--workers 16] [--host-queries 20000]

The coastline is formed by exact operations only (sums, products, quotients, integer arithmetic: the same bits on every machine):
a mainland ring around (1, 60) that holds 60 % of the edges, star-shaped about its centre, ten stretches of which each is smooth
over nine tenths of its length (a tenth of its vertices) and densely indented over the last tenth (nine tenths of its vertices,
alternating in radius: spacing graded about 80 : 1); and 4 000 islands of equal vertex count on a lattice east of it.  The
queries: `--queries` positions drawn over the box of the rings, once as drawn and once sorted by the cell of the index's grid
(what the model's spatial re-sort gives).  One JSON line each:

  index     create_ms: odr_shape_create (grid and lists built on the host, uploaded); the odr_shape_stats figures
  contains  kernel_ms: device time of the launches of one odr_shape_contains (median of R calls after a warm-up call); call_ms: the
            whole synchronous call with uploads and downloads; hbm_fraction: the bytes the launch must move at least (16 in, 4 out
            per position) over the kernel time, as a share of 8 TB/s
  sample    kernel_ms: the odr_shape_sample launch (projection-free lon / lat, coverage, walk, merge), median of R after a warm-up
  host      the host-evaluated lane for `--host-queries` of the positions, and that time scaled to all of them: download_ms,
            predicate_ms, upload_ms; the device's mask is compared with the host's first
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _unit(index, salt):
    """A fixed pseudo-random value in [0, 1] per (index, salt): multiples of 1 / 1000."""
    h = (np.asarray(index, np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(2 ** 32)
    return ((h >> np.uint64(8)) % np.uint64(1001)).astype(np.float64) / 1000.0


def _diamond(u):
    """Direction (dx, dy) with |dx| + |dy| = 1 for the turn u in [0, 1): piecewise linear, exact."""
    q = np.floor(4.0 * u)
    t = 4.0 * u - q
    a, b = 1.0 - t, t
    dx = np.where(q == 0, a, np.where(q == 1, -b, np.where(q == 2, -a, b)))
    dy = np.where(q == 0, b, np.where(q == 1, a, np.where(q == 2, -b, -a)))
    return dx, dy


def coastline(n_edges, n_islands=4000):
    """[ring, ...]: the mainland first, then the islands."""
    n_main = int(0.6 * n_edges) // 10 * 10
    per = n_main // 10
    k = np.arange(per, dtype=np.float64)
    f = k / per
    dense = f >= 0.1
    local = np.where(dense, 0.9 + (f - 0.1) / 9.0, f * 9.0)      # a tenth of the vertices over 0.9 of the stretch, the rest over 0.1
    u = np.concatenate([(j + local) / 10.0 for j in range(10)])
    idx = np.arange(n_main)
    tri = np.abs(2.0 * (3.0 * u - np.floor(3.0 * u)) - 1.0)
    r = 1.2 * (0.75 + 0.25 * tri)
    r = r * np.where(np.tile(dense, 10), 1.0 - 0.01 * (idx % 2) - 0.005 * _unit(idx, 3), 1.0 - 0.01 * _unit(idx, 5))
    dx, dy = _diamond(u)
    rings = [np.c_[1.0 + 1.5 * r * dx, 60.0 + r * dy]]
    per_island = max(8, (n_edges - n_main) // n_islands)
    ui = np.arange(per_island, dtype=np.float64) / per_island
    ddx, ddy = _diamond(ui)
    for i in range(n_islands):
        cx, cy = 3.6 + 0.03 * (i % 80), 58.8 + 0.05 * (i // 80)
        rad = 0.011 * (0.6 + 0.4 * _unit(np.arange(per_island) + i * per_island, 7))
        rings.append(np.c_[cx + rad * ddx, cy + rad * ddy])
    return rings


def host_predicate(rings, x, y, workers):
    """contains_xy of the union on the host: matplotlib per ring behind a bounding-box prefilter."""
    from matplotlib.path import Path
    pts = np.c_[x, y]
    boxes = [(r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max()) for r in rings]

    def one(k):
        x0, x1, y0, y1 = boxes[k]
        m = np.flatnonzero((x >= x0) & (x <= x1) & (y >= y0) & (y <= y1))
        if not len(m):
            return m
        return m[Path(rings[k]).contains_points(pts[m])]
    out = np.zeros(len(x), bool)
    with ThreadPoolExecutor(max(1, min(16, workers))) as ex:
        for hit in ex.map(one, range(len(rings))):
            out[hit] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--edges', type=int, default=1000000)
    ap.add_argument('--queries', type=int, default=10000000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--host-queries', type=int, default=20000)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd import readers
    from opendrift_amd.device import Context
    ctx = Context(device=0, seed=0)
    rings = coastline(a.edges)
    r = readers.ShapeReader(rings)
    t0 = time.perf_counter()
    shape = ctx.shape(r.x1, r.y1, r.x2, r.y2, r.poly, r.n_polygons)
    create_ms = 1e3 * (time.perf_counter() - t0)
    st = shape.stats()
    print(json.dumps(dict(what='index', edges=len(r.x1), polygons=r.n_polygons, create_ms=round(create_ms, 1), **st)), flush=True)

    nq = a.queries
    rng = np.random.default_rng(3)
    x0, x1, y0, y1 = r.box
    qx, qy = rng.uniform(x0, x1, nq), rng.uniform(y0, y1, nq)
    nx, ny = int(st['nx']), int(st['ny'])
    cell = (np.minimum(ny - 1, (ny * (qy - y0) / (y1 - y0)).astype(np.int64)) * nx + np.minimum(nx - 1, (nx * (qx - x0) / (x1 - x0)).astype(np.int64)))
    order = np.argsort(cell, kind='stable')
    got = None
    for name, sx, sy in (('as drawn', qx, qy), ('sorted', qx[order], qy[order])):
        call, kernel = [], []
        for _ in range(a.repeats + 1):      # the first call warms up
            t0 = time.perf_counter()
            got = shape.contains(sx, sy)
            call.append(1e3 * (time.perf_counter() - t0))
            kernel.append(ctx.shape_last_kernel_ms())
        ms = float(np.median(kernel[1:]))
        print(json.dumps(dict(what='contains', queries=nq, order=name, kernel_ms=round(ms, 3), kernel_ms_all=[round(v, 3) for v in kernel[1:]],
                              call_ms=round(float(np.median(call[1:])), 1), land=int((got == 1).sum()),
                              hbm_fraction=round(20.0 * nq / (ms * 1e-3) / 8e12, 4))), flush=True)

    sx, sy = qx[order], qy[order]
    P = ctx.particles(nq)
    P.append(sx, sy, z=np.zeros(nq))
    kernel = []
    for _ in range(a.repeats + 1):
        P.shape_sample(shape, True)
        kernel.append(ctx.shape_last_kernel_ms())
    ms = float(np.median(kernel[1:]))
    dev = P.env_download('land_binary_mask')
    assert np.array_equal(dev, got), 'the sample launch differs from the bare query'
    print(json.dumps(dict(what='sample', elements=nq, kernel_ms=round(ms, 3), kernel_ms_all=[round(v, 3) for v in kernel[1:]],
                          hbm_fraction=round(24.0 * nq / (ms * 1e-3) / 8e12, 4))), flush=True)

    # the host-evaluated lane: download, predicate, upload
    t0 = time.perf_counter()
    d = P.download()
    download_ms = 1e3 * (time.perf_counter() - t0)
    nh = min(nq, a.host_queries)
    pick = rng.choice(nq, nh, replace=False)
    t0 = time.perf_counter()
    host = host_predicate(rings, d['lon'][pick], d['lat'][pick], a.workers)
    predicate_ms = 1e3 * (time.perf_counter() - t0)
    differ = int((host != (dev[pick] == 1)).sum())
    t0 = time.perf_counter()
    P.env_upload('land_binary_mask', dev)
    ctx.sync()
    upload_ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(what='host', elements=nq, download_ms=round(download_ms, 1), upload_ms=round(upload_ms, 1), predicate_queries=nh,
                          predicate_ms=round(predicate_ms, 1), predicate_ms_scaled_to_all=round(predicate_ms * nq / nh, 1), workers=min(16, a.workers),
                          differ_from_device=differ)), flush=True)
    assert differ == 0, 'the device differs from matplotlib at %d positions' % differ
    P.close()
    shape.close()
    ctx.close()


if __name__ == '__main__':
    main()
