#!/usr/bin/env python
"""Nearest node / face lookup of an unstructured mesh on one MI355X (csrc/odr_umesh.hip.h): the bare query odr_umesh_nearest and the
whole odr_umesh_sample launch, next to scipy's cKDTree -- the reference's index -- on the same machine in the same process.

    python tools/bench_umesh.py [--points 1000000] [--queries 10000000] [--layers 10] [--repeats 3] [--workers 16]

The mesh: `--points` random points over a 60 km square in UTM 33, a quarter of them in a corner a hundredth of its size (spacing
graded 100 : 1), and as many face centres drawn the same way.  The queries: `--queries` positions inside the box of the nodes,
once as drawn (neighbouring lanes far apart) and once sorted by the cell of a 1024 x 1024 raster (what the model's spatial re-sort
gives).  One JSON line each:

  index     create_ms: odr_umesh_create -- both k-d trees built on the host, everything uploaded; ckdtree_build_ms: cKDTree(points)
  nearest   kernel_ms: the device time of the launches of one odr_umesh_nearest (events around them, median of R calls after a
            warm-up call); call_ms: the whole synchronous call with its uploads and downloads; ckdtree_ms: ONE
            cKDTree.query(k=1, workers=W) of the same queries; the device's indices are compared with cKDTree's first
  sample    kernel_ms: the odr_umesh_sample launch for u, v and w on `--layers` sigma layers of the faces (projection, coverage,
            one face search, one sigma search, three gathers, the rotation, the merge), median of R launches after a warm-up
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
UTM = '+proj=utm +zone=33 +ellps=WGS84'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--queries', type=int, default=10000000)
    ap.add_argument('--layers', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from scipy.spatial import cKDTree
    from opendrift_amd import projection
    from opendrift_amd.device import Context
    import umesh_host as U
    ctx = Context(device=0, seed=0)
    n, nq, L = a.points, a.queries, a.layers
    x, y = U.graded_points(n, 1)
    xc, yc = U.graded_points(n, 2)
    rng = np.random.default_rng(3)
    s = (-(np.arange(L) + 0.5) / L).astype(np.float32)[:, None] * np.ones((1, n), np.float32)
    h = rng.uniform(20, 200, n).astype(np.float32)
    t0 = time.perf_counter()
    mesh = ctx.umesh(x, y, xc, yc, proj=projection.parse_proj4(UTM), siglay_center=s, h_center=h)
    create_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    tree = cKDTree(np.c_[x, y])
    print(json.dumps(dict(what='index', points=n, faces=n, create_ms=round(create_ms, 1),
                          ckdtree_build_ms=round(1e3 * (time.perf_counter() - t0), 1))), flush=True)

    qx, qy = rng.uniform(x.min(), x.max(), nq), rng.uniform(y.min(), y.max(), nq)
    fine = rng.random(nq) < 0.25      # a quarter in the refined corner, as the points
    qx[fine] = x.min() + 0.01 * (x.max() - x.min()) * rng.random(fine.sum())
    qy[fine] = y.min() + 0.01 * (y.max() - y.min()) * rng.random(fine.sum())
    cell = (np.minimum(1023, (1024 * (qy - y.min()) / np.ptp(y)).astype(np.int64)) * 1024 +
            np.minimum(1023, (1024 * (qx - x.min()) / np.ptp(x)).astype(np.int64)))
    order = np.argsort(cell, kind='stable')
    for name, sx, sy in (('as drawn', qx, qy), ('sorted', qx[order], qy[order])):
        call, kernel = [], []
        for r in range(a.repeats + 1):      # the first call warms up
            t0 = time.perf_counter()
            got = mesh.nearest(sx, sy)
            call.append(1e3 * (time.perf_counter() - t0))
            kernel.append(ctx.umesh_last_kernel_ms())
        t0 = time.perf_counter()
        want = tree.query(np.c_[sx, sy], k=1, workers=a.workers)[1]
        host_ms = 1e3 * (time.perf_counter() - t0)
        bad, excused = U.unexcused_mismatches(x, y, sx, sy, got, want)
        assert bad == 0, 'the device differs from cKDTree at %d queries' % bad
        print(json.dumps(dict(what='nearest', queries=nq, order=name, kernel_ms=round(float(np.median(kernel[1:])), 3),
                              call_ms=round(float(np.median(call[1:])), 1), ckdtree_ms=round(host_ms, 1), ckdtree_workers=a.workers,
                              excused_mismatches=excused)), flush=True)

    # the whole launch: elements at the sorted positions, u, v, w on the layers of the faces
    sx, sy = qx[order], qy[order]
    lon, lat = projection.Proj(UTM)(sx, sy, inverse=True)
    z = -rng.uniform(0, 100, nq)
    names = ['x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity']
    for k, v in enumerate(names):
        mesh.set_level(0, 0.0, v, rng.standard_normal((L, n)).astype(np.float32), True)
    P = ctx.particles(nq)
    P.append(lon, lat, z=z)
    kernel = []
    for r in range(a.repeats + 1):
        P.umesh_sample(mesh, 0, names, [True] * 3)
        kernel.append(ctx.umesh_last_kernel_ms())
    u = P.env_download(names[0])
    print(json.dumps(dict(what='sample', elements=nq, variables=3, layers=L, kernel_ms=round(float(np.median(kernel[1:])), 3),
                          covered=int(np.isfinite(u).sum()))), flush=True)
    P.close()
    mesh.close()
    ctx.close()


if __name__ == '__main__':
    main()
