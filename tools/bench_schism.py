#!/usr/bin/env python
"""Three-nearest inverse-distance interpolation on a SCHISM-style mesh on one MI355X (csrc/odr_schism.hip.h): the bare queries
odr_schism_nearest3 in 2-D and in 3-D and the whole odr_schism_sample launch, next to odr_umesh_sample (nearest node, nearest
level, one time level) on the same mesh and to scipy's cKDTree -- the reference's index -- on the same machine in the same process.

    python tools/bench_schism.py [--points 1000000] [--queries 10000000] [--levels 30] [--repeats 3] [--workers 16]
                                 [--host-queries 1000000]

The mesh: `--points` random points over a 60 km square in UTM 33, a quarter of them in a corner a hundredth of its size (spacing
graded 100 : 1), `--levels` vertical levels over depths of 20 .. 200 m that move with an elevation.  The queries: `--queries`
positions inside the box of the nodes at depths of 0 .. 100 m, sorted by the cell of a 1024 x 1024 raster (what the model's spatial
re-sort gives); the bare 2-D query also as drawn.  One JSON line each:

  index     create_ms: odr_schism_create (tree and hull grid built on the host, uploaded); level_upload_ms: zcor + u + v + one 2-D
            variable of one time level; ckdtree_build_ms / ckdtree3_build_ms: cKDTree over the nodes / over one level's cloud
  nearest3  kernel_ms: device time of the launches of one odr_schism_nearest3 (median of R calls after a warm-up); visits: mean
            tree nodes whose distance a query formed; ckdtree_ms: ONE cKDTree.query(k=3, workers=W) of `--host-queries` of the
            same queries, scaled to all of them in ckdtree_ms_scaled; the device's answer is compared with it first
  sample    kernel_ms of one launch: `what` names the variant -- the full call (u, v 3-D + one 2-D variable between two time
            levels, rotated), its parts (one level only; the 2-D variable only; u, v only) and odr_umesh_sample for u, v + the 2-D
            variable on the same mesh
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
U_, V_, SSH = 'x_sea_water_velocity', 'y_sea_water_velocity', 'sea_surface_height'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--queries', type=int, default=10000000)
    ap.add_argument('--levels', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--host-queries', type=int, default=1000000)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from scipy.spatial import ConvexHull, cKDTree
    from opendrift_amd import projection
    from opendrift_amd.device import Context
    import umesh_host as U
    ctx = Context(device=0, seed=0)
    n, nq, L, nh = a.points, a.queries, a.levels, min(a.host_queries, a.queries)
    x, y = U.graded_points(n, 1)
    rng = np.random.default_rng(3)
    depth = rng.uniform(20, 200, n)
    s = 1.0 - np.arange(L) / (L - 1)      # level 0 at the sea bed
    zcor = [(e[:, None] - (depth + e)[:, None] * s[None, :]).astype(np.float32) for e in (rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n))]
    for z in zcor:
        z[depth < 40, :3] = np.nan      # the shallow tenth: three levels below the sea bed
    ring = ConvexHull(np.c_[x, y]).vertices
    proj = projection.parse_proj4(UTM)
    t0 = time.perf_counter()
    mesh = ctx.schism(x, y, x[ring], y[ring], n_levels=L, proj=proj)
    create_ms = 1e3 * (time.perf_counter() - t0)
    fields = {v: [rng.standard_normal((n, L)).astype(np.float32) for _ in range(2)] for v in (U_, V_)}
    fields[SSH] = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    upload_ms = []
    for k in range(2):
        t0 = time.perf_counter()
        mesh.set_zcor(k, 3600.0 * k, zcor[k])
        for v in (U_, V_, SSH):
            mesh.set_level(k, 3600.0 * k, v, fields[v][k])
        upload_ms.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    tree = cKDTree(np.c_[x, y])
    build2 = 1e3 * (time.perf_counter() - t0)
    keep = ~np.isnan(zcor[0])
    t0 = time.perf_counter()
    tree3 = cKDTree(np.c_[np.repeat(x, L).reshape(n, L)[keep], np.repeat(y, L).reshape(n, L)[keep], zcor[0][keep].astype(np.float64)])
    build3 = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(what='index', points=n, levels=L, hull_vertices=len(ring), create_ms=round(create_ms, 1),
                          level_upload_ms=round(float(np.median(upload_ms)), 1), ckdtree_build_ms=round(build2, 1),
                          ckdtree3_build_ms=round(build3, 1))), flush=True)

    qx, qy = rng.uniform(x.min(), x.max(), nq), rng.uniform(y.min(), y.max(), nq)
    fine = rng.random(nq) < 0.25      # a quarter in the refined corner, as the points
    qx[fine] = x.min() + 0.01 * (x.max() - x.min()) * rng.random(fine.sum())
    qy[fine] = y.min() + 0.01 * (y.max() - y.min()) * rng.random(fine.sum())
    qz = -rng.uniform(0, 100, nq)
    cell = (np.minimum(1023, (1024 * (qy - y.min()) / np.ptp(y)).astype(np.int64)) * 1024 +
            np.minimum(1023, (1024 * (qx - x.min()) / np.ptp(x)).astype(np.int64)))
    order = np.argsort(cell, kind='stable')
    sx, sy, sz = qx[order], qy[order], qz[order]
    sub = np.sort(rng.permutation(nq)[:nh])
    for name, args, host in (('2-D as drawn', (qx, qy, None), tree), ('2-D sorted', (sx, sy, None), tree), ('3-D sorted', (sx, sy, sz), tree3)):
        kernel = []
        for r in range(a.repeats + 1):      # the first call warms up
            idx, dist, seen = mesh.nearest3(*args, slot=0, visits=True)
            kernel.append(ctx.schism_last_kernel_ms())
        pts = np.c_[args[0][sub], args[1][sub]] if args[2] is None else np.c_[args[0][sub], args[1][sub], args[2][sub]]
        t0 = time.perf_counter()
        want_d, want_i = host.query(pts, k=3, workers=a.workers)
        host_ms = 1e3 * (time.perf_counter() - t0)
        assert np.array_equal(dist[sub], want_d), 'the device differs from cKDTree in a distance'
        ties = int((idx[sub] != want_i).any(axis=1).sum())      # (equal distances: either index is right)
        print(json.dumps(dict(what='nearest3', queries=nq, order=name, kernel_ms=round(float(np.median(kernel[1:])), 3),
                              visits=round(float(seen.mean()), 2), ckdtree_queries=nh, ckdtree_ms=round(host_ms, 1),
                              ckdtree_ms_scaled=round(host_ms * nq / nh, 1), ckdtree_workers=a.workers, tied_queries=ties)), flush=True)

    lon, lat = projection.Proj(UTM)(sx, sy, inverse=True)
    P = ctx.particles(nq)
    P.append(lon, lat, z=sz)

    def timed(what, launch, clock):
        kernel = []
        for r in range(a.repeats + 1):
            launch()
            kernel.append(clock())
        covered = int(np.isfinite(P.env_download(SSH)).sum())
        print(json.dumps(dict(what='sample', variant=what, elements=nq, kernel_ms=round(float(np.median(kernel[1:])), 3), covered=covered)), flush=True)
    clock = ctx.schism_last_kernel_ms
    timed('u, v (3-D) + one 2-D variable, two time levels', lambda: P.schism_sample(mesh, 0, 1, 0.25, [U_, V_, SSH], [True] * 3), clock)
    timed('u, v (3-D) + one 2-D variable, one time level', lambda: P.schism_sample(mesh, 0, None, 0.0, [U_, V_, SSH], [True] * 3), clock)
    timed('u, v (3-D), two time levels', lambda: P.schism_sample(mesh, 0, 1, 0.25, [U_, V_], [True] * 2), clock)
    timed('u, v (3-D), one time level', lambda: P.schism_sample(mesh, 0, None, 0.0, [U_, V_], [True] * 2), clock)
    timed('one 2-D variable, two time levels', lambda: P.schism_sample(mesh, 0, 1, 0.25, [SSH], [True]), clock)
    mesh.close()

    # the nearest-node reader on the same mesh: u, v on L sigma levels of the nodes + the 2-D variable, the nearest time level
    sig = (-(np.arange(L) + 0.5) / L).astype(np.float32)[:, None] * np.ones((1, n), np.float32)
    um = ctx.umesh(x, y, proj=proj, siglay=sig, h=depth.astype(np.float32))
    for v in (U_, V_):
        um.set_level(0, 0.0, v, np.ascontiguousarray(fields[v][0].T), False)
    um.set_level(0, 0.0, SSH, fields[SSH][0], False)
    timed('odr_umesh_sample: u, v on the sigma layers + one 2-D variable, nearest node', lambda: P.umesh_sample(um, 0, [U_, V_, SSH], [True] * 3),
          ctx.umesh_last_kernel_ms)
    um.close()
    P.close()
    ctx.close()


if __name__ == '__main__':
    main()
