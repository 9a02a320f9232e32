#!/usr/bin/env python
"""Seeding within a polygon on one MI355X: Context.points_within_polygon (odr_polygon_points) for 1e5, 1e6 and 1e7 elements in
star-shaped rings of 64 and 1024 vertices -- the headline workload seeds 10 M elements, and a satellite-derived slick contour has
about a thousand vertices.

    python tools/bench_seed.py [--numbers 100000,1000000,10000000] [--rings 64,1024] [--repeats R] [--host-max N]

One JSON line per (ring, number): `call_ms` the whole synchronous call (set-up on the host, upload of the ring, launches, download
of 16 B per element), `kernel_ms` the device time of its launches (events around them), each the median of R calls after a warm-up
call; `host_ms` ONE run of the reference's method restated in NumPy with matplotlib's Path.contains_points on the host, measured in
the same process (numbers above --host-max are not run on the host).  The grid size and the inside count of the two are compared
before anything is reported; the first call is compared with the host build of the header bit for bit up to --host-check
elements.
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
R = 6370997.0


def numpy_points_within_polygon(lons, lats, number):
    """basemodel/__init__.py:1487-1558 with NumPy's sin / cos / arctan2 / arcsin and matplotlib's Path on the host"""
    from matplotlib.path import Path
    lons, lats = np.asarray(lons, np.float64), np.asarray(lats, np.float64)
    r6 = lambda v: float('%f' % v)
    phi1, phi2 = np.radians(r6(lats.min())), np.radians(r6(lats.max()))
    phi0, lam0 = np.radians(r6((lats.min() + lats.max()) / 2)), np.radians(r6((lons.min() + lons.max()) / 2))
    n = (np.sin(phi1) + np.sin(phi2)) / 2
    c = np.cos(phi1) ** 2 + 2 * n * np.sin(phi1)
    rho0 = np.sqrt(c - 2 * n * np.sin(phi0)) / n
    ring = np.c_[lons, lats]
    if (ring[0] != ring[-1]).any():
        ring = np.vstack([ring, ring[:1]])
    rho = np.sqrt(c - 2 * n * np.sin(np.radians(ring[:, 1]))) / n
    theta = n * ((np.radians(ring[:, 0]) - lam0 + np.pi) % (2 * np.pi) - np.pi)
    x, y = R * rho * np.sin(theta), R * (rho0 - rho * np.cos(theta))
    area = 0.0
    for i in range(-1, len(x) - 1):
        area += x[i] * (y[i + 1] - y[i - 1])
    deltax = np.sqrt(abs(area) / 2 / number)
    xvec = np.linspace(x.min() + deltax / 2, x.max() - deltax / 2, int((x.max() - x.min()) / deltax))
    yvec = np.linspace(y.min() + deltax / 2, y.max() - deltax / 2, int((y.max() - y.min()) / deltax))
    gx, gy = np.meshgrid(xvec, yvec)
    gx, gy = gx.ravel() / R, rho0 - gy.ravel() / R
    rr = np.sign(n) * np.hypot(gx, gy)
    lon = np.degrees(lam0 + np.arctan2(np.sign(n) * gx, np.sign(n) * gy) / n)
    lat = np.degrees(np.arcsin(np.clip((c - (rr * n) ** 2) / (2 * n), -1, 1)))
    ind = Path(ring).contains_points(np.c_[lon, lat])
    L = int(ind.sum())
    k = np.arange(number) % max(L, 1)
    return lon[ind][k], lat[ind][k], dict(n_inside=L, nx=len(xvec), ny=len(yvec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--numbers', default='100000,1000000,10000000')
    ap.add_argument('--rings', default='64,1024')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--host-max', type=int, default=10000000)
    ap.add_argument('--host-check', type=int, default=1000000)
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    from opendrift_amd.device import Context
    import seed_host as sh
    ctx = Context(device=0, seed=0)
    for m in [int(v) for v in a.rings.split(',')]:
        ring = sh.star_ring(m, 4.5, 60.2, 2.0, m)
        for number in [int(v) for v in a.numbers.split(',')]:
            call, kernel = [], []
            for r in range(a.repeats + 1):      # the first call warms up
                t0 = time.perf_counter()
                lon, lat, info = ctx.points_within_polygon(*ring, number, info=True)
                call.append(1e3 * (time.perf_counter() - t0))
                kernel.append(ctx.polygon_points_last_kernel_ms())
            res = dict(ring_vertices=m, number=number, **info, edge_tests=info['nx'] * info['ny'] * (m + 1),
                       call_ms=round(float(np.median(call[1:])), 2), kernel_ms=round(float(np.median(kernel[1:])), 3))
            if number <= a.host_check:
                want = sh.points_within_polygon(*ring, number, info=True)
                assert want[2] == info and np.array_equal(want[0], lon) and np.array_equal(want[1], lat), 'the device differs from the host build'
            if number <= a.host_max:
                t0 = time.perf_counter()
                hlon, hlat, hinfo = numpy_points_within_polygon(*ring, number)
                res['host_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
                assert (hinfo['nx'], hinfo['ny']) == (info['nx'], info['ny']), (hinfo, info)
                res['host_n_inside'] = hinfo['n_inside']
                if hinfo['n_inside'] == info['n_inside']:
                    res['max_abs_diff_deg'] = float(max(np.abs(hlon - lon).max(), np.abs(hlat - lat).max()))
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
