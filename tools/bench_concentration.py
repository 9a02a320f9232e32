#!/usr/bin/env python
"""Projected density maps and radionuclide concentration maps on one MI355X: odr_density_map_proj and odr_species_layer_map at 10 M
trajectories x 24 output times against odr_density_map on the same longitudes / latitudes and edges (kind latlong: the projected
kernel should cost that plus its projection), and against the reference's NumPy loops on the same machine.

    python tools/bench_concentration.py [--n N] [--times T] [--repeats R] [--numpy-n M] [--skip-numpy]

One JSON line.  `*_kernel_ms`: the device time of the launches (events around them, summed over the slabs), the median of R calls
after a warm-up call; `*_call_ms`: the whole synchronous call from host arrays (upload in slabs, launches, download).
  density_map         odr_density_map, 347 x 442 bins in degrees
  proj_latlong        odr_density_map_proj, the same edges, kind latlong      ratio_latlong = proj_latlong / density_map (kernel)
  proj_laea           odr_density_map_proj, Lambert azimuthal equal-area, 500 m pixels
  species_moll        odr_species_layer_map, Mollweide, 500 m pixels, 3 species x 5 layers
The NumPy loops (np.histogram2d per output time and map, resp. per output time, species and layer on a boolean selection, after
projecting with projection.Proj) run ONCE on the first M trajectories (default 1 M: the full size takes minutes); `numpy_*_s` is
that time, `numpy_*_over_call` the ratio per entry to the device call.  The latlong maps are compared with odr_density_map's
(equal), the others with NumPy's on the M trajectories: the host mirror's projection and the device's differ by 1e-9 m, so an entry
within that of an edge may fall either way -- at most one entry in a million may, or nothing is reported.
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
STRANDED = 2
LAEA = '+proj=laea +lat_0=60 +lon_0=5 +ellps=WGS84'
MOLL = '+proj=moll +ellps=WGS84 +lon_0=0.0'
Z_ARRAY = np.array([-10000.0, -25.0, -10.0, -5.0, -1.0, 0.0])


def cloud(n, nt, rng):
    """a plume (half of the elements within a few bins of the release point), float32 throughout; a fifth of the entries NaN"""
    shape = (n, nt)
    core = rng.uniform(size=(n, 1)) < 0.5
    sig = np.where(core, np.float32(0.003), np.float32(0.05)).astype(np.float32)
    drift = (np.arange(nt, dtype=np.float32) * np.float32(0.002))[None, :]
    lon = rng.standard_normal(shape, dtype=np.float32) * sig + np.float32(4.9) + drift
    lat = rng.standard_normal(shape, dtype=np.float32) * (sig * np.float32(0.6)) + np.float32(60.1) + drift / 2
    z = -30.0 * rng.random(shape, dtype=np.float32)
    u = rng.random(shape, dtype=np.float32)
    z[u < 0.4] = 0.0
    status = np.zeros(shape, np.float32)
    status[u < 0.1] = STRANDED
    specie = np.floor(3 * rng.random(shape, dtype=np.float32))
    late = np.arange(nt)[None, :] < np.where(rng.random(n) < 0.4, rng.integers(0, nt, n), 0)[:, None]
    out = [lon, lat, z, status, specie]
    for a in out:
        a[late] = np.nan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000000)
    ap.add_argument('--times', type=int, default=24)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--numpy-n', type=int, default=1000000)
    ap.add_argument('--skip-numpy', action='store_true')
    a = ap.parse_args()
    import __graft_entry__ as G
    G.build()
    import conc_host
    from opendrift_amd import projection
    from opendrift_amd.device import Context
    ctx = Context(device=0, seed=0)
    lon, lat, z, status, specie = cloud(a.n, a.times, np.random.default_rng(0))
    bins = (np.arange(348) * (0.5 / 347) + 4.65, np.arange(443) * (0.3 / 442) + 59.95)
    grids = {}
    for name, proj4 in (('laea', LAEA), ('moll', MOLL)):
        P = projection.Proj(proj4)
        x, y = P(np.array([4.65, 5.15]), np.array([59.95, 60.25]))
        grids[name] = (P, np.arange(min(x), max(x), 500.0), np.arange(min(y), max(y), 500.0))

    def timed(call, last_ms):
        kernel, whole = [], []
        for r in range(a.repeats + 1):      # the first call warms up
            t0 = time.perf_counter()
            out = call()
            whole.append(1e3 * (time.perf_counter() - t0))
            kernel.append(last_ms())
        return out, round(float(np.median(kernel[1:])), 4), round(float(np.median(whole[1:])), 2)

    res = dict(n_trajectories=a.n, n_times=a.times, bins_latlong=[347, 442], bins_laea=[len(g) - 1 for g in grids['laea'][1:]],
               bins_moll=[len(g) - 1 for g in grids['moll'][1:]])
    base, res['density_map_kernel_ms'], res['density_map_call_ms'] = timed(
        lambda: ctx.density_map(lon, lat, z, status, bins[0], bins[1], stranded_code=STRANDED), ctx.density_last_kernel_ms)
    out, res['proj_latlong_kernel_ms'], res['proj_latlong_call_ms'] = timed(
        lambda: ctx.density_map_proj(None, lon, lat, z, status, bins[0], bins[1], stranded_code=STRANDED), ctx.conc_last_kernel_ms)
    assert all(np.array_equal(h, w) for h, w in zip(out, base)), 'odr_density_map_proj (latlong) differs from odr_density_map'
    res['ratio_latlong'] = round(res['proj_latlong_kernel_ms'] / res['density_map_kernel_ms'], 3)
    P, xs, ys = grids['laea']
    laea, res['proj_laea_kernel_ms'], res['proj_laea_call_ms'] = timed(
        lambda: ctx.density_map_proj(P.params, lon, lat, z, status, xs, ys, stranded_code=STRANDED), ctx.conc_last_kernel_ms)
    res['ratio_laea'] = round(res['proj_laea_kernel_ms'] / res['density_map_kernel_ms'], 3)
    Pm, xm, ym = grids['moll']
    spec, res['species_moll_kernel_ms'], res['species_moll_call_ms'] = timed(
        lambda: ctx.species_layer_map(Pm.params, lon, lat, z, specie, xm, ym, Z_ARRAY, 3), ctx.conc_last_kernel_ms)
    res['ratio_species_moll'] = round(res['species_moll_kernel_ms'] / res['density_map_kernel_ms'], 3)
    res['entries_counted'] = [float(h.sum()) for h in base] + [float(laea[0].sum()), float(spec.sum())]
    res['kernel_entries_per_s'] = {k: round(a.n * a.times / (1e-3 * res[k + '_kernel_ms']), 0) for k in ('density_map', 'proj_latlong', 'proj_laea', 'species_moll')}
    if not a.skip_numpy:
        m = min(a.numpy_n, a.n)
        sub = [v[:m] for v in (lon, lat, z, status, specie)]
        scale = a.n / m
        t0 = time.perf_counter()
        want = conc_host.density_proj_maps(P, *sub[:4], xs, ys, None, STRANDED)
        res['numpy_n'] = m
        res['numpy_proj_laea_s'] = round(time.perf_counter() - t0, 3)
        res['numpy_proj_laea_over_call'] = round(1e3 * res['numpy_proj_laea_s'] * scale / res['proj_laea_call_ms'], 1)
        res['numpy_proj_laea_over_kernel'] = round(1e3 * res['numpy_proj_laea_s'] * scale / res['proj_laea_kernel_ms'], 1)
        t0 = time.perf_counter()
        wspec = conc_host.species_layer_maps(Pm, sub[0], sub[1], sub[2], sub[4], xm, ym, Z_ARRAY, 3)
        res['numpy_species_moll_s'] = round(time.perf_counter() - t0, 3)
        res['numpy_species_moll_over_call'] = round(1e3 * res['numpy_species_moll_s'] * scale / res['species_moll_call_ms'], 1)
        res['numpy_species_moll_over_kernel'] = round(1e3 * res['numpy_species_moll_s'] * scale / res['species_moll_kernel_ms'], 1)
        got = ctx.density_map_proj(P.params, *sub[:4], xs, ys, stranded_code=STRANDED)
        gspec = ctx.species_layer_map(Pm.params, sub[0], sub[1], sub[2], sub[4], xm, ym, Z_ARRAY, 3)
        # entries within rounding of an edge may fall either way (the host mirror and the device differ by 1e-9 m): a handful in 24 M
        res['bins_differing_from_numpy'] = [int((h != w).sum()) for h, w in zip(list(got) + [gspec], list(want) + [wspec])]
        res['entries_differing_from_numpy'] = [float(np.abs(h - w).sum() / 2) for h, w in zip(list(got) + [gspec], list(want) + [wspec])]
        assert max(res['entries_differing_from_numpy']) <= 1e-6 * m * a.times, 'the device maps differ from NumPy'
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
