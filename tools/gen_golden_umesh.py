"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c36_unstructured.npz from the REFERENCE ITSELF.

The reference's own unstructured reader (opendrift/readers/reader_netCDF_CF_unstructured.py on basereader/unstructured.py),
imported through oracle/refshim.py, answers every query recorded here.  No netCDF library is installed, so the instance is made
with object.__new__ and handed what the reader's constructor would have read from a file: x, y, xc, yc, times, the box, proj4, the
variable mapping and a dict-like stand-in for `dataset` whose variables carry .dimensions, .shape and __getitem__; then
UnstructuredReader.__init__ runs and _build_ckdtree_ makes the two trees.  get_variables, the sigma rules, nearest_time, the
coverage test and rotate_vectors are the reference's own code.

Cases:
  a   a UTM 33 mesh of random nodes, one corner refined 100 : 1, faces = the centroids of the nodes' Delaunay triangles; 5 sigma
      layers / 6 levels; 3 hourly time levels; u, v, w on the faces' layers, temperature on the nodes' levels, salinity on the
      nodes' layers (its dimension is declared 'siglev' so that the reference takes its 3-D path).  4 133 query points: inside
      and outside the box, above the surface and below the bottom, at, between, exactly midway between, before and after the
      time levels.  Recorded: the un-rotated values (NaN where the reference gives nothing), the node / face indices, the sigma
      indices, u and v rotated to east / north, the rotation angle.
  b   the same mesh mapped to degrees, +proj=latlong: no rotation.
  c   two runs of the reference's OceanDrift (Euler, runge-kutta4) with the reader of (a) as the only source of the current.

The fields and sigma arrays are formed by tests/umesh_host.py (exact operations only), so the file holds coordinates, queries and
answers but not the arrays.

Conditions asserted here so that the golden cannot hide a failure:
  * every query of (a) and (b) is farther than 1e-3 m (1e-8 deg) from the Voronoi edge of its nearest node and face, i.e. the
    second-nearest distance exceeds the nearest by more than that, and farther than that from the edges of the box;
  * in (c) the smallest gap between the nearest and the second-nearest face distance over EVERY sample of EVERY stage exceeds
    1 m (1000 x the 1e-7 deg position bound the runs are held to): candidates are run first, the elements that keep the gap are
    seeded again and the run is repeated and checked; the smallest gap is stored;
  * the reader never failed in (c), every element moved more than 0.02 deg and stayed inside the mesh's box, and the run spans
    all three time levels.

    python tools/gen_golden_umesh.py
"""
import os
import sys
from datetime import timedelta

import numpy as np
from scipy.spatial import Delaunay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as gg  # noqa: E402  (installs the shim)
import pyproj  # noqa: E402  (the shim's)
from opendrift.readers.basereader.unstructured import UnstructuredReader  # noqa: E402
from opendrift.readers.reader_netCDF_CF_unstructured import Reader  # noqa: E402

import umesh_host as U  # noqa: E402

UTM = '+proj=utm +zone=33 +ellps=WGS84'
NQ = 4133
NAMES = U.FACE_VARIABLES + U.NODE_VARIABLES
# seconds after the first level for the query groups: at a level, between, exactly midway (twice), the last level, before, after
QUERY_SECONDS = (0, 1200, 1800, 5400, 7200, -3600, 10800)


class _Var:
    def __init__(self, a, dims):
        self.a, self.dimensions, self.shape = a, dims, a.shape

    def __getitem__(self, key):
        return self.a[key]


def reference_reader(x, y, xc, yc, proj4, gaps=None):
    """The reference's Reader over the golden mesh.  gaps: a list that receives, per _nearest_face_ call, the gap between the
    nearest and the second-nearest distance of every position."""
    f = U.mesh_fields(len(x), len(xc))
    r = object.__new__(Reader)
    r.name, r.proj4, r.proj = 'c36', proj4, None
    r.x, r.y, r.xc, r.yc = x, y, xc, yc
    r.times = np.array([gg.T0 + timedelta(seconds=U.LEVEL_SECONDS * k) for k in range(U.N_TIMES)])
    r.start_time, r.end_time, r.time_step = r.times[0], r.times[-1], None
    r.xmin, r.xmax, r.ymin, r.ymax = np.min(x), np.max(x), np.min(y), np.max(y)
    short = {'x_sea_water_velocity': 'u', 'y_sea_water_velocity': 'v', 'upward_sea_water_velocity': 'ww',
             'sea_water_temperature': 'temp', 'sea_water_salinity': 'salinity'}
    r.variable_mapping = dict(short)
    r.variables = list(short)
    r.node_variables, r.face_variables = list(U.NODE_VARIABLES), list(U.FACE_VARIABLES)
    ds = {k: _Var(f[k], ('sig', 'pt')) for k in ('siglay', 'siglev', 'siglay_center', 'siglev_center')}
    ds['h'], ds['h_center'] = _Var(f['h'], ('node',)), _Var(f['h_center'], ('nele',))
    for v in U.FACE_VARIABLES:
        ds[short[v]] = _Var(f['face_arrays'][v], ('time', 'siglay', 'nele'))
    for v in U.NODE_VARIABLES:      # ('siglev': the name the reference's node branch asks for, whatever the count)
        ds[short[v]] = _Var(f['node_arrays'][v], ('time', 'siglev', 'node'))
    r.dataset = ds
    UnstructuredReader.__init__(r)
    r.nodes_idx, r.faces_idx = r._build_ckdtree_(x, y), r._build_ckdtree_(xc, yc)
    if gaps is not None:
        inner, covers, last = r._nearest_face_, r.covers_positions_xy, {}

        def covers_positions_xy(qx, qy, z=0):
            res = covers(qx, qy, z)
            last['n'], last['indices'] = len(np.atleast_1d(qx)), res[0]
            return res

        def nearest_face(qx, qy):      # (called with the covered positions of the last covers_positions_xy)
            d = r.faces_idx.query(np.vstack((qx, qy)).T, k=2)[0]
            gap = np.zeros(last['n'])      # a position the reader does not cover counts as no gap at all
            gap[last['indices']] = d[:, 1] - d[:, 0]
            gaps.append(gap)
            return inner(qx, qy)
        r._nearest_face_, r.covers_positions_xy = nearest_face, covers_positions_xy
    return r, f


def mesh(seed):
    x, y = U.graded_points(2000, seed)
    tri = Delaunay(np.c_[x, y]).simplices
    xc, yc = x[tri].sum(axis=1) / 3.0, y[tri].sum(axis=1) / 3.0
    keep = np.random.default_rng(seed + 1).permutation(len(xc))[:3800]      # (face centres need not be ordered in any way)
    return x, y, xc[keep], yc[keep]


def query_points(r, seed, geographic):
    """lon, lat, z, time group of NQ queries that keep 1e-3 m (1e-8 deg) from every decision the reader makes in the plane."""
    rng = np.random.default_rng(seed)
    tol = 1e-8 if geographic else 1e-3
    w, h = r.xmax - r.xmin, r.ymax - r.ymin
    lon, lat = np.empty(0), np.empty(0)
    while len(lon) < NQ:
        n = NQ
        qx = rng.uniform(r.xmin - 0.08 * w, r.xmax + 0.08 * w, n)
        qy = rng.uniform(r.ymin - 0.08 * h, r.ymax + 0.08 * h, n)
        fine = rng.random(n) < 0.25      # a quarter in the refined corner
        qx[fine] = r.xmin + 0.012 * w * rng.random(fine.sum())
        qy[fine] = r.ymin + 0.012 * h * rng.random(fine.sum())
        lo, la = r.xy2lonlat(qx, qy)
        x2, y2 = r.lonlat2xy(r.modulate_longitude(lo), la)      # what the reference will search with
        ok = np.ones(n, bool)
        for tree in (r.nodes_idx, r.faces_idx):
            d = tree.query(np.c_[x2, y2], k=2)[0]
            ok &= d[:, 1] - d[:, 0] > tol
        for q, a, b in ((x2, r.xmin, r.xmax), (y2, r.ymin, r.ymax)):
            ok &= (np.abs(q - a) > tol) & (np.abs(q - b) > tol)
        lon, lat = np.concatenate([lon, lo[ok]]), np.concatenate([lat, la[ok]])
    lon, lat = lon[:NQ], lat[:NQ]
    z = (-rng.uniform(0, 220, NQ)).astype(np.float32)
    z[rng.random(NQ) < 0.05] = np.float32(1.5)       # above the surface
    z[rng.random(NQ) < 0.05] = np.float32(-900.0)    # below every bottom
    z[rng.random(NQ) < 0.05] = np.float32(0.0)
    group = rng.integers(0, len(QUERY_SECONDS), NQ).astype(np.int8)
    return lon, lat, z.astype(np.float64), group


def queries_case(tag, r, f, seed, geographic):
    lon, lat, z, group = query_points(r, seed, geographic)
    latlong = pyproj.Proj('+proj=latlong')
    x, y = r.lonlat2xy(r.modulate_longitude(lon), lat)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = {v: np.full(NQ, np.nan, np.float32) for v in NAMES}
    rot_u, rot_v = np.full(NQ, np.nan, np.float32), np.full(NQ, np.nan, np.float32)
    node, face = np.asarray(r._nearest_node_(x, y), np.int32), np.asarray(r._nearest_face_(x, y), np.int32)
    sig = {k: np.full(NQ, -1, np.int8) for k in ('face_lay', 'node_lev', 'node_lay')}
    inside = (x >= r.xmin) & (x <= r.xmax) & (y >= r.ymin) & (y <= r.ymax)
    for g, sec in enumerate(QUERY_SECONDS):
        m = group == g
        t = gg.T0 + timedelta(seconds=sec)
        try:
            env, _ = r.get_variables_interpolated(list(NAMES), time=t, lon=lon[m], lat=lat[m], z=z[m], rotate_to_proj=None)
            env_r, _ = r.get_variables_interpolated(list(NAMES), time=t, lon=lon[m], lat=lat[m], z=z[m], rotate_to_proj=latlong)
        except Exception as e:
            assert sec < 0 or sec > U.LEVEL_SECONDS * (U.N_TIMES - 1), (sec, e)      # only the times outside may raise
            print(tag, 'group', sec, 's:', type(e).__name__)
            continue
        assert 0 <= sec <= U.LEVEL_SECONDS * (U.N_TIMES - 1)
        for v in NAMES:
            out[v][m] = np.ma.filled(np.ma.masked_invalid(np.asarray(env[v], np.float64)), np.nan).astype(np.float32)
        rot_u[m] = np.ma.filled(np.ma.masked_invalid(np.asarray(env_r['x_sea_water_velocity'], np.float64)), np.nan).astype(np.float32)
        rot_v[m] = np.ma.filled(np.ma.masked_invalid(np.asarray(env_r['y_sea_water_velocity'], np.float64)), np.nan).astype(np.float32)
        k = np.flatnonzero(m & inside)
        sig['face_lay'][k] = r.__nearest_face_sigma__(r.dataset['u'], face[k], z[k])
        sig['node_lev'][k] = r.__nearest_node_sigma__(r.dataset['temp'], node[k], z[k])
        sig['node_lay'][k] = r.__nearest_node_sigma__(r.dataset['salinity'], node[k], z[k])
    covered = np.isfinite(out[NAMES[0]])
    assert (covered <= inside).all() and 0.5 * NQ < covered.sum() < 0.8 * NQ, covered.sum()
    assert (sig['face_lay'][covered] >= 0).all() and len(np.unique(sig['face_lay'][covered])) == U.N_SIGLAY
    assert len(np.unique(sig['node_lev'][covered])) == U.N_SIGLAY + 1
    # rot_angle_rad of rotate_vectors, from the reference: a unit x vector comes back as (cos, sin)
    if geographic:
        rot = np.zeros(NQ)
        assert np.array_equal(rot_u[covered], out['x_sea_water_velocity'][covered])
    else:
        c, s = r.rotate_vectors(x, y, np.ones(NQ), np.zeros(NQ), r.proj, latlong)
        rot = np.arctan2(s, c)
        assert np.abs(rot).max() > 0.01
    print(tag, 'covered', covered.sum(), 'of', NQ, 'rotation', rot.min(), rot.max())
    res = {'lon': lon, 'lat': lat, 'z': z.astype(np.float32), 'group': group, 'x': x, 'y': y, 'node': node, 'face': face,
           'rot': rot, 'rot_u': rot_u, 'rot_v': rot_v, **{'sig_' + k: v for k, v in sig.items()}, **out}
    if geographic:
        for k in ('x', 'y', 'rot', 'rot_u', 'rot_v'):
            res.pop(k)
    return {'%s_%s' % (tag, k): v for k, v in res.items()}


def model_runs(x, y, xc, yc, seed, n_keep=200, n_candidates=320, steps=8, dt=900.0):
    """The two OceanDrift runs; returns None when fewer than n_keep candidates keep the 1 m gap."""
    assert steps * dt >= 2 * U.LEVEL_SECONDS      # the nearest time level changes twice during the run
    rng = np.random.default_rng(seed)
    r0, _ = reference_reader(x, y, xc, yc, UTM)
    # seeded over the western half of the mesh (the current sets east), the refined corner included
    qx = rng.uniform(r0.xmin + 2000.0, r0.xmin + 30000.0, n_candidates)
    qy = rng.uniform(r0.ymin + 8000.0, r0.ymax - 8000.0, n_candidates)
    qx[:40], qy[:40] = r0.xmin + 100.0 + 400.0 * rng.random(40), r0.ymin + 100.0 + 400.0 * rng.random(40)
    lon, lat = r0.xy2lonlat(qx, qy)
    z = -np.round(rng.uniform(0, 60, n_candidates) * 4.0) / 4.0      # (exact in float32, which the reference's elements hold)

    def run(scheme, sel):
        gaps = []
        r, _ = reference_reader(x, y, xc, yc, UTM, gaps=gaps)
        o = gg._base(scheme)
        o.add_reader(r)
        o.set_config('environment:constant:land_binary_mask', 0)
        o.set_config('drift:stokes_drift', False)
        o.set_config('drift:vertical_advection', False)
        o.set_config('drift:vertical_mixing', False)
        np.random.seed(0)
        o.seed_elements(lon=lon[sel], lat=lat[sel], z=z[sel], time=gg.T0, wind_drift_factor=0.0)
        res, _ = gg._run(o, dt, steps)
        assert r.number_of_fails == 0 and not o.env.discarded_readers, 'the reference dropped the reader'
        assert all(len(g) == len(sel) for g in gaps), 'a sample did not cover every element'
        return res, np.min(np.stack(gaps), axis=0), len(gaps)

    everyone = np.arange(n_candidates)
    worst = np.minimum(run('euler', everyone)[1], run('runge-kutta4', everyone)[1])
    good = np.flatnonzero(worst > 1.5)
    print('c: candidates that keep the gap', len(good), 'of', n_candidates)
    if len(good) < n_keep:
        return None
    sel = good[:n_keep]
    out, smallest = {}, np.inf
    for tag, scheme in (('euler', 'euler'), ('rk4', 'runge-kutta4')):
        res, gap, calls = run(scheme, sel)
        smallest = min(smallest, gap.min())
        moved = np.hypot(res['lon'][-1] - res['lon'][0], res['lat'][-1] - res['lat'][0])
        print('c', tag, 'samples per element', calls, 'smallest gap', gap.min(), 'm; moved', moved.min(), '..', moved.max(), 'deg')
        assert moved.min() > 0.02 and (res['status'] == 0).all()
        out.update({'c_%s_%s' % (tag, k): v for k, v in res.items() if k in ('lon', 'lat', 'z')})
    if not smallest > 1.0:
        return None
    out.update(c_dt=dt, c_steps=steps, c_smallest_gap_m=smallest)
    return out


def main():
    x, y, xc, yc = mesh(36)
    out = dict(x=x, y=y, xc=xc, yc=yc, proj4=UTM, n_siglay=U.N_SIGLAY, level_seconds=U.LEVEL_SECONDS, n_times=U.N_TIMES,
               query_seconds=np.array(QUERY_SECONDS), names=np.array(NAMES))
    r, f = reference_reader(x, y, xc, yc, UTM)
    out.update(queries_case('a', r, f, 361, False))
    bx, by = U.latlong_mesh(x, y)
    bxc, byc = U.latlong_mesh(xc, yc)
    rb, fb = reference_reader(bx, by, bxc, byc, '+proj=latlong')
    out.update(queries_case('b', rb, fb, 362, True))
    runs, seed = None, 363
    while runs is None:
        runs = model_runs(x, y, xc, yc, seed)
        seed += 1000
    out.update(runs)
    path = os.path.join(gg.GOLD, 'c36_unstructured.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 1 << 20


if __name__ == '__main__':
    main()
