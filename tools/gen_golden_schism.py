"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c41_schism.npz from the REFERENCE ITSELF.

The reference's own SCHISM reader (opendrift/readers/reader_schism_native.py), imported through oracle/refshim.py, answers every
query recorded here.  No netCDF library is installed, so the instance is made with object.__new__ and handed what the reader's
constructor would have read from a file: x, y, times, the box, proj4, use_3d, the variable mapping and a stand-in for `dataset`
that serves zcor, hvel, dahv, elev, depth and vertical_velocity; then the base class's __init__ runs and the reader's own
_build_ckdtree_ makes reader_KDtree.  get_variables, convert_3d_to_array, the blocks (ReaderBlockUnstruct), nearest_time, the
time weights, the range check and rotate_vectors are the reference's own code: _get_variables_interpolated_ runs unchanged
against the stand-in (none of its pdb.set_trace() paths is reached).

shapely is not installed: `boundary` is an object of this file that answers the hull test (inside every edge of scipy's ConvexHull,
which the reference also builds), so a position ON the hull's edge is NOT pinned by this file; every query keeps 1e-3 m from it.

Cases:
  a   a UTM 33 mesh of 2 000 random nodes in 20 km, one corner refined 100 : 1; 6 levels, depths 20 .. 80 m, zcor moving with a
      time-varying elevation; the shallowest fifth of the nodes has 1 .. 3 levels below the sea bed; 3 hourly time levels; 3-D u, v,
      w, 2-D elevation, static depth.  4 096 queries: inside and outside the hull, above the surface and below the deepest level,
      at, between, exactly midway between, before and after the time levels, a few exactly ON a node.  The reference is asked in
      its own coordinates (get_variables_interpolated_xy) with x, y = lonlat2xy(lon, lat) as get_variables_interpolated forms them,
      except the on-node queries, whose x, y are the node's own.  Recorded: the un-rotated values, u and v rotated to east / north,
      the cosine and sine of that rotation, and per time level the three neighbours and distances of the reference's trees.
      a_stable / a_rot_stable flag the queries whose float32 answers do not hang on the last bits of the projected position
      (and, rotated, of the angle) -- see POSITION_NOISE below: a reader that is handed longitude and latitude is held to the
      golden's bits at those, and to the neighbouring float32 at the few others (at most 10 % of the covered may be flagged).
  b   the same mesh mapped to degrees, +proj=latlong, depth-averaged currents: 2-D only, no rotation.
  c   two runs of the reference's OceanDrift (Euler, runge-kutta4; 12 steps) with the reader of (b) as the only current.
  d   a run of the reference's OceanDrift (Euler, 4 steps, elements at fixed depths) with the 3-D reader of (a).

The fields come from tests/schism_host.py (exact operations only), so the file holds coordinates, queries and answers.

Conditions asserted here so that the golden cannot hide a failure:
  * (a), (b): at every query and each of its time levels, consecutive distances among the four nearest differ by more than 1e-3 m
    in 2-D (1e-8 deg in b) and 1e-6 m in 3-D, and the query is farther than 1e-3 m (1e-8 deg) from the hull's edge; a query that
    fails is drawn again, at most 1 % may be; at least 100 3-D queries have their neighbours in more than one column and at least
    100 touch a column with NaN levels;
  * (c), (d): over EVERY sample of EVERY stage the gap between the third and the fourth nearest distance exceeds 1e-6 deg (c: the
    0.1 m of the mesh in degrees) / 0.05 m (d): candidates are run first, the elements that keep the gap are seeded again and the
    run is repeated and checked; at most 10 % (c) / a third (d) of the candidates are dropped and at least 50 remain; the reader
    never fails, every element moves more than 0.02 deg and stays inside the hull, and the run spans all three time levels.

    python tools/gen_golden_schism.py
"""
import os
import sys
from datetime import timedelta

import numpy as np
from scipy.spatial import ConvexHull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as gg  # noqa: E402  (installs the shim)
import pyproj  # noqa: E402  (the shim's)
from opendrift.readers.basereader.unstructured import UnstructuredReader  # noqa: E402
from opendrift.readers import reader_schism_native as rsn  # noqa: E402

import schism_host as S  # noqa: E402

NQ = 4096
# seconds after the first level for the query groups: at a level, between, exactly midway (twice), the last level, before, after
QUERY_SECONDS = (0, 1200, 1800, 5400, 7200, -3600, 10800)
# What a reader that is handed LONGITUDE and LATITUDE cannot share with the reference: the last bits of the projected position
# and of the rotation's angle.  The UTM series is some twenty float64 operations on a northing of 6.5e6 m, whose unit in the last
# place is 9.3e-10 m: two correct implementations differ by several of those.  The angle the reference forms numerically, as the
# azimuth of a 10 m line between two inverse projections: its OWN value moves by up to 4e-11 rad when the position moves by
# 2e-8 m (the true angle moves by 1e-15; measured below and asserted).  A value is a float32; where it lies within that noise of
# a rounding boundary its LAST BIT is not defined by longitude and latitude.  Such queries stay in the file and are flagged
# (a_stable, a_rot_stable false): the reference is asked again at x, y +- POSITION_NOISE (20 units in the last place) along
# either axis -- the values are locally linear in the position, so no shift within the noise crosses a boundary the four do not
# -- and the rotation is formed again with the angle +- ANGLE_NOISE, more than three times the reference's own scatter.
POSITION_NOISE, ANGLE_NOISE = 2e-8, 1.5e-10
NAMES_A = (S.U_, S.V_, S.W_, S.SSH, S.DEPTH)
NAMES_B = (S.U_, S.V_, S.SSH, S.DEPTH)


class _Var:
    def __init__(self, a):
        self.a, self.shape, self.ndim, self.attrs = a, a.shape, a.ndim, {}

    def __getitem__(self, key):
        return self.a[key]


class _Dataset:
    def __init__(self, variables):
        self.variables = variables


class Hull:
    """The hull test the reference leaves to shapely: inside every edge of the counter-clockwise ring."""

    def __init__(self, x, y):
        ring = ConvexHull(np.vstack((x, y)).T).vertices
        self.x, self.y = x[ring], y[ring]

    def signed_distances(self, qx, qy):
        """[n, edges]: distance to the line of every edge, positive inside."""
        x2, y2 = np.roll(self.x, -1), np.roll(self.y, -1)
        ex, ey = x2 - self.x, y2 - self.y
        return (ex[None, :] * (qy[:, None] - self.y[None, :]) - ey[None, :] * (qx[:, None] - self.x[None, :])) / np.hypot(ex, ey)[None, :]

    def contains(self, qx, qy):
        qx, qy = np.atleast_1d(np.asarray(qx, np.float64)), np.atleast_1d(np.asarray(qy, np.float64))
        return (self.signed_distances(qx, qy) > 0).all(axis=1)

    def edge_distance(self, qx, qy):
        return np.abs(self.signed_distances(qx, qy)).min(axis=1)


sys.modules['shapely.vectorized'].contains = lambda boundary, x, y: boundary.contains(x, y)


def reference_reader(x, y, proj4, three_d, log=None):
    """The reference's Reader over the golden mesh.  log: a list that receives, per ReaderBlockUnstruct.interpolate call, a dict
    with the block's time, the positions and the four nearest of the reference's 2-D and (if any) 3-D tree."""
    f = S.mesh_fields(len(x))
    r = object.__new__(rsn.Reader)
    r.name, r.proj4, r.proj = 'c41', proj4, None
    r.interpolation, r.convolve, r.return_block = 'linearNDFast', None, True
    r.x, r.y = x, y
    r.times = S.times()
    r.start_time, r.end_time, r.time_step = r.times[0], r.times[-1], r.times[1] - r.times[0]
    r.xmin, r.xmax, r.ymin, r.ymax = np.min(x), np.max(x), np.min(y), np.max(y)
    r.use_3d = three_d
    ds = {'elev': _Var(f['elev']), 'depth': _Var(f['depth'])}
    r.variable_mapping = {S.SSH: 'elev', S.DEPTH: 'depth'}
    if three_d:
        r.nb_levels = S.N_LEVELS
        ds.update(zcor=_Var(f['zcor']), hvel=_Var(np.stack((f['u'], f['v']), axis=-1)), vertical_velocity=_Var(f['w']))
        r.variable_mapping.update({S.U_: 'hvel', S.V_: 'hvel', S.W_: 'vertical_velocity'})
    else:
        ds.update(dahv=_Var(np.stack((f['du'], f['dv']), axis=-1)))
        r.variable_mapping.update({S.U_: 'dahv', S.V_: 'dahv'})
    r.dataset = _Dataset(ds)
    r.variables = list(r.variable_mapping)
    UnstructuredReader.__init__(r)
    r.reader_KDtree = r._build_ckdtree_(x, y)
    r.boundary = Hull(x, y)
    r.var_block_before, r.var_block_after = {}, {}
    if log is not None:
        r._log = log
    return r, f


_interpolate = rsn.ReaderBlockUnstruct.interpolate


def _recording_interpolate(self, x, y, z=None, variables=None, profiles=[], profiles_depth=None):
    log = getattr(_recording_interpolate, 'log', None)
    if log is not None:
        rec = dict(time=self.time, x=np.array(x), y=np.array(y), z=np.array(z), covered=dict(getattr(_recording_interpolate, 'last', {})))
        rec['d2'], rec['i2'] = self.block_KDtree.query(np.vstack((x, y)).T, 4)
        if hasattr(self, 'z_3d'):
            rec['d3'], rec['i3'] = self.block_KDtree_3d.query(np.vstack((x, y, z)).T, 4)
            rec['columns'] = self.x_3d, self.y_3d
        log.append(rec)
    return _interpolate(self, x, y, z, variables, profiles, profiles_depth)


rsn.ReaderBlockUnstruct.interpolate = _recording_interpolate


def draw_queries(r, hull, rng, n, geographic):
    w, h = r.xmax - r.xmin, r.ymax - r.ymin
    qx = rng.uniform(r.xmin - 0.08 * w, r.xmax + 0.08 * w, n)
    qy = rng.uniform(r.ymin - 0.08 * h, r.ymax + 0.08 * h, n)
    fine = rng.random(n) < 0.25      # a quarter in the refined corner
    qx[fine] = r.xmin + 0.012 * w * rng.random(fine.sum())
    qy[fine] = r.ymin + 0.012 * h * rng.random(fine.sum())
    lon, lat = r.xy2lonlat(qx, qy)
    x, y = r.lonlat2xy(r.modulate_longitude(lon), lat)      # what get_variables_interpolated searches with
    z = (-rng.uniform(0, 85, n)).astype(np.float32)
    z[rng.random(n) < 0.05] = np.float32(1.5)       # above the surface
    z[rng.random(n) < 0.05] = np.float32(-900.0)    # below every bottom
    z[rng.random(n) < 0.05] = np.float32(0.0)
    group = rng.integers(0, len(QUERY_SECONDS), n).astype(np.int8)
    return np.asarray(lon, np.float64), np.asarray(lat, np.float64), np.asarray(x, np.float64), np.asarray(y, np.float64), z.astype(np.float64), group


def queries_case(tag, r, f, seed, geographic, names):
    rng = np.random.default_rng(seed)
    hull = r.boundary
    tol2, tol3 = (1e-8, None) if geographic else (1e-3, 1e-6)
    lon, lat, x, y, z, group = draw_queries(r, hull, rng, NQ, geographic)
    on_node = rng.permutation(len(r.x))[:16]      # exactly ON a node (the 1e-10 floor): interior nodes, their own coordinates
    on_node = on_node[hull.edge_distance(r.x[on_node], r.y[on_node]) > 10 * tol2][:12]
    x[:len(on_node)], y[:len(on_node)] = r.x[on_node], r.y[on_node]
    lon[:len(on_node)], lat[:len(on_node)] = r.xy2lonlat(x[:len(on_node)], y[:len(on_node)])
    three_d = bool(r.use_3d)
    latlong = pyproj.Proj('+proj=latlong')
    redrawn = 0
    while True:      # the conditions, per query and per time level it touches; a query that fails is drawn again
        bad = hull.edge_distance(x, y) <= tol2
        d = r.reader_KDtree.query(np.vstack((x, y)).T, 4)[0]
        bad |= (np.diff(d, axis=1) <= tol2).any(axis=1)
        if three_d:
            for g, sec in enumerate(QUERY_SECONDS):
                if not 0 <= sec <= S.LEVEL_SECONDS * (S.N_TIMES - 1):
                    continue
                m = group == g
                t = gg.T0 + timedelta(seconds=sec)
                for k in set(r.nearest_time(t)[4:6]):
                    cx, cy, cz = S.cloud(r.x, r.y, f['zcor'][k])
                    d3 = rsn.cKDTree(np.vstack((cx, cy, cz)).T).query(np.vstack((x[m], y[m], z[m])).T, 4)[0]
                    bad[np.flatnonzero(m)[(np.diff(d3, axis=1) <= tol3).any(axis=1)]] = True
        k = np.flatnonzero(bad)
        if not len(k):
            break
        assert not (k < len(on_node)).any(), 'an on-node query fails the conditions'
        redrawn += len(k)
        lon[k], lat[k], x[k], y[k], z[k], group[k] = draw_queries(r, hull, rng, len(k), geographic)
    assert redrawn <= 0.01 * NQ, redrawn
    out = {v: np.full(NQ, np.nan, np.float32) for v in names}
    rot_u, rot_v = np.full(NQ, np.nan, np.float32), np.full(NQ, np.nan, np.float32)
    nb = {k: np.full((NQ, 3), -1, np.int64) for k in ('i2', 'i3b', 'i3a')}
    nb.update({k: np.full((NQ, 3), np.nan) for k in ('d2', 'd3b', 'd3a')})
    inside = hull.contains(x, y)
    weights = np.full(len(QUERY_SECONDS), np.nan)
    many_columns = nan_columns = 0
    stable, rot_stable, scatter = np.ones(NQ, bool), np.ones(NQ, bool), 0.0
    for g, sec in enumerate(QUERY_SECONDS):
        m = group == g
        t = gg.T0 + timedelta(seconds=sec)
        log = []
        _recording_interpolate.log = log
        try:
            env, _ = r.get_variables_interpolated_xy(list(names), time=t, x=x[m], y=y[m], z=z[m], rotate_to_proj=None)
            calls = list(log)
            env_r, _ = r.get_variables_interpolated_xy(list(names), time=t, x=x[m], y=y[m], z=z[m], rotate_to_proj=latlong)
        except Exception as e:
            assert sec < 0 or sec > S.LEVEL_SECONDS * (S.N_TIMES - 1), (sec, repr(e))      # only the times outside may raise
            print(tag, 'group', sec, 's:', type(e).__name__)
            continue
        finally:
            _recording_interpolate.log = None
        assert 0 <= sec <= S.LEVEL_SECONDS * (S.N_TIMES - 1)
        _, tb, ta, _, _, _ = r.nearest_time(t)
        blend = t != tb
        assert len(calls) == (2 if blend else 1) and calls[0]['time'] == tb and (not blend or calls[1]['time'] == ta)
        weights[g] = (t - tb).total_seconds() / (ta - tb).total_seconds() if blend else 0.0
        k = np.flatnonzero(m & inside)
        assert len(k) == len(calls[0]['x'])
        for v in names:
            out[v][m] = np.ma.filled(np.ma.masked_invalid(np.asarray(env[v], np.float64)), np.nan).astype(np.float32)
        rot_u[m] = np.ma.filled(np.ma.masked_invalid(np.asarray(env_r[S.U_], np.float64)), np.nan).astype(np.float32)
        rot_v[m] = np.ma.filled(np.ma.masked_invalid(np.asarray(env_r[S.V_], np.float64)), np.nan).astype(np.float32)
        nb['i2'][k], nb['d2'][k] = calls[0]['i2'][:, :3], calls[0]['d2'][:, :3]
        if three_d:
            for c, key in zip(calls, ('b', 'a')):
                nb['i3' + key][k], nb['d3' + key][k] = c['i3'][:, :3], c['d3'][:, :3]
                cx, cy = c['columns']
                i3 = c['i3'][:, :3]
                many_columns += int(((cx[i3] != cx[i3][:, :1]) | (cy[i3] != cy[i3][:, :1])).any(axis=1).sum())
            dry = np.isnan(f['zcor'][0]).any(axis=1)
            nan_columns += int(dry[calls[0]['i2'][:, :3]].any(axis=1).sum())
        if geographic:      # (longitude and latitude ARE the coordinates: every reader of the file searches at the same bits)
            continue
        # which answers do not hang on the last bits of a projection or of the rotation's angle (see the module's docstring)
        fill = lambda a: np.ma.filled(np.ma.masked_invalid(np.asarray(a, np.float64)), np.nan)
        same = lambda a, b32: (fill(a).astype(np.float32) == b32) | (np.isnan(fill(a)) & np.isnan(b32))
        ok, ok_r = np.ones(int(m.sum()), bool), np.ones(int(m.sum()), bool)
        for dx, dy in ((POSITION_NOISE, 0.0), (-POSITION_NOISE, 0.0), (0.0, POSITION_NOISE), (0.0, -POSITION_NOISE)):
            e2, _ = r.get_variables_interpolated_xy(list(names), time=t, x=x[m] + dx, y=y[m] + dy, z=z[m], rotate_to_proj=None)
            e3, _ = r.get_variables_interpolated_xy(list(names), time=t, x=x[m] + dx, y=y[m] + dy, z=z[m], rotate_to_proj=latlong)
            for v in names:
                ok &= same(e2[v], out[v][m])
            ok_r &= same(e3[S.U_], rot_u[m]) & same(e3[S.V_], rot_v[m])
        # the rotation itself, from the components as the reference held them there (float64; a blended value is a float32 in it)
        uu, vv = fill(env[S.U_]), fill(env[S.V_])
        c0, s0 = r.rotate_vectors(x[m], y[m], np.ones(int(m.sum())), np.zeros(int(m.sum())), r.proj, latlong)
        assert same(uu * c0 - vv * s0, rot_u[m]).all() and same(uu * s0 + vv * c0, rot_v[m]).all()
        c2, s2 = r.rotate_vectors(x[m] + POSITION_NOISE, y[m], np.ones(int(m.sum())), np.zeros(int(m.sum())), r.proj, latlong)
        scatter = max(scatter, float(np.abs(np.arctan2(s2, c2) - np.arctan2(s0, c0)).max()))
        for da in (ANGLE_NOISE, -ANGLE_NOISE):
            c1, s1 = c0 * np.cos(da) - s0 * np.sin(da), s0 * np.cos(da) + c0 * np.sin(da)
            ok_r &= same(uu * c1 - vv * s1, rot_u[m]) & same(uu * s1 + vv * c1, rot_v[m])
        stable[m], rot_stable[m] = ok, ok_r
    covered = np.isfinite(out[S.DEPTH])
    if not geographic:
        loose, loose_r = int((covered & ~stable).sum()), int((covered & ~rot_stable).sum())
        print(tag, 'covered queries whose answers hang on the last bits of the position:', loose, '; of position or angle, rotated:', loose_r)
        print(tag, 'scatter of the reference\'s own rotation angle under a shift of %g m: %.2g rad' % (POSITION_NOISE, scatter))
        assert 0 < 3 * scatter <= ANGLE_NOISE
        assert loose <= 0.10 * covered.sum() and loose_r <= 0.10 * covered.sum(), (loose, loose_r)
    assert (covered <= inside).all() and 0.5 * NQ < covered.sum() < 0.8 * NQ, covered.sum()
    if three_d:
        assert many_columns >= 100 and nan_columns >= 100, (many_columns, nan_columns)
    if geographic:
        cs, sn = np.ones(NQ), np.zeros(NQ)
        assert np.array_equal(rot_u[covered], out[S.U_][covered])
    else:      # the cosine and sine rotate_vectors uses: a unit x vector comes back as (cos, sin)
        cs, sn = r.rotate_vectors(x, y, np.ones(NQ), np.zeros(NQ), r.proj, latlong)
        assert np.abs(np.arctan2(sn, cs)).max() > 0.01
    print(tag, 'covered', covered.sum(), 'of', NQ, 'redrawn', redrawn, 'neighbours in several columns', many_columns,
          'touching a column with NaN levels', nan_columns)
    res = {'lon': lon, 'lat': lat, 'z': z.astype(np.float32), 'group': group, 'x': x, 'y': y, 'cs': cs, 'sn': sn, 'rot_u': rot_u,
           'rot_v': rot_v, 'w': weights, 'n_on_node': len(on_node), 'stable': stable, 'rot_stable': rot_stable, **nb, **out}
    if geographic:
        for k in ('cs', 'sn', 'rot_u', 'rot_v', 'i3b', 'd3b', 'i3a', 'd3a', 'stable', 'rot_stable'):
            res.pop(k)
    return {'%s_%s' % (tag, k): v for k, v in res.items()}


def model_runs(tag, x, y, proj4, three_d, schemes, steps, dt, gap, max_dropped, seed, n_candidates=240):
    """OceanDrift runs of the reference with the mesh reader as the only current; None when too few candidates keep the gap."""
    assert steps * dt >= 2 * S.LEVEL_SECONDS      # the run spans all three time levels
    rng = np.random.default_rng(seed)
    r0, _ = reference_reader(x, y, proj4, three_d)
    w, h = r0.xmax - r0.xmin, r0.ymax - r0.ymin
    # seeded over the western part of the mesh (the current sets east), the refined corner's surroundings included
    qx = rng.uniform(r0.xmin + 0.06 * w, r0.xmin + 0.45 * w, n_candidates)
    qy = rng.uniform(r0.ymin + 0.2 * h, r0.ymax - 0.2 * h, n_candidates)
    qx[:30], qy[:30] = r0.xmin + w * (0.02 + 0.02 * rng.random(30)), r0.ymin + h * (0.10 + 0.08 * rng.random(30))
    lon, lat = r0.xy2lonlat(qx, qy)
    z = -np.round(rng.uniform(1, 70, n_candidates) * 4.0) / 4.0 if three_d else np.zeros(n_candidates)      # (exact in float32)

    def run(scheme, sel, final=False):
        log = []
        r, _ = reference_reader(x, y, proj4, three_d)
        o = gg._base(scheme)
        o.add_reader(r)
        o.set_config('environment:constant:land_binary_mask', 0)
        o.set_config('drift:stokes_drift', False)
        o.set_config('drift:vertical_advection', False)
        o.set_config('drift:vertical_mixing', False)
        np.random.seed(0)
        o.seed_elements(lon=lon[sel], lat=lat[sel], z=z[sel], time=gg.T0, wind_drift_factor=0.0)
        covers, last = r.covers_positions_xy, {}

        def covers_positions_xy(qx, qy, z=0):      # (interpolate is called with the covered positions of the last call of this)
            res = covers(qx, qy, z)
            last['n'], last['indices'] = len(np.atleast_1d(qx)), res[0]
            return res
        r.covers_positions_xy = covers_positions_xy
        _recording_interpolate.log, _recording_interpolate.last = log, last
        try:
            res, _ = gg._run(o, dt, steps)
        finally:
            _recording_interpolate.log, _recording_interpolate.last = None, {}
        assert r.number_of_fails == 0 and not o.env.discarded_readers, 'the reference dropped the reader'
        assert not final or all(len(c['x']) == len(sel) for c in log), 'a sample did not cover every element: one left the hull'
        gaps = np.zeros((len(log), len(sel)))      # an element the reader does not cover counts as no gap at all
        for j, c in enumerate(log):
            d = c['d3'] if three_d else c['d2']
            gaps[j, c['covered']['indices']] = d[:, 3] - d[:, 2]
        assert {c['time'] for c in log} == set(r.times), 'the run does not span all three time levels'
        return res, gaps.min(axis=0), len(log)

    everyone = np.arange(n_candidates)
    worst = np.min([run(s, everyone)[1] for s in schemes], axis=0)
    good = np.flatnonzero(worst > 1.5 * gap)
    print(tag, 'candidates that keep the gap', len(good), 'of', n_candidates)
    assert n_candidates - len(good) <= max_dropped * n_candidates, 'too many candidates dropped: coarsen the mesh'
    assert len(good) >= 50
    sel = good[:160]
    out, smallest = {}, np.inf
    for scheme in schemes:
        key = {'euler': 'euler', 'runge-kutta4': 'rk4'}[scheme]
        res, g, calls = run(scheme, sel, final=True)
        smallest = min(smallest, g.min())
        moved = np.hypot(res['lon'][-1] - res['lon'][0], res['lat'][-1] - res['lat'][0])
        print(tag, key, 'interpolate calls', calls, 'smallest gap', g.min(), '; moved', moved.min(), '..', moved.max(), 'deg')
        assert moved.min() > 0.02 and (res['status'] == 0).all()
        out.update({'%s_%s_%s' % (tag, key, k): v for k, v in res.items() if k in ('lon', 'lat', 'z', 'status')})
    if not smallest > gap:
        return None
    out.update({tag + '_dt': dt, tag + '_steps': steps, tag + '_smallest_gap': smallest})
    return out


def main():
    x, y = S.mesh_xy()
    out = dict(x=x, y=y, proj4=S.UTM, n_levels=S.N_LEVELS, level_seconds=S.LEVEL_SECONDS, n_times=S.N_TIMES,
               query_seconds=np.array(QUERY_SECONDS), names_a=np.array(NAMES_A), names_b=np.array(NAMES_B))
    r, f = reference_reader(x, y, S.UTM, True)
    out.update(queries_case('a', r, f, 411, False, NAMES_A))
    bx, by = S.latlong_mesh(x, y)
    rb, fb = reference_reader(bx, by, '+proj=latlong', False)
    out.update(queries_case('b', rb, fb, 412, True, NAMES_B))
    for tag, args in (('c', (bx, by, '+proj=latlong', False, ('euler', 'runge-kutta4'), 12, 600.0, 1e-6, 0.10)),
                      ('d', (x, y, S.UTM, True, ('euler',), 4, 1800.0, 0.05, 1.0 / 3.0))):
        runs, seed = None, 413
        while runs is None:
            runs = model_runs(tag, *args, seed)
            seed += 1000
        out.update(runs)
    path = os.path.join(gg.GOLD, 'c41_schism.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 1 << 20


if __name__ == '__main__':
    main()
