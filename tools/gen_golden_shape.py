"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c37_shape_landmask.npz from the REFERENCE ITSELF.

The reference's own shape reader (opendrift/readers/reader_shape.py) and its OceanDrift, imported through oracle/refshim.py, answer
everything recorded here.  shapely is not installed and is a mock in the shim; before the reader is imported this generator puts a
small stand-in of its own in its place:
  contains_xy    matplotlib's Path.contains_points per ring, combined as "inside the exterior and inside no hole", OR over polygons
  unary_union    a container of the polygons with .bounds and .buffer (the identity, asked with a distance of 0 only)
  Polygon, MultiPolygon, LineString, MultiLineString   what reader_shape.unwrap walks
so the predicate in the golden file is matplotlib's, independent of this project's crossing rule.

Cases:
  a   12 star-shaped polygons in lon / lat, several overlapping, half with a hole, one island polygon inside a hole; 4 133 queries
      inside and outside the box of the rings.  Recorded: the mask of the reference's get_variables_interpolated, NaN outside.
  b   the rings of (a) mapped to 0 .. 80 x 0 .. 60 and rounded to a 1/4 lattice, queries on a 1/8 lattice.
  c   the rings of (a) in +proj=utm +zone=33 +ellps=WGS84 coordinates, queries given as lon / lat.  (The reference passes the
      projected bounds through lonlat2xy, reader_shape.py:102-104, which leaves it without a usable box: the mask is its _on_land
      at the projected queries and the box of the rings is applied here.)
  d   (a) with invert=True.
  e   get_nearest_outside and closest_ocean_points (land_buffer_distance = 0) for seeds on land and in water.
  f   two OceanDrift runs (stranding with Euler, previous with runge-kutta4), a constant current that drives the elements into the
      coast, the shape reader as the only source of land_binary_mask; after the steps the closing interact_with_coastline(final=True)
      of run().

Conditions asserted here and stored, so that the file cannot hide a failure:
  * in a - d every kept query is farther than 1e-9 (ring units) from every edge; the share of queries dropped for being nearer is
    below 5 %;
  * in f the smallest distance between any position the reader was asked at and any edge (and the box) exceeds 1e-5 deg: candidates
    are run first, the elements that keep the gap are seeded again and the run is repeated and checked;
  * in f at least a quarter of the elements strand / are sent back, at least a quarter never touch land, the reader never fails.

    python tools/gen_golden_shape.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as gg  # noqa: E402  (installs the shim)
from matplotlib.path import Path  # noqa: E402

UTM = '+proj=utm +zone=33 +ellps=WGS84'
LONLAT = '+proj=lonlat +ellps=WGS84'
NQ = 4133


# ---- the stand-in for shapely
class LineString:
    def __init__(self, xy):
        xy = np.asarray(xy, np.float64)
        if not np.array_equal(xy[0], xy[-1]):
            xy = np.vstack([xy, xy[:1]])
        self.coords = xy
        self.xy = (xy[:, 0], xy[:, 1])


class MultiLineString:
    def __init__(self, lines):
        self.geoms = list(lines)


class Polygon:
    def __init__(self, exterior, holes=()):
        self.exterior, self.interiors = LineString(exterior), [LineString(h) for h in holes]
        self.boundary = MultiLineString([self.exterior] + self.interiors) if self.interiors else self.exterior

    def contains(self, x, y):
        pts = np.c_[x, y]
        inside = Path(self.exterior.coords).contains_points(pts)
        for h in self.interiors:
            inside &= ~Path(h.coords).contains_points(pts)
        return inside


class MultiPolygon:
    def __init__(self, polys):
        self.geoms = list(polys)
        xy = np.vstack([p.exterior.coords for p in self.geoms])
        self.bounds = (xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max())

    def buffer(self, distance):
        assert distance == 0, 'the stand-in offsets nothing'
        return self


def _install_shapely():
    m = types.ModuleType('shapely')
    m.LineString, m.MultiLineString, m.Polygon, m.MultiPolygon = LineString, MultiLineString, Polygon, MultiPolygon
    m.unary_union = lambda polys: MultiPolygon(polys)

    def contains_xy(geom, x, y):
        x, y = np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64))
        out = np.zeros(len(x), bool)
        for p in geom.geoms:
            out |= p.contains(x, y)
        return out
    m.contains_xy = contains_xy
    ops = types.ModuleType('shapely.ops')
    ops.unary_union = m.unary_union
    m.ops, m.vectorized = ops, types.ModuleType('shapely.vectorized')
    sys.modules['shapely'], sys.modules['shapely.ops'], sys.modules['shapely.vectorized'] = m, ops, m.vectorized


_install_shapely()
from opendrift.readers import reader_constant  # noqa: E402
from opendrift.readers.reader_shape import Reader  # noqa: E402


# ---- polygons
def polygons_a(seed):
    """[(exterior, [holes])]: star-shaped rings around 12 centres in 4 .. 6 E, 59.5 .. 61 N; the last one an island in a hole."""
    rng = np.random.default_rng(seed)
    centres = np.c_[rng.uniform(4.3, 5.7, 11), rng.uniform(59.8, 60.7, 11)]
    centres[1] = centres[0] + [0.25, 0.1]      # overlapping neighbours
    centres[3] = centres[2] + [-0.2, 0.15]
    centres[5] = centres[4] + [0.1, -0.2]
    out = []
    for k, c in enumerate(centres):
        n = int(rng.integers(12, 60))
        th = np.sort(rng.uniform(0, 2 * np.pi, n))
        if k % 3 == 0:
            th = th[::-1]      # either orientation
        rad = rng.uniform(0.12, 0.38, n)
        ext = np.c_[c[0] + 1.6 * rad * np.cos(th), c[1] + rad * np.sin(th)]
        if k % 4 == 1:
            ext = np.vstack([ext, ext[:1]])      # closed and open rings
        holes = [np.c_[c[0] + 0.55 * 1.6 * rad * np.cos(th), c[1] + 0.55 * rad * np.sin(th)]] if k % 2 == 0 else []
        out.append((ext, holes))
    c = centres[0]      # (has a hole)
    th = np.linspace(0, 2 * np.pi, 9)[:-1]
    out.append((np.c_[c[0] + 0.05 * np.cos(th), c[1] + 0.03 * np.sin(th)], []))
    return out


def mapped(polys, fn):
    return [(fn(e), [fn(h) for h in holes]) for e, holes in polys]


def lattice(xy):
    """0 .. 80 x 0 .. 60 on a 1/4 lattice; vertices that fall together are dropped."""
    q = np.round(np.c_[(xy[:, 0] - 4.0) * 40.0, (xy[:, 1] - 59.5) * 40.0] * 4.0) / 4.0
    keep = np.ones(len(q), bool)
    keep[1:] = (np.diff(q, axis=0) != 0).any(axis=1)
    return q[keep]


def edges_of(polys):
    seg = []
    for e, holes in polys:
        for r in [e] + list(holes):
            r = np.asarray(r)
            seg.append(np.c_[r, np.roll(r, -1, axis=0)])
    return np.vstack(seg)


def edge_distance(seg, x, y, chunk=2048):
    """Smallest distance of each point to any segment."""
    out = np.empty(len(x))
    ax, ay, bx, by = (seg[:, k][None, :] for k in range(4))
    dx, dy = bx - ax, by - ay
    L2 = np.where(dx * dx + dy * dy > 0, dx * dx + dy * dy, 1.0)
    for o in range(0, len(x), chunk):
        px, py = x[o:o + chunk, None], y[o:o + chunk, None]
        t = np.clip(((px - ax) * dx + (py - ay) * dy) / L2, 0.0, 1.0)
        out[o:o + chunk] = np.hypot(px - (ax + t * dx), py - (ay + t * dy)).min(axis=1)
    return out


def reference_reader(polys, proj4=LONLAT, **kw):
    return Reader([Polygon(e, holes) for e, holes in polys], proj4_str=proj4, **kw)


def ring_arrays(prefix, polys):
    rings = [(r, k) for k, (e, holes) in enumerate(polys) for r in [e] + list(holes)]
    return {prefix + '_ring_xy': np.vstack([np.asarray(r, np.float64) for r, _ in rings]),
            prefix + '_ring_n': np.array([len(r) for r, _ in rings], np.int32),
            prefix + '_ring_poly': np.array([k for _, k in rings], np.int32)}


def queries_case(tag, polys, proj4, seed, invert=False, lattice_queries=False, lonlat=None):
    """The reference's mask at NQ queries; returns the dict of arrays and the kept lon / lat."""
    r = reference_reader(polys, proj4, invert=invert)
    seg = edges_of(polys)
    x0, x1, y0, y1 = seg[:, 0].min(), seg[:, 0].max(), seg[:, 1].min(), seg[:, 1].max()
    rng = np.random.default_rng(seed)
    if lonlat is None:
        lon = rng.uniform(x0 - 0.08 * (x1 - x0), x1 + 0.08 * (x1 - x0), NQ)
        lat = rng.uniform(y0 - 0.08 * (y1 - y0), y1 + 0.08 * (y1 - y0), NQ)
        if lattice_queries:
            lon, lat = np.round(lon * 8.0) / 8.0, np.round(lat * 8.0) / 8.0
    else:
        lon, lat = lonlat
    x, y = (lon, lat) if proj4 == LONLAT else [np.asarray(a, np.float64) for a in r.lonlat2xy(lon, lat)]
    d = edge_distance(seg, x, y)
    keep = d > 1e-9
    dropped = 1.0 - keep.mean()
    assert dropped < 0.05, dropped
    lon, lat, x, y = lon[keep], lat[keep], x[keep], y[keep]
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    mask = np.full(len(lon), np.nan, np.float32)
    if proj4 == LONLAT:
        mask[inside] = np.asarray(r.get_variables(['land_binary_mask'], x=x[inside], y=y[inside])['land_binary_mask'], np.float32)
    else:      # (get_variables would refuse every position: its check_arguments tests the box that lonlat2xy made of projected bounds)
        mask[inside] = np.asarray(r._on_land(x[inside], y[inside]), np.float32)
    if proj4 == LONLAT:      # the reference's own coverage test and masking
        assert (r.xmin, r.xmax, r.ymin, r.ymax) == (x0, x1, y0, y1)
        env = r.get_variables_interpolated(['land_binary_mask'], time=gg.T0, lon=lon, lat=lat, z=np.zeros(len(lon)))[0]
        own = np.ma.filled(np.ma.masked_invalid(np.asarray(env['land_binary_mask'], np.float64)), np.nan).astype(np.float32)
        assert np.array_equal(np.isnan(own), np.isnan(mask)) and np.array_equal(own[inside], mask[inside])
    land = np.nansum(mask == 1)
    print(tag, 'kept', keep.sum(), 'of', NQ, 'dropped %.2f %%' % (100 * dropped), 'inside the box', inside.sum(), 'land', land,
          'smallest edge distance', d[keep].min())
    assert 0.1 * inside.sum() < land < 0.9 * inside.sum()
    out = {tag + '_lon': lon, tag + '_lat': lat, tag + '_mask': mask, tag + '_dropped': dropped, tag + '_min_edge_distance': d[keep].min()}
    return out, (lon, lat)


def case_e(polys, seed):
    rng = np.random.default_rng(seed)
    r = reference_reader(polys, land_buffer_distance=0)
    lon = rng.uniform(r.xmin + 0.05, r.xmax - 0.05, 400).astype(np.float32)
    lat = rng.uniform(r.ymin + 0.05, r.ymax - 0.05, 400).astype(np.float32)
    nx, ny, dist = r.get_nearest_outside(lon.astype(np.float64), lat.astype(np.float64), 0)
    # the two nearest vertices must not be tied (a closed ring holds its first vertex twice: the same point either way)
    from scipy.spatial import cKDTree
    d2 = cKDTree(np.unique(r._land_kdtree.data, axis=0)).query(np.c_[lon, lat].astype(np.float64), k=2)[0]
    assert (d2[:, 1] - d2[:, 0]).min() > 1e-9
    o = gg._base('euler')
    o.add_reader(r)
    o.env.finalize()
    lo, la, idx = o.closest_ocean_points(lon.copy(), lat.copy())
    assert lo.dtype == np.float32 and 50 < len(idx) < 350, len(idx)
    print('e: moved', len(idx), 'of', len(lon))
    return dict(e_lon=lon, e_lat=lat, e_nearest_x=nx, e_nearest_y=ny, e_nearest_distance=dist, e_moved_lon=lo, e_moved_lat=la,
                e_land_indices=np.asarray(idx, np.int32))


def model_runs(polys, seed, n_keep=240, n_candidates=600, steps=10, dt=900.0, u=0.9, v=0.35):
    seg = edges_of(polys)
    rng = np.random.default_rng(seed)
    r0 = reference_reader(polys)
    lon = rng.uniform(r0.xmin + 0.1, r0.xmax - 0.35, 4 * n_candidates)
    lat = rng.uniform(r0.ymin + 0.1, r0.ymax - 0.2, 4 * n_candidates)
    water = ~np.asarray(r0.get_variables(['land_binary_mask'], x=lon, y=lat)['land_binary_mask'], bool)
    lon, lat = np.float32(lon[water][:n_candidates]).astype(np.float64), np.float32(lat[water][:n_candidates]).astype(np.float64)
    assert len(lon) == n_candidates

    def run(action, scheme, sel):
        r = reference_reader(polys)
        o = gg._base(scheme)
        gap, touched = np.full(len(sel), np.inf), np.zeros(len(sel), bool)
        covers, on_land = r.covers_positions_xy, r._on_land
        last = {}

        def covers_positions_xy(qx, qy, z=0):
            res = covers(qx, qy, z)
            qx, qy = np.atleast_1d(qx), np.atleast_1d(qy)
            assert len(qx) == len(o.elements.ID), 'a sample that is not of the elements'
            ids = np.asarray(o.elements.ID, int)
            d = edge_distance(seg, np.asarray(qx, np.float64), np.asarray(qy, np.float64))
            d = np.minimum(d, np.minimum(np.minimum(qx - r.xmin, r.xmax - qx), np.minimum(qy - r.ymin, r.ymax - qy)))
            gap[ids] = np.minimum(gap[ids], d)
            last['ids'] = ids[res[0]]
            return res

        def _on_land(x, y):
            m = on_land(x, y)
            touched[last['ids']] |= np.asarray(m, bool)
            return m
        r.covers_positions_xy, r._on_land = covers_positions_xy, _on_land
        o.add_reader(r)
        o.add_reader(reader_constant.Reader({'x_sea_water_velocity': u, 'y_sea_water_velocity': v, 'x_wind': 0.0, 'y_wind': 0.0}))
        o.set_config('general:coastline_action', action)
        o.set_config('general:coastline_approximation_precision', None)      # (its search reads the global landmask, not the reader)
        o.set_config('seed:ocean_only', False)
        o.set_config('drift:stokes_drift', False)
        o.set_config('drift:vertical_advection', False)
        o.set_config('drift:vertical_mixing', False)
        np.random.seed(0)
        o.seed_elements(lon=lon[sel], lat=lat[sel], z=0.0, time=gg.T0, wind_drift_factor=0.0)
        res, _ = gg._run(o, dt, steps)
        o.interact_with_coastline(final=True)      # what run() does behind its loop
        o.remove_deactivated_elements()
        final = np.full((3, len(sel)), np.nan)
        for arr in (o.elements, o.elements_deactivated):
            if len(arr):
                ID = np.atleast_1d(arr.ID).astype(int)
                final[0, ID], final[1, ID], final[2, ID] = arr.lon, arr.lat, np.atleast_1d(arr.status) * np.ones(len(ID))
        assert r.number_of_fails == 0 and not o.env.discarded_readers, 'the reference dropped the reader'
        assert np.isfinite(final).all()
        return res, final, gap, touched, list(o.status_categories)

    everyone = np.arange(n_candidates)
    worst = np.minimum(run('stranding', 'euler', everyone)[2], run('previous', 'runge-kutta4', everyone)[2])
    good = np.flatnonzero(worst > 2e-5)
    print('f: candidates that keep the gap', len(good), 'of', n_candidates)
    if len(good) < n_keep:
        return None
    sel = good[:n_keep]
    out, smallest = {}, np.inf
    for tag, action, scheme in (('stranding', 'stranding', 'euler'), ('previous', 'previous', 'runge-kutta4')):
        res, final, gap, touched, categories = run(action, scheme, sel)
        smallest = min(smallest, gap.min())
        hit = (final[2] != 0) if action == 'stranding' else touched
        print('f', tag, scheme, 'smallest gap', gap.min(), 'deg; hit land', hit.sum(), 'never', (~touched).sum(), 'of', n_keep, categories)
        assert hit.sum() >= n_keep // 4 and (~touched).sum() >= n_keep // 4
        assert np.array_equal(hit, touched)
        out.update({'f_%s_lon0' % tag: res['lon'][0], 'f_%s_lat0' % tag: res['lat'][0], 'f_%s_lon' % tag: final[0], 'f_%s_lat' % tag: final[1],
                    'f_%s_status' % tag: final[2].astype(np.int32), 'f_%s_touched' % tag: touched,
                    'f_%s_categories' % tag: np.array(categories)})
    if not smallest > 1e-5:
        return None
    out.update(f_dt=dt, f_steps=steps, f_u=u, f_v=v, f_smallest_gap_deg=smallest)
    return out


def main():
    a = polygons_a(37)
    out = {}
    out.update(ring_arrays('a', a))
    res, lonlat_a = queries_case('a', a, LONLAT, 371)
    out.update(res)
    b = [(lattice(e), [lattice(h) for h in holes]) for e, holes in a]
    out.update(ring_arrays('b', b))
    out.update(queries_case('b', b, LONLAT, 372, lattice_queries=True)[0])
    proj = reference_reader(a, UTM)

    def to_utm(xy):
        x, y = proj.lonlat2xy(xy[:, 0], xy[:, 1])
        return np.c_[x, y]
    c = mapped(a, to_utm)
    out.update(ring_arrays('c', c))
    out.update(queries_case('c', c, UTM, 373, lonlat=lonlat_a)[0])
    out.update(queries_case('d', a, LONLAT, 374, invert=True)[0])
    out.update(case_e(a, 375))
    runs, seed = None, 376
    while runs is None:
        runs = model_runs(a, seed)
        seed += 1000
    out.update(runs)
    path = os.path.join(gg.GOLD, 'c37_shape_landmask.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes')
    assert size < 400000


if __name__ == '__main__':
    main()
