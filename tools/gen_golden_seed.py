"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c35_seed_geometry.npz from the REFERENCE ITSELF.

The reference's own OpenDriftSimulation.points_within_polygon and seed_cone (opendrift/models/basemodel/__init__.py:1487-1558,
:1240-1353), imported through oracle/refshim.py, are called here; matplotlib supplies the real Polygon and Path.  pyproj is not
installed and the shim has neither +proj=aea nor Geod.npts, so this tool patches two stand-ins into the reference's module:

  Proj   for the one string the reference builds, '+proj=aea +lat_1= +lat_2= +lat_0= +lon_0= +R=6370997.0 +units=m +ellps=WGS84'.
         PROJ lets +R overrule +ellps (ell_set.cpp: "Specifying R overrules everything"): the SPHERICAL Albers, Snyder 14-1 ..
         14-11, evaluated with mpmath at 40 digits and rounded to float64.  The inverse hands lam0 + theta / n out as it is.
  Geod   the shim's, plus npts(lon1, lat1, lon2, lat2, n): the n points at i * s12 / (n + 1), i = 1 .. n, by the shim's inv and
         fwd (the oracle's geodesic.c).

The grid points, their inside flags and the grid size are RECORDED from the reference's own calls (the arrays it hands to
proj(..., inverse=True), what Path.contains_points returns), so the reference alone decides every mask and grid size.  seed_cone
runs on a stand-in `self` that records what reaches seed_elements.

Conditions asserted here so that the golden cannot hide a failure:
  (a) every grid point of every case lies at least 1e-9 deg from every ring edge;
  (b) the fractional parts of (xmax - xmin) / deltax and (ymax - ymin) / deltax lie in [0.01, 0.99];
  (c) the truncate, duplicate, border and centre branches are each taken by at least one case;
  (d) the file is under 1 MiB.

    python tools/gen_golden_seed.py
"""
import os
import sys
from datetime import datetime, timedelta

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from opendrift.models.basemodel import Mode, OpenDriftSimulation  # noqa: E402
import opendrift.models.basemodel as _basemodel  # noqa: E402
from matplotlib.path import Path  # noqa: E402

from seed_host import star_ring  # noqa: E402

mp.mp.dps = 40
EPOCH = datetime(2020, 1, 1)
RECORD = {}      # what the reference's last points_within_polygon call handed to the stand-ins


class _AlbersProj:
    def __init__(self, srs):
        p = refshim._parse_proj4(srs)
        assert p.get('proj') == 'aea' and 'R' in p, srs
        rad = lambda key: mp.mpf(float(p[key])) * mp.pi / 180
        self.R = mp.mpf(float(p['R']))
        phi1, phi2, phi0, self.lam0 = rad('lat_1'), rad('lat_2'), rad('lat_0'), rad('lon_0')
        self.n = (mp.sin(phi1) + mp.sin(phi2)) / 2
        assert abs(self.n) >= 1e-10
        self.C = mp.cos(phi1) ** 2 + 2 * self.n * mp.sin(phi1)
        self.rho0 = self.R * mp.sqrt(self.C - 2 * self.n * mp.sin(phi0)) / self.n

    def _forward(self, lon, lat):
        lam, phi = mp.mpf(float(lon)) * mp.pi / 180, mp.mpf(float(lat)) * mp.pi / 180
        dl = lam - self.lam0
        dl -= 2 * mp.pi * mp.floor((dl + mp.pi) / (2 * mp.pi))      # into [-pi, pi)
        rho = self.R * mp.sqrt(self.C - 2 * self.n * mp.sin(phi)) / self.n
        theta = self.n * dl
        return float(rho * mp.sin(theta)), float(self.rho0 - rho * mp.cos(theta))

    def _inverse(self, x, y):
        x, y = mp.mpf(float(x)), self.rho0 - mp.mpf(float(y))
        sgn = mp.sign(self.n)
        rho = sgn * mp.hypot(x, y)
        theta = mp.atan2(sgn * x, sgn * y)
        v = (self.C - (rho * self.n / self.R) ** 2) / (2 * self.n)
        phi = mp.asin(v) if abs(v) <= 1 else mp.sign(v) * mp.pi / 2
        return float((self.lam0 + theta / self.n) * 180 / mp.pi), float(phi * 180 / mp.pi)

    def __call__(self, a, b, inverse=False):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        f = self._inverse if inverse else self._forward
        out = np.array([f(u, v) for u, v in zip(a.ravel(), b.ravel())], np.float64).reshape(-1, 2)
        u, v = out[:, 0].reshape(a.shape), out[:, 1].reshape(a.shape)
        if inverse:
            RECORD['grid_shape'], RECORD['grid_lon'], RECORD['grid_lat'] = a.shape, u.ravel().copy(), v.ravel().copy()
        else:
            RECORD['ring_x'], RECORD['ring_y'] = u.copy(), v.copy()
        return u, v


class _RecordingPath(Path):
    def contains_points(self, points, *a, **kw):
        ind = Path.contains_points(self, points, *a, **kw)
        RECORD['ind'] = np.array(ind, bool)
        RECORD['ring'] = np.array(self.vertices, np.float64)
        return ind


class _NptsGeod(refshim.Geod):
    def npts(self, lon1, lat1, lon2, lat2, npts, radians=False, **kw):
        assert not radians
        az, _, s12 = self.inv(float(lon1), float(lat1), float(lon2), float(lat2))
        dist = np.arange(1, npts + 1) * (s12 / (npts + 1))
        lo, la, _ = self.fwd(np.full(npts, float(lon1)), np.full(npts, float(lat1)), np.full(npts, az), dist)
        return list(zip(np.asarray(lo).tolist(), np.asarray(la).tolist()))


_basemodel.pyproj.Proj = _AlbersProj
_basemodel.pyproj.Geod = _NptsGeod
_basemodel.Path = _RecordingPath


class _ConeStandIn:
    """`self` of seed_cone: the mode its decorator asks for, a configuration, and a seed_elements that records its arguments"""
    def __init__(self):
        self.mode, self.seed_geojson, self.seeded = Mode.Ready, [], None

    def get_config(self, key):
        assert key == 'seed:number'
        return 100

    def get_configspec(self, prefix):
        return {}

    def seed_elements(self, **kw):
        self.seeded = kw


def segment_distance(px, py, ring):
    """the smallest distance [deg] from every point to every edge of the closed ring"""
    ax, ay = ring[:-1, 0][None, :], ring[:-1, 1][None, :]
    bx, by = ring[1:, 0][None, :], ring[1:, 1][None, :]
    dx, dy = bx - ax, by - ay
    ll = dx * dx + dy * dy
    t = np.clip(((px[:, None] - ax) * dx + (py[:, None] - ay) * dy) / np.where(ll > 0, ll, 1.0), 0, 1)
    return np.hypot(px[:, None] - (ax + t * dx), py[:, None] - (ay + t * dy)).min()


def polygon_case(name, lons, lats, number, data, branches):
    RECORD.clear()
    lons, lats = np.asarray(lons, np.float64), np.asarray(lats, np.float64)
    lon, lat = OpenDriftSimulation.points_within_polygon(lons, lats, number)
    ny, nx = RECORD['grid_shape']
    ind = RECORD['ind']
    x, y = RECORD['ring_x'], RECORD['ring_y']
    area = 0.0
    for i in range(-1, len(x) - 1):
        area += x[i] * (y[i + 1] - y[i - 1])
    deltax = np.sqrt(abs(area) / 2 / number)
    frac = [np.ptp(x) / deltax % 1.0, np.ptp(y) / deltax % 1.0]
    assert all(0.01 <= f <= 0.99 for f in frac), (name, frac)                       # (b)
    assert (nx, ny) == (int(np.ptp(x) / deltax), int(np.ptp(y) / deltax))
    gap = segment_distance(RECORD['grid_lon'], RECORD['grid_lat'], RECORD['ring']) if ind.size else np.inf
    assert gap >= 1e-9, (name, gap)                                                 # (a)
    L = int(ind.sum())
    branch = 'centre' if ind.size == 0 else 'border' if L == 0 else 'truncate' if L > number else 'duplicate' if L < number else 'exact'
    branches.add(branch)
    assert lon.shape == lat.shape == (number, ) and lon.dtype == np.float64
    print('%-12s number %5d  grid %3d x %3d  inside %5d  %-9s frac %.3f %.3f  nearest edge %.1e deg'
          % (name, number, nx, ny, L, branch, frac[0], frac[1], gap))
    data.update({name + '_lons': lons, name + '_lats': lats, name + '_number': number, name + '_lon': lon, name + '_lat': lat,
                 name + '_mask': ind.reshape(ny, nx), name + '_nx': nx, name + '_ny': ny, name + '_n_inside': L, name + '_branch': branch})
    return nx, ny, L, branch


def cone_case(name, lon, lat, radius, number, hours, data):
    o = _ConeStandIn()
    time = [EPOCH, EPOCH + timedelta(hours=hours)] if hours else EPOCH
    OpenDriftSimulation.seed_cone(o, lon=lon, lat=lat, time=time, radius=radius, number=number)
    kw = o.seeded
    assert kw['radius'].dtype == np.float32 and kw['number'] == number
    data.update({'cone_%s_ends' % name: np.ravel(np.c_[np.atleast_1d(lon), np.atleast_1d(lat)]).astype(np.float64),
                 'cone_%s_radius_in' % name: np.atleast_1d(radius).astype(np.float64), 'cone_%s_number' % name: number,
                 'cone_%s_hours' % name: float(hours),
                 'cone_%s_lon' % name: np.asarray(kw['lon'], np.float64), 'cone_%s_lat' % name: np.asarray(kw['lat'], np.float64),
                 'cone_%s_radius' % name: kw['radius'],
                 'cone_%s_time' % name: np.array([(t - EPOCH).total_seconds() for t in np.atleast_1d(kw['time'])], np.float64)})
    print('cone %-8s number %4d  lon %.6f .. %.6f  lat %.6f .. %.6f  radius %g .. %g' % (
        name, number, kw['lon'][0], kw['lon'][-1], kw['lat'][0], kw['lat'][-1], kw['radius'][0], kw['radius'][-1]))
    return kw


WKT_RING = [(7.784889, 64.353442), (7.777561, 64.353842), (7.774236, 64.354707), (7.770215, 64.355829), (7.774269, 64.356015),
            (7.776829, 64.356863), (7.779107, 64.3578), (7.782827, 64.358355), (7.786346, 64.359615), (7.787109, 64.361975),
            (7.790125, 64.361132), (7.794584, 64.359908), (7.798455, 64.359624), (7.797258, 64.358193), (7.79978, 64.356904),
            (7.795957, 64.356494), (7.792955, 64.355335), (7.789134, 64.355339), (7.784889, 64.353442)]      # test_seed_wkt's ring


def main():
    data, branches, names = {}, set(), []

    def poly(name, lons, lats, number):
        names.append(name)
        return polygon_case(name, lons, lats, number, data, branches)

    sq = ([2, 3, 3, 2], [60, 60, 61, 61])
    assert poly('square_10', *sq, 10)[:3] == (2, 4, 8)
    assert poly('square_1000', *sq, 1000)[:3] == (22, 45, 990)
    w = np.array(WKT_RING)
    assert poly('wkt_100', w[:, 0], w[:, 1], 100)[:3] == (18, 12, 94)
    s65 = star_ring(65, 4.5, 60.2, 0.3, 65)
    for number in (64, 257, 4097):
        poly('star65_%d' % number, *s65, number)
    poly('star1025_1000', *star_ring(1025, -150.0, -33.0, 2.0, 1025), 1000)
    poly('seam_500', [179.5, 180.4, 180.3, 179.7], [10, 10.2, 11, 10.9], 500)
    # sliver: a triangle 60 km long and 2 km wide across its box, which its 8 x 7 grid of three elements' spacing misses altogether
    assert poly('sliver_3', [5.0, 5.78, 5.5522], [59.0, 59.35, 59.284], 3)[3] == 'border'
    assert poly('tiny_square_1', *sq, 1)[3] == 'centre'
    assert poly('tiny_tri_2', [10.0, 10.5, 10.1], [-20.0, -19.99, -19.95], 2)[3] == 'centre'
    assert {'truncate', 'duplicate', 'border', 'centre'} <= branches, branches      # (c)
    data['poly_names'] = np.array(names)

    kw = cone_case('run', [4.4, 4.5], [60.5, 60.6], 0, 100, 3, data)
    assert round(kw['lon'][50], 2) == 4.45      # the reference's own test_seed_cone (tests/models/test_run.py)
    kw = cone_case('seam', [176.5, -177.0], [-15.0, -10.0], [100.0, 20000.0], 500, 12, data)
    assert np.abs(np.diff(kw['lon'])).max() > 300 and 850e3 < _NptsGeod().inv(176.5, -15.0, -177.0, -10.0)[2] < 950e3
    kw = cone_case('point', 4.7, 60.1, [0.0, 5000.0], 50, 6, data)
    assert (np.asarray(kw['lon']) == 4.7).all() and kw['radius'][-1] == 5000
    data['cone_names'] = np.array(['run', 'seam', 'point'])

    path = os.path.join(ROOT, 'tests', 'golden', 'c35_seed_geometry.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20                                          # (d)


if __name__ == '__main__':
    main()
