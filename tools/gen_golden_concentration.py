"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c3x_concentration.npz from the REFERENCE ITSELF.

The reference's own OpenDriftSimulation.get_density_array_proj (opendrift/models/basemodel/__init__.py:4148-4245) and
RadionuclideDrift.get_radionuclide_density_array / horizontal_smooth (opendrift/models/radionuclides.py:1425-1492, :1518-1551),
imported through oracle/refshim.py, are called UNBOUND on a stand-in `self`: a `result` whose entries have `.values` and `.T`
([trajectory, time] float32 arrays), a `result.time` of datetimes, `get_property`, `nspecies` and `status_categories`.  density_proj
is always handed in as the shim's Proj of a kind it has (laea, polar stere, utm, merc) or left None for get_density_array_proj (the
shim has no Mollweide, so the radionuclide default is never asked for).

300 trajectories, 6 output times.  Population `nan`: the plume of tools/gen_golden_density.py with NaN before the release of half the
elements; population `full`: the same without NaN.  Every entry has a species 0 .. 2 and a depth drawn over five layers, some z
exactly on a layer bound, at -10000 (the open lower bound) and above 0.

Cases (prefix of the stored arrays; every case stores pixelsize_m, proj4, its corners if any, x_array, y_array, lon_array, lat_array):
  laea        get_density_array_proj, Lambert azimuthal equal-area, corners given, population nan: H, H_submerged, H_stranded
  laea_nostr  the same without a 'stranded' category
  laea_wint   weight = small-integer float32     laea_wreal  weight = real-valued float32
  laea_single the fourth output time alone
  utm         get_density_array_proj, UTM zone 31, no corners, population full
  default     get_density_array_proj, density_proj=None (longlat: pixelsize_m in degrees), no corners, population full
  quad        get_density_array_proj, polar stereographic about 70 E: the plume and the whole grid lie where x < 0 and y < 0, so
              (outsidex, outsidey) = 1.5 * the maxima is INSIDE the grid and the reference counts the removed entries there
  quad_wreal  the same with real weights
  rn          get_radionuclide_density_array, Mercator, corners given, population nan: H [time, species, layer, x, y]
  rn_full     get_radionuclide_density_array, laea, no corners, population full
  rn_single   the fourth output time alone
and horizontal_smooth of a plane of rn's H (summed over species and layers, so that it holds values above 1) for n = 0, 1, 3 and 60.

Conditions asserted here so that equality can be exact and nothing hides (the seed is re-drawn until they hold):
  (a) no finite entry projects within 1e-6 m (1e-11 degrees for longlat) of an edge of its case -- but for the entries that are the
      minimum of x or y in a case without corners: the reference's second edge is (min - pixelsize_m) + pixelsize_m, that minimum up
      to rounding, so the tests compare those cases with the first two bins of either axis merged;
  (b) surface, submerged, stranded and NaN each hold at least 5 % of the entries of population nan, every species and every layer at
      least 5 %, and some z is on a bound, -10000, above 0;
  (c) the x and y bin counts of every case differ;
  (d) some bin of every case's H holds at least 3;
  (e) the moved-entry bin of the quad case exists and is non-empty in all three maps;
  (f) the file is under 1 MiB.

    python tools/gen_golden_concentration.py
"""
import os
import sys
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
import pyproj  # noqa: E402  (the shim)
from opendrift.models.basemodel import OpenDriftSimulation  # noqa: E402
from opendrift.models.radionuclides import RadionuclideDrift  # noqa: E402

NTRAJ, NT = 300, 6
CATEGORIES = ['active', 'missing_data', 'stranded']
STRANDED = CATEGORIES.index('stranded')
NSPECIES = 3
Z_ARRAY = np.array([-10000.0, -100.0, -30.0, -10.0, -2.0, 0.0])      # five layers; every bound is a float32
LAEA = '+proj=laea +lat_0=60 +lon_0=5 +ellps=WGS84'
UTM = '+proj=utm +zone=31 +ellps=WGS84'
MERC = '+proj=merc +lat_ts=60 +ellps=WGS84'
QUAD = '+proj=stere +lat_0=90 +lon_0=70 +lat_ts=60 +ellps=WGS84'


class _TolerantProj(refshim.Proj):
    """get_density_array_proj constructs a Mollweide Proj that its next line replaces (:4171-4172); the shim has no Mollweide, so
    that one object is made without arithmetic.  It is never called."""
    def __init__(self, projparams=None, **kwargs):
        if '+proj=moll' in str(projparams):
            self.srs = str(projparams)
            return
        super().__init__(projparams, **kwargs)


pyproj.Proj = _TolerantProj


class _Var:
    def __init__(self, values):
        self.values = values

    @property
    def T(self):
        return self.values.T


class _Result(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


class _StandIn:
    def __init__(self, arrays, categories=CATEGORIES):
        nt = next(iter(arrays.values())).shape[1]
        self.result = _Result({k: _Var(v) for k, v in arrays.items()})
        self.result['time'] = [datetime(2024, 1, 1) + timedelta(hours=k) for k in range(nt)]
        self.status_categories = list(categories)
        self.nspecies = NSPECIES
        self._arrays = arrays

    def get_property(self, name):
        return self._arrays[name].T, None


def population(seed, with_nan):
    rng = np.random.default_rng(seed)
    shape = (NTRAJ, NT)
    core = rng.uniform(size=NTRAJ) < 0.5
    lon0 = np.where(core, rng.normal(4.9, 0.012, NTRAJ), rng.normal(4.9, 0.09, NTRAJ))
    lat0 = np.where(core, rng.normal(60.1, 0.006, NTRAJ), rng.normal(60.1, 0.03, NTRAJ))
    steps = np.arange(NT)[None, :]
    lon = lon0[:, None] + 0.004 * steps + rng.normal(0, 0.002, shape)
    lat = lat0[:, None] + 0.002 * steps + rng.normal(0, 0.001, shape)
    layer = rng.integers(0, len(Z_ARRAY) - 1, shape)
    lo, hi = np.maximum(Z_ARRAY[layer], -300.0), Z_ARRAY[layer + 1]
    z = lo + (hi - lo) * rng.uniform(0.05, 0.95, shape)
    u = rng.uniform(size=shape)
    z[u < 0.06] = Z_ARRAY[rng.integers(1, len(Z_ARRAY) - 1, shape)][u < 0.06]      # exactly on an inner bound
    z[(u >= 0.06) & (u < 0.08)] = -10000.0                                          # the open lower bound: no layer
    z[(u >= 0.08) & (u < 0.10)] = 0.5                                               # above the surface: no layer
    z[(u >= 0.10) & (u < 0.30)] = 0.0                                               # the closed upper bound
    z[(u >= 0.30) & (u < 0.33)] = -0.0
    status = np.zeros(shape)
    strand_at = np.where(rng.uniform(size=NTRAJ) < 0.28, rng.integers(1, NT, NTRAJ), NT)
    stranded = steps >= strand_at[:, None]
    status[stranded] = STRANDED
    z[stranded] = 0.0
    specie = rng.integers(0, NSPECIES, shape).astype(np.float64)
    wint = rng.integers(1, 10, shape).astype(np.float64)
    wreal = rng.uniform(0.05, 3.0, shape) * 10.0 ** rng.integers(-3, 4, shape)
    out = dict(lon=lon, lat=lat, z=z, status=status, specie=specie, mass_int=wint, mass=wreal)
    if with_nan:
        release = np.where(rng.uniform(size=NTRAJ) < 0.5, rng.integers(1, NT - 1, NTRAJ), 0)      # NaN before the release
        late = steps < release[:, None]
        odd = (rng.uniform(size=shape) < 0.01) & ~late & ~stranded      # a NaN z at a finite position
        z[odd] = np.nan
        for v in out.values():
            v[late] = np.nan
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def corners_for(proj4, pop, margin, far=None):
    """lon / lat corners whose projection is `margin` (x, y) metres outside the plume (far: the lower-left corner in metres)"""
    P = pyproj.Proj(proj4)
    ok = np.isfinite(pop['lon'])
    x, y = P(pop['lon'][ok].astype(np.float64), pop['lat'][ok].astype(np.float64))
    ll = far if far is not None else (x.min() - margin[0], y.min() - margin[1])
    ur = (x.max() + margin[0], y.max() + margin[1])
    a, b = P(ll[0], ll[1], inverse=True)
    c, d = P(ur[0], ur[1], inverse=True)
    return dict(llcrnrlon=a, llcrnrlat=b, urcrnrlon=c, urcrnrlat=d)


def edge_distance(proj4, pop, x_array, y_array, from_extremes):
    """The smallest distance of a finite projected entry from an edge.  from_extremes (no corners): the entries that ARE the minimum
    of x or of y are left out of that axis -- the reference's second edge is (min - pixelsize_m) + pixelsize_m, the minimum itself up
    to rounding, so which of the first two bins such an entry falls in is decided by the last bit (the tests merge those two)."""
    if proj4 is None:
        x, y = pop['lon'].astype(np.float64), pop['lat'].astype(np.float64)
    else:
        x, y = pyproj.Proj(proj4)(pop['lon'].astype(np.float64), pop['lat'].astype(np.float64))
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = x[ok], y[ok]
    if from_extremes:
        x, y = x[x != x.min()], y[y != y.min()]
    return min(np.abs(x[:, None] - x_array[None, :]).min(), np.abs(y[:, None] - y_array[None, :]).min())


def main():
    for seed in range(40, 80):
        bad = []
        data = dict(seed=seed, stranded_code=STRANDED, z_array=Z_ARRAY, nspecies=NSPECIES)
        pops = dict(nan=population(seed, True), full=population(seed + 1000, False))
        for tag, pop in pops.items():
            data.update({'%s_%s' % (tag, k): v for k, v in pop.items()})
        pn = pops['nan']
        z, status, lon = pn['z'], pn['status'], pn['lon']
        share = dict(nan=np.isnan(lon).mean(), stranded=(status == STRANDED).mean(),
                     surface=(np.isfinite(lon) & (z >= 0) & (status != STRANDED)).mean(), submerged=(z < 0).mean())
        share.update({'species%d' % k: (pn['specie'] == k).mean() for k in range(NSPECIES)})
        share.update({'layer%d' % k: ((z > Z_ARRAY[k]) & (z <= Z_ARRAY[k + 1])).mean() for k in range(len(Z_ARRAY) - 1)})
        bad += ['(b) %s %.3f' % kv for kv in share.items() if kv[1] < 0.05]
        if not ((z == -10000).any() and (z > 0).any() and np.isin(z, Z_ARRAY[1:-1]).any() and (np.isnan(z) & np.isfinite(lon)).any()):
            bad.append('(b) special z')

        def density_case(name, pop, proj4, pixel, corners=None, weight=None, categories=CATEGORIES, tol=1e-6):
            o = _StandIn(pop, categories)
            kw = dict(corners or {})
            if proj4 is not None:
                kw['density_proj'] = pyproj.Proj(proj4)
            out = OpenDriftSimulation.get_density_array_proj(o, pixel, weight=weight, **kw)
            H, Hsub, Hstr, lon_array, lat_array = out
            P = pyproj.Proj(proj4 or '+proj=longlat +a=6371229 +no_defs')
            kw.pop('density_proj', None)
            ax, ay = _corner_xy(o, P, pixel, kw)
            x_array, y_array = np.arange(*ax), np.arange(*ay)
            x0, _ = P(lon_array[:, 0].copy(), lat_array[:, 0].copy())      # the returned grid is the inverse projection of these edges
            _, y1 = P(lon_array[0, :].copy(), lat_array[0, :].copy())
            assert H.shape[1:] == (len(x_array) - 1, len(y_array) - 1) and np.allclose(x0, x_array, atol=1e-3) and np.allclose(y1, y_array, atol=1e-3)
            d = edge_distance(proj4, pop, x_array, y_array, not corners)
            if d < tol:
                bad.append('(a) %s %.3g' % (name, d))
            if len(x_array) == len(y_array):
                bad.append('(c) %s' % name)
            if weight is None and H.max() < 3:
                bad.append('(d) %s' % name)
            print('%-12s %3d x %3d bins, sums %g %g %g, largest %g, nearest edge %.3g' % (name, len(x_array) - 1, len(y_array) - 1, np.nansum(H),
                                                                                         np.nansum(Hsub), np.nansum(Hstr), np.nanmax(H), d))
            data.update({name + '_H': H, name + '_H_submerged': Hsub, name + '_H_stranded': Hstr, name + '_x_array': x_array,
                         name + '_y_array': y_array, name + '_lon_array': lon_array, name + '_lat_array': lat_array,
                         name + '_pixelsize_m': pixel, name + '_proj4': proj4 or ''})
            for k, v in (corners or {}).items():
                data['%s_%s' % (name, k)] = v
            return out, x_array, y_array

        def _corner_xy(o, P, pixel, kw):
            """the reference's arange arguments, restated (:4176-4184)"""
            if 'llcrnrlon' in kw:
                llx, lly = P(kw['llcrnrlon'], kw['llcrnrlat'])
                urx, ury = P(kw['urcrnrlon'], kw['urcrnrlat'])
            else:
                x, y = P(o.result.lon.values.T.copy(), o.result.lat.values.T.copy())
                llx, lly, urx, ury = x.min() - pixel, y.min() - pixel, x.max() + pixel, y.max() + pixel
            return (llx, urx, pixel), (lly, ury, pixel)

        c_laea = corners_for(LAEA, pn, (2300.0, 1700.0))
        density_case('laea', pn, LAEA, 1000.0, c_laea)
        out = density_case('laea_nostr', pn, LAEA, 1000.0, c_laea, categories=CATEGORIES[:2])[0]
        assert not out[2].any()
        density_case('laea_wint', pn, LAEA, 1000.0, c_laea, weight='mass_int')
        density_case('laea_wreal', pn, LAEA, 1000.0, c_laea, weight='mass')
        t = 3
        data['single_time_index'] = t
        single = {k: np.ascontiguousarray(v[:, t:t + 1]) for k, v in pn.items()}
        density_case('laea_single', single, LAEA, 1000.0, c_laea)
        density_case('utm', pops['full'], UTM, 1000.0)
        density_case('default', pops['full'], None, 0.01, tol=1e-11)
        # the south-west quadrant of a polar stereographic plane: the lower-left corner far enough out for 1.5 * the maxima
        P = pyproj.Proj(QUAD)
        ok = np.isfinite(pn['lon'])
        qx, qy = P(pn['lon'][ok].astype(np.float64), pn['lat'][ok].astype(np.float64))
        assert qx.max() < -30000 and qy.max() < -30000
        far = (1.5 * (qx.max() + 30000.0) - 95000.0, 1.5 * (qy.max() + 20000.0) - 65000.0)
        c_quad = corners_for(QUAD, pn, (30000.0, 20000.0), far=far)
        for name, weight in (('quad', None), ('quad_wreal', 'mass')):
            (H, Hsub, Hstr, _, _), x_array, y_array = density_case(name, pn, QUAD, 20000.0, c_quad, weight=weight)
            ox, oy = max(x_array) * 1.5, max(y_array) * 1.5
            if not (x_array[0] <= ox <= x_array[-1] and y_array[0] <= oy <= y_array[-1]):
                bad.append('(e) %s: the point is outside' % name)
                continue
            ix, iy = np.searchsorted(x_array, ox, side='right') - 1, np.searchsorted(y_array, oy, side='right') - 1
            data[name + '_outside_bin'] = np.array([ix, iy])
            if weight is None and not (H[:, ix, iy].min() > 0 and Hsub[:, ix, iy].min() > 0 and Hstr[:, ix, iy].min() > 0):
                bad.append('(e) %s: empty' % name)
            if weight is not None and not np.isnan(Hstr[:, ix, iy]).any():      # (a NaN weight of a removed entry shows there)
                bad.append('(e) %s: no NaN' % name)
            print('             moved-entry bin (%d, %d): %s %s %s' % (ix, iy, H[:, ix, iy], Hsub[:, ix, iy], Hstr[:, ix, iy]))

        def rn_case(name, pop, proj4, pixel, corners=None):
            o = _StandIn(pop)
            P = pyproj.Proj(proj4)
            kw = dict(corners or {})
            H, lon_array, lat_array = RadionuclideDrift.get_radionuclide_density_array(o, pixel, Z_ARRAY, density_proj=P, **kw)
            (ax, ay) = _corner_xy(o, P, pixel, kw)
            x_array, y_array = np.arange(*ax), np.arange(*ay)
            assert H.shape == (pop['lon'].shape[1], NSPECIES, len(Z_ARRAY) - 1, len(x_array) - 1, len(y_array) - 1)
            d = edge_distance(proj4, pop, x_array, y_array, not corners)
            if d < 1e-6:
                bad.append('(a) %s %.3g' % (name, d))
            if len(x_array) == len(y_array):
                bad.append('(c) %s' % name)
            if H.sum(axis=(1, 2)).max() < 3:
                bad.append('(d) %s' % name)
            print('%-12s %3d x %3d bins, sum %g, per species %s, per layer %s, nearest edge %.3g'
                  % (name, len(x_array) - 1, len(y_array) - 1, H.sum(), H.sum(axis=(0, 2, 3, 4)), H.sum(axis=(0, 1, 3, 4)), d))
            data.update({name + '_H': H, name + '_x_array': x_array, name + '_y_array': y_array, name + '_lon_array': lon_array,
                         name + '_lat_array': lat_array, name + '_pixelsize_m': pixel, name + '_proj4': proj4})
            for k, v in (corners or {}).items():
                data['%s_%s' % (name, k)] = v
            return H

        c_merc = corners_for(MERC, pn, (1900.0, 2600.0))
        H = rn_case('rn', pn, MERC, 1000.0, c_merc)
        rn_case('rn_full', pops['full'], LAEA, 1000.0)
        rn_case('rn_single', single, MERC, 1000.0, c_merc)
        plane = H[4].sum(axis=(0, 1))
        assert plane.max() >= 3 and plane.shape[0] != plane.shape[1]
        data['smooth_in'] = plane
        for n in (0, 1, 3, 60):
            s = RadionuclideDrift.horizontal_smooth(None, plane, n=n)
            assert s.dtype == np.float64 and s.shape == plane.shape
            data['smooth_n%d' % n] = s
        print('seed %d: %s' % (seed, bad or 'all conditions hold'))
        if not bad:
            break
    else:
        raise AssertionError('no seed satisfies the conditions')
    path = os.path.join(ROOT, 'tests', 'golden', 'c3x_concentration.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
