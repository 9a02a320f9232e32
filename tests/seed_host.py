"""TEST INFRASTRUCTURE: ctypes access to the seeding geometry of opendrift_amd/csrc/odr_seed.hip.h compiled for the host (g++
-ffp-contract=off, tests/hostshim in place of the HIP runtime header), see seed_host.cpp; the NumPy restatement of matplotlib's
crossing rule; the point sets and rings the tests share; and HostContext, which stands in for the model's device context."""
import ctypes as C

import numpy as np

from host_build import host_lib

_dp, _bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)

# Bounds: 4 x the host build's measured maximum over every case of tests/golden/c35_seed_geometry.npz.
# Measured: |lon - golden| 2.85e-14 deg (one ulp of 180), |lat - golden| 7.64e-14 deg (the seam case at 10 N, where the inverse's
# sin(lat) = (C - (rho n / R)^2) / (2 n) is a difference of two numbers near 1 over 2 n = 0.36).  The golden's Albers is a 40-digit
# evaluation rounded to float64.
C35_LON_BOUND_DEG = 4 * 2.85e-14
C35_LAT_BOUND_DEG = 4 * 7.64e-14


def _lib():
    return host_lib('seed_host', ('odr_seed.hip.h', 'odr_geodinv.hip.h', 'odr_geodesic.hip.h'))


def points_in_polygon(x, y, vx, vy):
    """The signature of opendrift_amd.device.Context.points_in_polygon, computed by the host build of the header."""
    x, y, vx, vy = (np.ascontiguousarray(a, np.float64).ravel() for a in (x, y, vx, vy))
    inside = np.zeros(len(x), np.uint8)
    _lib().seedh_points_in_polygon(C.c_longlong(len(x)), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), C.c_int(len(vx)),
                                  vx.ctypes.data_as(_dp), vy.ctypes.data_as(_dp), inside.ctypes.data_as(_bp))
    return inside.astype(bool)


def points_within_polygon(lons, lats, number, info=False, mask=False):
    """The signature of opendrift_amd.device.Context.points_within_polygon, computed by the host build of the header; mask=True
    adds info['mask']: the inside flag of every grid point, [ny, nx]."""
    lons, lats = (np.ascontiguousarray(a, np.float64).ravel() for a in (lons, lats))
    if len(lons) != len(lats):
        raise ValueError('lon and lat arrays must have same length.')
    number = int(number)
    lon, lat = np.empty(max(number, 0)), np.empty(max(number, 0))
    n_inside, nx, ny = C.c_longlong(), C.c_int(), C.c_int()

    def call(m):
        rc = _lib().seedh_polygon_points(C.c_int(len(lons)), lons.ctypes.data_as(_dp), lats.ctypes.data_as(_dp), C.c_longlong(number),
                                        lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp), C.byref(n_inside), C.byref(nx), C.byref(ny),
                                        None if m is None else m.ctypes.data_as(_bp))
        if rc:
            raise ValueError('points_within_polygon: invalid polygon or number')
    call(None)
    out = dict(n_inside=n_inside.value, nx=nx.value, ny=ny.value)
    if mask:
        out['mask'] = np.zeros((ny.value, nx.value), np.uint8)
        call(out['mask'])
        out['mask'] = out['mask'].astype(bool)
    return (lon, lat, out) if info or mask else (lon, lat)


def albers(lat1, lat2, lat0, lon0, a, b, forward=True):
    a, b = (np.ascontiguousarray(v, np.float64).ravel() for v in (a, b))
    u, v = np.empty(len(a)), np.empty(len(a))
    rc = _lib().seedh_albers(C.c_double(lat1), C.c_double(lat2), C.c_double(lat0), C.c_double(lon0), C.c_longlong(len(a)),
                            a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), u.ctypes.data_as(_dp), v.ctypes.data_as(_dp), C.c_int(int(forward)))
    if rc:
        raise ValueError('no Albers cone')
    return u, v


def crossing_rule(tx, ty, vx, vy):
    """matplotlib's point_in_path restated in NumPy float64 (no contraction): what Path(V).contains_points gives."""
    tx, ty = np.asarray(tx, np.float64), np.asarray(ty, np.float64)
    inside = np.zeros(tx.shape, bool)
    m = len(vx)
    x0, y0 = vx[0], vy[0]
    yflag0 = y0 >= ty
    for k in list(range(1, m)) + [0]:
        x1, y1 = vx[k], vy[k]
        yflag1 = y1 >= ty
        inside ^= (yflag0 != yflag1) & ((((y1 - ty) * (x0 - x1)) >= ((x1 - tx) * (y0 - y1))) == yflag1)
        yflag0, x0, y0 = yflag1, x1, y1
    return inside


def star_ring(m, lon0, lat0, radius_deg, seed):
    """A star-shaped ring of m vertices about (lon0, lat0): sorted angles, radii 0.35 .. 1.0 of radius_deg.  Not closed."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, m))
    r = radius_deg * rng.uniform(0.35, 1.0, m)
    return lon0 + r * np.cos(ang) / np.cos(np.radians(lat0)), lat0 + r * np.sin(ang)


def probe_points(vx, vy, nrandom, seed):
    """Random points over the ring's box and a margin, every vertex, every edge midpoint, and points that share a vertex's x or y."""
    rng = np.random.default_rng(seed)
    w, h = np.ptp(vx), np.ptp(vy)
    x = rng.uniform(vx.min() - 0.1 * w, vx.max() + 0.1 * w, nrandom)
    y = rng.uniform(vy.min() - 0.1 * h, vy.max() + 0.1 * h, nrandom)
    mx, my = 0.5 * (vx + np.roll(vx, -1)), 0.5 * (vy + np.roll(vy, -1))
    k = rng.integers(0, len(vx), 4 * len(vx))
    sx = np.concatenate([vx[k[::2]], rng.uniform(vx.min(), vx.max(), len(k[1::2]))])
    sy = np.concatenate([rng.uniform(vy.min(), vy.max(), len(k[::2])), vy[k[1::2]]])
    return np.concatenate([x, vx, mx, sx]), np.concatenate([y, vy, my, sy])


class HostContext:
    """Stands in for the model's device context in the CPU tests: the polygon placement by the host build; the cone's centre
    line, whose direct solve exists on the device alone, from the recorded points of the golden file."""

    def __init__(self, golden=None):
        self.golden, self.calls = golden, []

    def points_within_polygon(self, lons, lats, number, info=False):
        self.calls.append(('points_within_polygon', int(number)))
        return points_within_polygon(lons, lats, number, info=info)

    def geod_npts(self, lon1, lat1, lon2, lat2, npts):
        self.calls.append(('geod_npts', int(npts)))
        g = self.golden
        for name in [] if g is None else [str(n) for n in g['cone_names']]:
            ends = g['cone_%s_ends' % name]
            if len(ends) == 4 and np.array_equal(ends, [lon1, lat1, lon2, lat2]) and len(g['cone_%s_lon' % name]) == npts:
                return g['cone_%s_lon' % name].copy(), g['cone_%s_lat' % name].copy()
        # a line the golden does not hold: linear in lon / lat (enough for counts and dispatch, never compared with the reference)
        f = np.arange(1, npts + 1) / (npts + 1.0)
        return lon1 + f * (lon2 - lon1), lat1 + f * (lat2 - lat1)
