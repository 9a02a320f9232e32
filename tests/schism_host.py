"""TEST INFRASTRUCTURE: ctypes access to the arithmetic of opendrift_amd/csrc/odr_schism.hip.h compiled for the host (g++
-ffp-contract=off, tests/hostshim in place of the HIP runtime header), see schism_host.cpp; a brute-force three-nearest search; and
the mesh, fields and reader of tests/golden/c41_schism.npz, which the generator (tools/gen_golden_schism.py) and the tests form
alike with additions, multiplications, divisions and integer arithmetic only."""
import ctypes as C
import os
from datetime import datetime, timedelta

import numpy as np

from host_build import host_lib
from umesh_host import _unit, graded_points, same_bits, ulp32  # noqa: F401  (shared with the tests)

_dp, _fp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_fpp = C.POINTER(_fp)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c41_schism.npz')


def _lib():
    lib = host_lib('schism_host', ('odr_schism.hip.h', 'odr_umesh.hip.h', 'odr_shape.hip.h'))
    lib.sch_build.restype = C.c_void_p
    return lib


def _d(a):
    return np.ascontiguousarray(a, np.float64).ravel()


def _f(a):
    return np.ascontiguousarray(a, np.float32)


class HostMesh:
    """The search index of the header over the nodes (x, y), and the grid over the ring of their hull if one is given."""

    def __init__(self, x, y, hull_x=None, hull_y=None):
        self.x, self.y = _d(x), _d(y)
        self.n = len(self.x)
        hx, hy = (_d([]), _d([])) if hull_x is None else (_d(hull_x), _d(hull_y))
        h = _lib().sch_build(C.c_int(self.n), self.x.ctypes.data_as(_dp), self.y.ctypes.data_as(_dp), C.c_int(len(hx)),
                             hx.ctypes.data_as(_dp), hy.ctypes.data_as(_dp))
        assert h, 'the hull grid could not be built'
        self.h = C.c_void_p(h)

    def __del__(self):
        try:
            _lib().sch_free(self.h)
        except Exception:
            pass

    def nearest3(self, qx, qy, qz=None, zcor=None, visits=False):
        """(idx [n, 3] int64, dist [n, 3]); zcor [N, L]: the 3-D search.  visits=True: also the tree nodes visited per query."""
        qx, qy = _d(qx), _d(qy)
        idx, dist, seen = np.empty((len(qx), 3), np.int64), np.empty((len(qx), 3)), np.empty(len(qx), np.int32)
        if zcor is not None:
            zcor, qz = _f(zcor), _d(qz)
            assert zcor.shape[0] == self.n and len(qz) == len(qx)
        _lib().sch_nearest3(self.h, zcor.ctypes.data_as(_fp) if zcor is not None else None, C.c_int(zcor.shape[1] if zcor is not None else 0),
                            C.c_longlong(len(qx)), qx.ctypes.data_as(_dp), qy.ctypes.data_as(_dp),
                            qz.ctypes.data_as(_dp) if zcor is not None else None, idx.ctypes.data_as(_lp), dist.ctypes.data_as(_dp),
                            seen.ctypes.data_as(_ip))
        return (idx, dist, seen) if visits else (idx, dist)

    def covers(self, qx, qy):
        qx, qy = _d(qx), _d(qy)
        out = np.empty(len(qx), np.int32)
        _lib().sch_covers(self.h, C.c_longlong(len(qx)), qx.ctypes.data_as(_dp), qy.ctypes.data_as(_dp), out.ctypes.data_as(_ip))
        return out.astype(bool)

    def sample(self, x, y, z, before, after=None, w=0.0, zb=None, za=None, cs=None, sn=None, first=True, out=None):
        """One variable (before / after: a plane [N] or [N, L]) or a vector pair (lists of two planes) at the elements: the merged
        float32 values (a list for a pair).  after None: the level `before` alone."""
        pair = isinstance(before, (list, tuple))
        b = [_f(p) for p in (before if pair else [before])]
        a = b if after is None else [_f(p) for p in (after if pair else [after])]
        nv, levels = len(b), (b[0].shape[1] if b[0].ndim == 2 else 0)
        x, y, z = _d(x), _d(y), _d(z)
        n = len(x)
        outs = [np.full(n, np.nan, np.float32) for _ in range(nv)] if out is None else [np.array(o, np.float32) for o in (out if pair else [out])]
        zb = None if zb is None else _f(zb)
        za = zb if za is None else _f(za)
        arr = lambda ps: (_fp * nv)(*[p.ctypes.data_as(_fp) for p in ps])
        rot = cs is not None
        cs, sn = (_d(cs), _d(sn)) if rot else (None, None)
        _lib().sch_sample(self.h, C.c_longlong(n), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), z.ctypes.data_as(_dp), C.c_int(levels),
                          zb.ctypes.data_as(_fp) if levels else None, za.ctypes.data_as(_fp) if levels else None,
                          C.c_int(0 if after is None else 1), C.c_double(w), C.c_int(nv), arr(b), arr(a),
                          cs.ctypes.data_as(_dp) if rot else None, sn.ctypes.data_as(_dp) if rot else None, C.c_int(int(first)), arr(outs))
        return outs if pair else outs[0]


def brute3(px, py, pz, qx, qy, qz, chunk=256):
    """(idx, dist) of the three nearest of the points (px, py[, pz]) by NumPy's float64 (dx*dx + dy*dy) + dz*dz over ALL points;
    ties in ascending index (a stable sort)."""
    idx, dist = np.empty((len(qx), 3), np.int64), np.empty((len(qx), 3))
    for o in range(0, len(qx), chunk):
        s = slice(o, o + chunk)
        dx, dy = px[None, :] - qx[s, None], py[None, :] - qy[s, None]
        d2 = dx * dx + dy * dy
        if pz is not None:
            dz = pz[None, :] - qz[s, None]
            d2 = d2 + dz * dz
        k = np.argsort(d2, axis=1, kind='stable')[:, :3]
        idx[s], dist[s] = k, np.sqrt(np.take_along_axis(d2, k, axis=1))
    return idx, dist


def cloud(x, y, zcor):
    """(x_3d, y_3d, z_3d) as the reference flattens them: [N, L] row-major with the NaN entries removed; z promoted to float64."""
    keep = ~np.isnan(zcor)
    L = zcor.shape[1]
    return np.repeat(x, L).reshape(zcor.shape)[keep], np.repeat(y, L).reshape(zcor.shape)[keep], zcor[keep].astype(np.float64)


# ---- the mesh of tests/golden/c41_schism.npz: the file holds the node coordinates, the queries and the answers
N_LEVELS, N_TIMES, LEVEL_SECONDS = 6, 3, 3600
T0 = datetime(2020, 1, 1)
U_, V_, W_ = 'x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity'
SSH, DEPTH = 'sea_surface_height', 'sea_floor_depth_below_sea_level'
VARIABLES_3D, VARIABLES_2D = (U_, V_, W_), (SSH, DEPTH)
UTM = '+proj=utm +zone=33 +ellps=WGS84'
X0, Y0, SIZE = 400000.0, 6500000.0, 20000.0


def mesh_xy(seed=41, n=2000):
    return graded_points(n, seed, x0=X0, y0=Y0, size=SIZE)


def latlong_mesh(x, y):
    """The golden's geographic mesh: the UTM one mapped to degrees (exact operations)."""
    return 4.0 + (np.asarray(x) - X0) / 50000.0, 60.0 + (np.asarray(y) - Y0) / 100000.0


def mesh_fields(n):
    """dict(depth [N], elev [nt, N], zcor [nt, N, L], u, v, w [nt, N, L], du, dv [nt, N]) float32 of the golden mesh: depths 20 .. 80 m;
    the surface moves in time and zcor with it; the shallowest fifth of the nodes has 1 .. 3 levels below the sea bed (NaN); the
    elevation and w hold a few NaN (dry nodes)."""
    k = np.arange(n)
    depth = (50.0 + 30.0 * _unit(k, 5)).astype(np.float32)
    elev = np.stack([(0.25 * t + 0.3 * _unit(k, 7 + t)) for t in range(N_TIMES)]).astype(np.float32)
    s = 1.0 - np.arange(N_LEVELS, dtype=np.float64) / (N_LEVELS - 1)      # level 0 at the sea bed, the last one at the surface
    zcor = (elev.astype(np.float64)[:, :, None] - (depth.astype(np.float64)[None, :, None] + elev.astype(np.float64)[:, :, None]) * s).astype(np.float32)
    shallow = np.argsort(depth, kind='stable')[:n // 5]
    for j, node in enumerate(shallow):
        zcor[:, node, :1 + j % 3] = np.nan

    def field3(salt, mean, spread, per_level, per_time):
        a = np.empty((N_TIMES, n, N_LEVELS), np.float32)
        for t in range(N_TIMES):
            for lev in range(N_LEVELS):
                a[t, :, lev] = (mean + per_time * t + per_level * lev + spread * _unit(k, salt + 97 * t + 7 * lev)).astype(np.float32)
        return a
    u, v, w = field3(101, 0.5, 0.3, 0.04, 0.1), field3(202, 0.1, 0.4, -0.02, -0.15), field3(303, 0.0, 0.01, 0.0, 0.0)
    w[:, k % 89 == 3, N_LEVELS - 2] = np.nan
    ssh = elev.copy()
    ssh[:, k % 97 == 5] = np.nan
    du = np.stack([(0.6 + 0.1 * t + 0.3 * _unit(k, 404 + t)) for t in range(N_TIMES)]).astype(np.float32)
    dv = np.stack([(0.1 - 0.15 * t + 0.4 * _unit(k, 505 + t)) for t in range(N_TIMES)]).astype(np.float32)
    return dict(depth=depth, elev=ssh, zcor=zcor, u=u, v=v, w=w, du=du, dv=dv)


def times():
    return [T0 + timedelta(seconds=LEVEL_SECONDS * k) for k in range(N_TIMES)]


def golden_reader(g, case, variables=None):
    """readers.SchismReader over the mesh of the golden file g: case 'a' (UTM 33, 3-D) or 'b' (the same in degrees, depth-averaged)."""
    from opendrift_amd import readers
    x, y = g['x'], g['y']
    f = mesh_fields(len(x))
    if case == 'a':
        arrays = {U_: f['u'], V_: f['v'], W_: f['w'], SSH: f['elev'], DEPTH: f['depth']}
        kw = dict(zcor=f['zcor'], proj4=UTM)
    else:
        x, y = latlong_mesh(x, y)
        arrays = {U_: f['du'], V_: f['dv'], SSH: f['elev'], DEPTH: f['depth']}
        kw = dict(proj4='+proj=latlong')
    arrays = {k: v for k, v in arrays.items() if variables is None or k in variables}
    return readers.SchismReader(x, y, times(), arrays, name='c41_' + case, **kw)
