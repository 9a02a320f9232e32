"""TEST INFRASTRUCTURE: ctypes access to the unstructured-mesh arithmetic of opendrift_amd/csrc/odr_umesh.hip.h compiled for the host
(g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see umesh_host.cpp; NumPy's brute-force nearest point;
the criterion both the CPU and the GPU tests hold indices to; and the point sets they share."""
import ctypes as C
import os

import numpy as np

from host_build import host_lib

_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c36_unstructured.npz')


def _lib():
    lib = host_lib('umesh_host', ('odr_umesh.hip.h',))
    lib.umh_build.restype = C.c_void_p
    return lib


def _d(a):
    return np.ascontiguousarray(a, np.float64).ravel()


class HostIndex:
    """The k-d tree of the header over the points (x, y)."""

    def __init__(self, x, y):
        self.x, self.y = _d(x), _d(y)
        self.n = len(self.x)
        self.h = C.c_void_p(_lib().umh_build(C.c_int(self.n), self.x.ctypes.data_as(_dp), self.y.ctypes.data_as(_dp)))

    def __del__(self):
        try:
            _lib().umh_free(self.h)
        except Exception:
            pass

    def layout(self):
        px, py, ident = np.empty(self.n), np.empty(self.n), np.empty(self.n, np.int32)
        _lib().umh_layout(self.h, px.ctypes.data_as(_dp), py.ctypes.data_as(_dp), ident.ctypes.data_as(_ip))
        return px, py, ident

    def nearest(self, qx, qy, distances=False):
        qx, qy = _d(qx), _d(qy)
        out, d2 = np.empty(len(qx), np.int32), np.empty(len(qx))
        _lib().umh_nearest(self.h, C.c_longlong(len(qx)), qx.ctypes.data_as(_dp), qy.ctypes.data_as(_dp), out.ctypes.data_as(_ip),
                           d2.ctypes.data_as(_dp))
        return (out, d2) if distances else out


def sample(x, y, z, idx, box, data, sigma=None, h=None, first=True, out=None):
    """One variable at the elements whose nearest point is idx: (merged values, sigma indices); data [npts] or [nlev, npts]."""
    x, y, z = _d(x), _d(y), _d(z)
    idx = np.ascontiguousarray(idx, np.int32)
    data = np.ascontiguousarray(data, np.float32)
    nlev = data.shape[0] if data.ndim == 2 else 0
    npts = data.shape[-1]
    out = np.full(len(x), np.nan, np.float32) if out is None else np.array(out, np.float32)
    sig = np.empty(len(x), np.int32)
    if nlev:
        sigma, h = np.ascontiguousarray(sigma, np.float32), np.ascontiguousarray(h, np.float32)
        assert sigma.shape == (nlev, npts) and h.shape == (npts,)
    box = _d(box)
    _lib().umh_sample(C.c_longlong(len(x)), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), z.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                      box.ctypes.data_as(_dp), C.c_longlong(npts), C.c_int(nlev), sigma.ctypes.data_as(_fp) if nlev else None,
                      h.ctypes.data_as(_fp) if nlev else None, data.ctypes.data_as(_fp), C.c_int(int(first)), out.ctypes.data_as(_fp),
                      sig.ctypes.data_as(_ip))
    return out, sig


def rotate(u, v, cs, sn):
    u, v = np.array(u, np.float32), np.array(v, np.float32)
    cs, sn = _d(cs), _d(sn)
    _lib().umh_rotate(C.c_longlong(len(u)), u.ctypes.data_as(_fp), v.ctypes.data_as(_fp), cs.ctypes.data_as(_dp), sn.ctypes.data_as(_dp))
    return u, v


def dist2(px, py, qx, qy):
    """NumPy's float64 dx*dx + dy*dy, every operation rounded on its own."""
    dx, dy = px - qx, py - qy
    return dx * dx + dy * dy


def brute_nearest(px, py, qx, qy, chunk=512):
    out = np.empty(len(qx), np.int64)
    for o in range(0, len(qx), chunk):
        s = slice(o, o + chunk)
        out[s] = np.argmin(dist2(px[None, :], py[None, :], qx[s, None], qy[s, None]), axis=1)
    return out


def unexcused_mismatches(px, py, qx, qy, got, want):
    """(mismatches that are NOT excused, excused mismatches): an index may differ from the reference's only where NumPy's float64
    dx*dx + dy*dy of the two candidates are equal or adjacent floats."""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    k = np.flatnonzero(got != want)
    if not len(k):
        return 0, 0
    if (got[k] < 0).any() or (got[k] >= len(px)).any():
        return len(k), 0
    a, b = dist2(px[got[k]], py[got[k]], qx[k], qy[k]), dist2(px[want[k]], py[want[k]], qx[k], qy[k])
    ok = (a == b) | (np.nextafter(a, b) == b)
    return int((~ok).sum()), int(ok.sum())


def graded_points(n, seed, x0=400000.0, y0=6500000.0, size=60000.0, fine=0.25):
    """Random points over a square of `size` metres, a share `fine` of them in a corner of size / 100: spacing graded 100 : 1."""
    rng = np.random.default_rng(seed)
    nf = int(n * fine)
    x = np.concatenate([x0 + size * rng.random(n - nf), x0 + 0.01 * size * rng.random(nf)])
    y = np.concatenate([y0 + size * rng.random(n - nf), y0 + 0.01 * size * rng.random(nf)])
    return x, y


def queries(px, py, n, seed, outside=0.1):
    """Random queries over the points' box widened by `outside` of its size on every side, plus a few far outside it."""
    rng = np.random.default_rng(seed)
    w, h = max(np.ptp(px), 1.0), max(np.ptp(py), 1.0)
    qx = rng.uniform(px.min() - outside * w, px.max() + outside * w, n)
    qy = rng.uniform(py.min() - outside * h, py.max() + outside * h, n)
    far = max(1, n // 50)
    qx[:far] = px.min() + w * rng.uniform(-1e4, 1e4, far)
    qy[:far] = py.min() + h * rng.uniform(-1e4, 1e4, far)
    return qx, qy


# ---- the mesh of tests/golden/c36_unstructured.npz: the file holds the coordinates; everything else is formed here, by the
# generator (tools/gen_golden_umesh.py) and by the tests alike, with additions, multiplications, divisions and integer
# arithmetic only -- IEEE operations that give the same bits on every machine
N_SIGLAY, N_TIMES, LEVEL_SECONDS = 5, 3, 3600
FACE_VARIABLES = ('x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity')
NODE_VARIABLES = ('sea_water_temperature', 'sea_water_salinity')      # on the levels, on the layers


def _unit(index, salt):
    """A fixed pseudo-random value in [-1, 1] per (index, salt): multiples of 1 / 1000."""
    h = (np.asarray(index, np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(2 ** 32)
    return ((h >> np.uint64(8)) % np.uint64(2001)).astype(np.float64) / 1000.0 - 1.0


def _sigma(npts, salt):
    """(siglay [L, npts], siglev [L + 1, npts], h [npts]) float32: levels from 0 to -1, stretched differently in every column."""
    s = (np.arange(N_SIGLAY + 1, dtype=np.float64) / N_SIGLAY)[:, None]
    c = 0.25 * (_unit(np.arange(npts), salt) + 1.0)[None, :]
    siglev = (-s - c * s * (1.0 - s)).astype(np.float32)
    siglay = ((siglev[:-1] + siglev[1:]) * np.float32(0.5)).astype(np.float32)
    h = (110.0 + 90.0 * _unit(np.arange(npts), salt + 1)).astype(np.float32)
    return siglay, siglev, h


def mesh_fields(n_nodes, n_faces):
    """The sigma arrays and the variables of the golden mesh: dict(siglay, siglev, h, siglay_center, siglev_center, h_center,
    node_arrays {name: [nt, levels, N]}, face_arrays {name: [nt, L, E]})."""
    out = {}
    out['siglay'], out['siglev'], out['h'] = _sigma(n_nodes, 11)
    out['siglay_center'], out['siglev_center'], out['h_center'] = _sigma(n_faces, 23)

    def field(npts, nlev, salt, mean, spread, per_level, per_time):
        k = np.arange(npts)
        a = np.empty((N_TIMES, nlev, npts), np.float32)
        for t in range(N_TIMES):
            for lev in range(nlev):
                a[t, lev] = (mean + per_time * t + per_level * lev + spread * _unit(k, salt + 97 * t + 7 * lev)).astype(np.float32)
        return a
    out['face_arrays'] = {
        'x_sea_water_velocity': field(n_faces, N_SIGLAY, 101, 0.7, 0.3, -0.05, 0.1),
        'y_sea_water_velocity': field(n_faces, N_SIGLAY, 202, 0.1, 0.4, 0.02, -0.15),
        'upward_sea_water_velocity': field(n_faces, N_SIGLAY, 303, 0.0, 0.01, 0.0, 0.0)}
    out['node_arrays'] = {
        'sea_water_temperature': field(n_nodes, N_SIGLAY + 1, 404, 9.0, 2.0, -0.8, 0.3),
        'sea_water_salinity': field(n_nodes, N_SIGLAY, 505, 33.0, 1.0, 0.3, 0.0)}
    return out


def latlong_mesh(x, y):
    """The golden's geographic mesh: the UTM one mapped to degrees (exact operations)."""
    return 4.0 + (np.asarray(x) - 400000.0) / 60000.0, 60.0 + (np.asarray(y) - 6500000.0) / 120000.0


def golden_reader(g, case, variables=None):
    """readers.UnstructuredReader over the mesh of the golden file g: case 'a' (UTM 33) or 'b' (the same in degrees)."""
    from datetime import datetime, timedelta
    from opendrift_amd import readers
    x, y, xc, yc, proj4 = g['x'], g['y'], g['xc'], g['yc'], str(g['proj4'])
    if case == 'b':
        (x, y), (xc, yc), proj4 = latlong_mesh(x, y), latlong_mesh(xc, yc), '+proj=latlong'
    f = mesh_fields(len(x), len(xc))
    times = [datetime(2020, 1, 1) + timedelta(seconds=LEVEL_SECONDS * k) for k in range(N_TIMES)]
    pick = lambda d: {k: v for k, v in d.items() if variables is None or k in variables}
    return readers.UnstructuredReader(x, y, xc, yc, times, pick(f['node_arrays']), pick(f['face_arrays']), proj4=proj4, name='c36_' + case,
                                      **{k: f[k] for k in ('siglay', 'siglev', 'siglay_center', 'siglev_center', 'h', 'h_center')})


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN placement included (any NaN equals any NaN)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def ulp32(v):
    """One float32 unit in the last place at magnitude v."""
    v = np.maximum(np.abs(np.asarray(v, np.float32)), np.finfo(np.float32).tiny)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)
