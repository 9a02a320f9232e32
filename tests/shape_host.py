"""TEST INFRASTRUCTURE: ctypes access to the coastline-polygon arithmetic of opendrift_amd/csrc/odr_shape.hip.h compiled for the host
(g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see shape_host.cpp; the polygons of
tests/golden/c37_shape_landmask.npz; and the small shapes at which the index can go wrong, shared by the CPU and the GPU tests."""
import ctypes as C
import os

import numpy as np

from host_build import host_lib

_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c37_shape_landmask.npz')
UTM = '+proj=utm +zone=33 +ellps=WGS84'


def _lib():
    lib = host_lib('shape_host', ('odr_shape.hip.h',))
    lib.shh_build.restype = C.c_void_p
    lib.shh_error.restype = C.c_char_p
    return lib


def _d(a):
    return np.ascontiguousarray(a, np.float64).ravel()


class HostShape:
    """The index of the header over the edges of a readers.ShapeReader (or anything with x1, y1, x2, y2, poly, n_polygons, invert)."""

    def __init__(self, reader, nx=0, ny=0):
        self.e = [_d(getattr(reader, k)) for k in ('x1', 'y1', 'x2', 'y2')]
        self.poly = np.ascontiguousarray(reader.poly, np.int32)
        self.h = C.c_void_p(_lib().shh_build(C.c_longlong(len(self.poly)), *[a.ctypes.data_as(_dp) for a in self.e], self.poly.ctypes.data_as(_ip),
                                             C.c_int(reader.n_polygons), C.c_int(nx), C.c_int(ny), C.c_int(int(reader.invert))))
        err = _lib().shh_error(self.h).decode()
        if err:
            raise ValueError(err)

    def __del__(self):
        try:
            _lib().shh_free(self.h)
        except Exception:
            pass

    def stats(self):
        a = np.zeros(11)
        _lib().shh_stats(self.h, a.ctypes.data_as(_dp))
        return dict(zip(('cells', 'entries', 'longest_list', 'mean_list', 'nudges', 'nx', 'ny', 'x0', 'y0', 'dx', 'dy'), a.tolist()))

    def cell_counts(self):
        """(edge entries, toggle entries) per cell, [ny, nx]."""
        s = self.stats()
        nx, ny = int(s['nx']), int(s['ny'])
        e, t = np.zeros(nx * ny, np.int32), np.zeros(nx * ny, np.int32)
        _lib().shh_cell_counts(self.h, e.ctypes.data_as(_ip), t.ctypes.data_as(_ip))
        return e.reshape(ny, nx), t.reshape(ny, nx)

    def _ask(self, fn, x, y):
        x, y = _d(x), _d(y)
        out = np.empty(len(x), np.float32)
        fn(self.h, C.c_longlong(len(x)), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), out.ctypes.data_as(_fp))
        return out

    def contains(self, x, y):
        """The mask through the index, as k_shape_contains: float32 1 / 0, NaN outside the box."""
        return self._ask(_lib().shh_contains, x, y)

    def all_edges(self, x, y):
        """The definition over all edges, same box and inversion."""
        return self._ask(_lib().shh_all_edges, x, y)

    def sample(self, x, y, first, out):
        x, y = _d(x), _d(y)
        out = np.array(out, np.float32)
        _lib().shh_sample(self.h, C.c_longlong(len(x)), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), C.c_int(int(first)), out.ctypes.data_as(_fp))
        return out


def same_mask(a, b):
    """float32 masks equal value for value, NaN placement included."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ---- the polygons of the golden file: the file holds every ring's vertices in one array with the ring lengths and, per ring, its
# polygon and whether it is a hole
def golden_polygons(g, prefix):
    """[(exterior, [holes])] from <prefix>_ring_xy, _ring_n, _ring_poly."""
    xy, n, poly = g[prefix + '_ring_xy'], g[prefix + '_ring_n'], g[prefix + '_ring_poly']
    rings, o = [], 0
    for k in n:
        rings.append(xy[o:o + k])
        o += k
    out = []
    for p in range(int(poly.max()) + 1):
        mine = [r for r, q in zip(rings, poly) if q == p]
        out.append((mine[0], mine[1:]))
    return out


def golden_reader(g, case):
    """readers.ShapeReader of case 'a' (lon / lat), 'b' (1/4 lattice), 'c' (UTM 33) or 'd' (inverted a)."""
    from opendrift_amd import readers
    prefix = {'a': 'a', 'b': 'b', 'c': 'c', 'd': 'a'}[case]
    return readers.ShapeReader(golden_polygons(g, prefix), proj4_str=UTM if case == 'c' else '+proj=lonlat +ellps=WGS84', invert=case == 'd')


class Geo:
    """The three lines of a geometry object: anything with __geo_interface__."""

    def __init__(self, gi):
        self.__geo_interface__ = gi


# ---- the smallest shapes at which the index can still go wrong: name -> (polygons, invert, nx, ny)
def _square(x0, y0, s):
    return np.array([[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]], float)


def edge_shapes():
    big = _square(0.0, 0.0, 16.0)
    return {
        'triangle': ([np.array([[0.0, 0.0], [4.0, 0.5], [1.5, 3.0]])], False, 0, 0),
        'one_cell': ([np.array([[0.0, 0.0], [4.0, 0.5], [1.5, 3.0]]), _square(3.0, 2.0, 2.0)], False, 1, 1),
        # a big square on a fine grid: cells deep inside hold one toggle and nothing else, cells of the hole's interior nothing
        'toggle_and_empty_cells': ([(big, [_square(4.0, 4.0, 8.0)])], False, 16, 16),
        # the intersection of two overlapping squares is land: one parity over all edges would call it water
        'overlapping_squares': ([_square(0.0, 0.0, 4.0), _square(2.0, 2.0, 4.0)], False, 5, 5),
        'hole_with_island': ([(_square(0.0, 0.0, 9.0), [_square(2.0, 2.0, 5.0)]), _square(3.5, 3.5, 2.0)], False, 0, 0),
        'inverted': ([(_square(0.0, 0.0, 9.0), [_square(2.0, 2.0, 5.0)]), _square(3.5, 3.5, 2.0)], True, 3, 4),
        'geo_multipolygon': ([Geo({'type': 'MultiPolygon', 'coordinates': [[_square(0.0, 0.0, 3.0).tolist()],
                                                                           [_square(5.0, 1.0, 2.0).tolist(), _square(5.5, 1.5, 0.5).tolist()]]})], False, 0, 0),
    }


def shape_queries(reader, n, seed):
    """n queries over the box of the rings widened by a tenth: random ones, some on a 1/8 lattice, the corners and mid-sides of the box
    (queries exactly on the right and top bound), one not finite."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = reader.box
    w, h = x1 - x0, y1 - y0
    qx, qy = rng.uniform(x0 - 0.1 * w, x1 + 0.1 * w, n), rng.uniform(y0 - 0.1 * h, y1 + 0.1 * h, n)
    k = n // 3
    qx[:k], qy[:k] = np.round(qx[:k] * 8.0) / 8.0 + 1.0 / 16.0, np.round(qy[:k] * 8.0) / 8.0 + 1.0 / 16.0
    special = [(x1, 0.5 * (y0 + y1) + 0.01 * h), (0.5 * (x0 + x1) + 0.01 * w, y1), (x1, y1), (x0, y0), (np.nan, y0), (x0, np.inf)]
    for j, (sx, sy) in enumerate(special[:n]):
        qx[n - 1 - j], qy[n - 1 - j] = sx, sy
    return qx, qy


def lines_through_vertices(nx=4, ny=4):
    """Polygons whose vertices and axis-parallel edges lie exactly on the lines a grid of nx x ny cells has BEFORE its origin is
    shifted: the box is fixed by an outer rectangle, the grid of that box is read from a first build, and a second polygon is
    placed on its lines."""
    from opendrift_amd import readers
    outer = np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 6.0], [0.0, 6.0]])
    s = HostShape(readers.ShapeReader([outer]), nx, ny).stats()
    assert s['nudges'] == 0
    lx = [s['x0'] + i * s['dx'] for i in range(nx + 1)]      # sh_line: one product, one sum
    ly = [s['y0'] + j * s['dy'] for j in range(ny + 1)]
    inner = np.array([[lx[1], ly[1]], [lx[3], ly[1]], [lx[3], ly[2]], [lx[2], ly[2]], [lx[2], ly[3]], [lx[1], ly[3]]])
    assert 0.0 < lx[1] and lx[3] < 8.0 and 0.0 < ly[1] and ly[3] < 6.0
    return [(outer, [inner])]
