"""TEST INFRASTRUCTURE: ctypes access to the gradient stencil and the cell function of opendrift_amd/csrc/odr_ftle.hip.h compiled for
the host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see ftle_host.cpp; the NumPy restatement of
physics_methods.ftle that the GPU tests compare with; the error measure and the measured bounds of the FTLE tests."""
import ctypes as C

import numpy as np

from host_build import host_lib

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)

# max |host build - reference| / (1 / |T| + |reference|) over every finite cell of tests/golden/c33_ftle.npz: measured 8.71e-08 over
# the fields of (a) and 1.04e-07 over the maps of (b) on the CPU the golden was written on (tools/gen_golden_ftle.py prints them);
# the bound is 4 x the larger.  The reference takes BLAS's float32 D, LAPACK's float32 eigenvalue of it and
# float32 sqrt / log; the device one multiply and one add per term of D, the float64 closed form and one rounding of the exponent.
ARITHMETIC_MEASURED = 1.04e-07
ARITHMETIC_BOUND = 4 * ARITHMETIC_MEASURED

# max |device displacement - host displacement| / largest |coordinate| of the grid (tests/test_gpu_ftle.py): the device's proj_fwd
# against opendrift_amd.projection.Proj on 129 x 131 cells.  Measured on an MI355X: 0 for latlong, 3.91e-16 for the double gyre's
# stereographic sphere, 1.20e-15 for a polar stereographic ellipsoid (a few float64 roundings of coordinates of 1.4e6 m: the host
# takes np.tan and a power, the device cos / (1 + sin) and a series of the ellipsoidal factor); the bound is 4 x the largest.
PROJECTION_MEASURED = 1.20e-15
PROJECTION_BOUND = 4 * PROJECTION_MEASURED


def _lib():
    return host_lib('ftle_host', ('odr_ftle.hip.h',))


def gradient(f):
    """The header's np.gradient(f) of a 2-D float64 plane: [along axis 0, along axis 1]."""
    f = np.ascontiguousarray(f, np.float64)
    ny, nx = f.shape
    g0, g1 = np.empty_like(f), np.empty_like(f)
    _lib().ftleh_gradient(C.c_int(nx), C.c_int(ny), f.ctypes.data_as(_dp), g0.ctypes.data_as(_dp), g1.ctypes.data_as(_dp))
    return [g0, g1]


def ftle_map(dX, dY, delta, duration_seconds):
    """physics_methods.ftle(dX, dY, delta, duration) by the host build of the header: float32 [ny, nx]."""
    dX, dY = np.ascontiguousarray(dX, np.float64), np.ascontiguousarray(dY, np.float64)
    assert dX.ndim == 2 and dX.shape == dY.shape
    ny, nx = dX.shape
    out = np.empty((ny, nx), np.float32)
    _lib().ftleh_map(C.c_int(nx), C.c_int(ny), dX.ctypes.data_as(_dp), dY.ctypes.data_as(_dp), C.c_double(delta),
                    C.c_double(duration_seconds), out.ctypes.data_as(_fp))
    return out


def numpy_ftle(dX, dY, delta, duration_seconds):
    """physics_methods.ftle (models/physics_methods.py:458-484) restated with NumPy on whole arrays: np.gradient, the float32 J and
    D, np.linalg.eigvalsh of the float32 D in place of the loop's eigvals, float32 sqrt and log.  A cell with a NaN in its stencil
    is NaN (the reference's LAPACK call raises there)."""
    dx, dy = np.gradient(np.asarray(dX, np.float64)), np.gradient(np.asarray(dY, np.float64))
    J = np.empty(dx[0].shape + (2, 2), np.float32)
    J[..., 0, 0] = dx[0] / (2 * delta)
    J[..., 1, 0] = dy[0] / (2 * delta)
    J[..., 0, 1] = dx[1] / (2 * delta)
    J[..., 1, 1] = dy[1] / (2 * delta)
    D = np.matmul(np.swapaxes(J, -1, -2), J)
    assert D.dtype == np.float32
    bad = ~np.isfinite(D).all(axis=(-1, -2))
    D[bad] = np.eye(2, dtype=np.float32)
    lam = np.linalg.eigvalsh(D)[..., -1]
    assert lam.dtype == np.float32
    with np.errstate(divide='ignore', invalid='ignore'):
        out = (np.log(np.sqrt(np.maximum(lam, np.float32(0)))) / np.float32(abs(duration_seconds))).astype(np.float32)
    out[bad] = np.nan
    return out


def measure(got, want, duration_seconds):
    """max over the finite cells of `want` of |got - want| / (1 / |T| + |want|); the places of -inf and NaN must be identical."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN cells differ: %d / %d' % (np.isnan(got).sum(), np.isnan(want).sum())
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), '-inf cells differ: %d / %d' % (np.isneginf(got).sum(), np.isneginf(want).sum())
    assert not np.isposinf(got).any() and not np.isposinf(want).any()
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    return float(np.max(np.abs(g - w) / (1.0 / abs(duration_seconds) + np.abs(w))))
