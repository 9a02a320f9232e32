"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_plast.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see plast_host.cpp."""
import ctypes as C

import numpy as np

from host_build import f32, f64, host_lib

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _lib():
    return host_lib('plast_host', ('odr_plast.hip.h',))


def stokes_from_wind(x_wind, y_wind, stokes_coeff, hs_coeff):
    """(float32 Stokes x, Stokes y, wave height) per element from the float32 wind."""
    n = len(x_wind)
    xw, yw = f32(x_wind, n), f32(y_wind, n)
    sc, hc = f64(stokes_coeff, len(stokes_coeff)), f64(hs_coeff, 2)
    sx, sy, hs = (np.empty(n, np.float32) for _ in range(3))
    _lib().plasth_stokes_from_wind(C.c_longlong(n), xw.ctypes.data_as(_fp), yw.ctypes.data_as(_fp), sc.ctypes.data_as(_dp),
                                   C.c_int(len(sc)), hc.ctypes.data_as(_dp), sx.ctypes.data_as(_fp), sy.ctypes.data_as(_fp),
                                   hs.ctypes.data_as(_fp))
    return sx, sy, hs


def depth(K, w, E, z_before=None):
    """(float64 z, refused): z = -(K / w) E per element; refused: some scale is one NumPy refuses, z is z_before then."""
    n = len(E)
    K, w, E = f32(K, n), f32(w, n), f64(E, n)
    z = f64(np.nan if z_before is None else z_before, n)
    refused = _lib().plasth_depth(C.c_longlong(n), K.ctypes.data_as(_fp), w.ctypes.data_as(_fp), E.ctypes.data_as(_dp),
                                  z.ctypes.data_as(_dp))
    return z, bool(refused)
