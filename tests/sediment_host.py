"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_sediment.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see sediment_host.cpp."""
import ctypes as C

import numpy as np

from host_build import host_lib


def _lib():
    L = host_lib('sediment_host', ('odr_sediment.hip.h',))
    L.sedh_resuspend.restype = C.c_longlong
    return L


def resuspend(u, v, threshold, moving, z):
    """(int32 moving, float64 z, count) after SedimentDrift.resuspension; threshold is cast to float32 as NumPy 2 does."""
    n = len(u)
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    moving, z = np.array(moving, np.int32), np.array(z, np.float64)
    count = _lib().sedh_resuspend(C.c_longlong(n), u.ctypes.data_as(C.POINTER(C.c_float)), v.ctypes.data_as(C.POINTER(C.c_float)),
                                 C.c_float(np.float32(threshold)), moving.ctypes.data_as(C.POINTER(C.c_int)),
                                 z.ctypes.data_as(C.POINTER(C.c_double)))
    return moving, z, int(count)
