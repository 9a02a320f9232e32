"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_larval.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see larval_host.cpp."""
import ctypes as C

import numpy as np

from host_build import f32, host_lib

_fp = C.POINTER(C.c_float)


def _lib():
    return host_lib('larval_host', ('odr_larval.hip.h',))


def update(temperature, dt, stage_fraction, hatched, weight, length):
    """update_fish_larvae of every element: (stage_fraction, hatched, weight, length) after the call, float32 copies, and
    `written`: bit 0 stage_fraction, bit 1 hatched, bit 2 weight and length were stored."""
    n = len(temperature)
    T, s, h, w, L = (f32(a, n) for a in (temperature, stage_fraction, hatched, weight, length))
    written = np.zeros(n, np.uint8)
    _lib().larvh_update(C.c_longlong(n), T.ctypes.data_as(_fp), C.c_double(dt), s.ctypes.data_as(_fp), h.ctypes.data_as(_fp),
                       w.ctypes.data_as(_fp), L.ctypes.data_as(_fp), written.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return s, h, w, L, written


def migrate(hatched, length, fraction_swimming, dt, direction, z):
    """larvae_vertical_migration of every element: (float64 z after the call, float32 displacement that was added)."""
    n = len(z)
    h, L = f32(hatched, n), f32(length, n)
    z = np.array(z, dtype=np.float64, order='C')
    disp = np.zeros(n, np.float32)
    _lib().larvh_migrate(C.c_longlong(n), h.ctypes.data_as(_fp), L.ctypes.data_as(_fp), C.c_double(fraction_swimming), C.c_double(dt),
                        C.c_int(int(direction)), z.ctypes.data_as(C.POINTER(C.c_double)), disp.ctypes.data_as(_fp))
    return z, disp
