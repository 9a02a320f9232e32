"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_egg.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see egg_host.cpp."""
import ctypes as C

import numpy as np

from host_build import host_lib

_fp = C.POINTER(C.c_float)


def _lib():
    return host_lib('egg_host', ('odr_egg.hip.h', 'odr_seawater.hip.h'))


def terminal_velocity(temperature, salinity, diameter, neutral_buoyancy_salinity):
    """(float32 terminal velocity, bool high-Reynolds branch taken) per element."""
    n = len(temperature)
    arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (n,))) for a in
            (temperature, salinity, diameter, neutral_buoyancy_salinity)]
    w, high = np.empty(n, np.float32), np.empty(n, np.uint8)
    _lib().eggh_terminal_velocity(C.c_longlong(n), *[a.ctypes.data_as(_fp) for a in arrs], w.ctypes.data_as(_fp),
                                 high.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return w, high.astype(bool)
