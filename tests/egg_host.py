"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_egg.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see egg_host.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'oracle', '_build', 'egg_host.so')
SRC = [os.path.join(HERE, 'egg_host.cpp'), os.path.join(HERE, 'hostshim', 'hip', 'hip_runtime.h')] + \
    [os.path.join(ROOT, 'opendrift_amd', 'csrc', f) for f in ('odr_egg.hip.h', 'odr_seawater.hip.h')]
_fp = C.POINTER(C.c_float)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or any(os.path.getmtime(OUT) < os.path.getmtime(s) for s in SRC):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(HERE, 'hostshim'),
                                   '-shared', '-fPIC', '-o', OUT, SRC[0]])
        _lib = C.CDLL(OUT)
    return _lib


def terminal_velocity(temperature, salinity, diameter, neutral_buoyancy_salinity):
    """(float32 terminal velocity, bool high-Reynolds branch taken) per element."""
    n = len(temperature)
    arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (n,))) for a in
            (temperature, salinity, diameter, neutral_buoyancy_salinity)]
    w, high = np.empty(n, np.float32), np.empty(n, np.uint8)
    lib().eggh_terminal_velocity(C.c_longlong(n), *[a.ctypes.data_as(_fp) for a in arrs], w.ctypes.data_as(_fp),
                                 high.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return w, high.astype(bool)
