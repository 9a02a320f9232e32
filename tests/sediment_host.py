"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_sediment.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see sediment_host.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'oracle', '_build', 'sediment_host.so')
SRC = [os.path.join(HERE, 'sediment_host.cpp'), os.path.join(HERE, 'hostshim', 'hip', 'hip_runtime.h'),
       os.path.join(ROOT, 'opendrift_amd', 'csrc', 'odr_sediment.hip.h')]
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or any(os.path.getmtime(OUT) < os.path.getmtime(s) for s in SRC):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(HERE, 'hostshim'),
                                   '-shared', '-fPIC', '-o', OUT, SRC[0]])
        _lib = C.CDLL(OUT)
        _lib.sedh_resuspend.restype = C.c_longlong
    return _lib


def resuspend(u, v, threshold, moving, z):
    """(int32 moving, float64 z, count) after SedimentDrift.resuspension; threshold is cast to float32 as NumPy 2 does."""
    n = len(u)
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    moving, z = np.array(moving, np.int32), np.array(z, np.float64)
    count = lib().sedh_resuspend(C.c_longlong(n), u.ctypes.data_as(C.POINTER(C.c_float)), v.ctypes.data_as(C.POINTER(C.c_float)),
                                 C.c_float(np.float32(threshold)), moving.ctypes.data_as(C.POINTER(C.c_int)),
                                 z.ctypes.data_as(C.POINTER(C.c_double)))
    return moving, z, int(count)
