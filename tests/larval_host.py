"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_larval.hip.h compiled for the
host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see larval_host.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'oracle', '_build', 'larval_host.so')
SRC = [os.path.join(HERE, 'larval_host.cpp'), os.path.join(HERE, 'hostshim', 'hip', 'hip_runtime.h'),
       os.path.join(ROOT, 'opendrift_amd', 'csrc', 'odr_larval.hip.h')]
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


def _f32(a, n):
    return np.array(np.broadcast_to(np.asarray(a, np.float32), (n,)), dtype=np.float32, order='C')


def update(temperature, dt, stage_fraction, hatched, weight, length):
    """update_fish_larvae of every element: (stage_fraction, hatched, weight, length) after the call, float32 copies, and
    `written`: bit 0 stage_fraction, bit 1 hatched, bit 2 weight and length were stored."""
    n = len(temperature)
    T, s, h, w, L = (_f32(a, n) for a in (temperature, stage_fraction, hatched, weight, length))
    written = np.zeros(n, np.uint8)
    lib().larvh_update(C.c_longlong(n), T.ctypes.data_as(_fp), C.c_double(dt), s.ctypes.data_as(_fp), h.ctypes.data_as(_fp),
                       w.ctypes.data_as(_fp), L.ctypes.data_as(_fp), written.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return s, h, w, L, written


def migrate(hatched, length, fraction_swimming, dt, direction, z):
    """larvae_vertical_migration of every element: (float64 z after the call, float32 displacement that was added)."""
    n = len(z)
    h, L = _f32(hatched, n), _f32(length, n)
    z = np.array(z, dtype=np.float64, order='C')
    disp = np.zeros(n, np.float32)
    lib().larvh_migrate(C.c_longlong(n), h.ctypes.data_as(_fp), L.ctypes.data_as(_fp), C.c_double(fraction_swimming), C.c_double(dt),
                        C.c_int(int(direction)), z.ctypes.data_as(C.POINTER(C.c_double)), disp.ctypes.data_as(_fp))
    return z, disp
