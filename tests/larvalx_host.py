"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_larvalx.hip.h and odr_solar.hip.h
compiled for the host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see larvalx_host.cpp; and the
three time scalars of the solar elevation, formed as opendrift_amd.oceandrift forms them."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'oracle', '_build', 'larvalx_host.so')
SRC = [os.path.join(HERE, 'larvalx_host.cpp'), os.path.join(HERE, 'hostshim', 'hip', 'hip_runtime.h'),
       os.path.join(ROOT, 'opendrift_amd', 'csrc', 'odr_larvalx.hip.h'), os.path.join(ROOT, 'opendrift_amd', 'csrc', 'odr_solar.hip.h')]
MODES = {'depth': 1, 'dvm': 2}      # include/odrift.h ODR_LARVALX_DEPTH / _DVM
_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
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


def _f64(a, n):
    return np.array(np.broadcast_to(np.asarray(a, np.float64), (n,)), dtype=np.float64, order='C')


def elevation(lon, lat, scalars):
    """Solar elevation [deg] of every element; scalars: (declination_rad, equation of time [min], minutes of the day)."""
    n = len(lon)
    lon, lat, out = _f64(lon, n), _f64(lat, n), np.zeros(n)
    lib().larvxh_elevation(C.c_longlong(n), lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp), *(C.c_double(float(s)) for s in scalars),
                           out.ctypes.data_as(_dp))
    return out


def hatch(increment, stage_fraction, hatched):
    """update_fish_larvae of every element: (stage_fraction, hatched) after the call, float32 copies."""
    n = len(stage_fraction)
    s, h = _f32(stage_fraction, n), _f32(hatched, n)
    lib().larvxh_hatch(C.c_longlong(n), C.c_double(increment), s.ctypes.data_as(_fp), h.ctypes.data_as(_fp))
    return s, h


def behave(z, hatched, depth, lon, lat, mode, only_hatched, z_f32, band0, band1, w_active, dt, scalars=(0.0, 0.0, 0.0)):
    """_apply_vertical_behavior of every element: (float64 z after the call, the day flag each moving element used).
    band0 / band1: (centre, half-width) of the depth or night band and of the day band."""
    n = len(z)
    z, lon, lat = _f64(z, n), _f64(lon, n), _f64(lat, n)
    h, d = _f32(hatched, n), _f32(depth, n)
    day = np.zeros(n, np.uint8)
    lib().larvxh_behave(C.c_longlong(n), h.ctypes.data_as(_fp), d.ctypes.data_as(_fp), lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp),
                        C.c_int(MODES[mode]), C.c_int(int(only_hatched)), C.c_int(int(z_f32)), *(C.c_double(float(v)) for v in tuple(band0) + tuple(band1)),
                        C.c_double(w_active), C.c_double(dt), *(C.c_double(float(s)) for s in scalars), z.ctypes.data_as(_dp),
                        day.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return z, day.astype(bool)
