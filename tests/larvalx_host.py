"""TEST INFRASTRUCTURE: ctypes access to the per-element arithmetic of opendrift_amd/csrc/odr_larvalx.hip.h and odr_solar.hip.h
compiled for the host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see larvalx_host.cpp; and the
three time scalars of the solar elevation, formed as opendrift_amd.oceandrift forms them."""
import ctypes as C

import numpy as np

from host_build import f32, f64, host_lib

MODES = {'depth': 1, 'dvm': 2}      # include/odrift.h ODR_LARVALX_DEPTH / _DVM
_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _lib():
    return host_lib('larvalx_host', ('odr_larvalx.hip.h', 'odr_solar.hip.h'))


def elevation(lon, lat, scalars):
    """Solar elevation [deg] of every element; scalars: (declination_rad, equation of time [min], minutes of the day)."""
    n = len(lon)
    lon, lat, out = f64(lon, n), f64(lat, n), np.zeros(n)
    _lib().larvxh_elevation(C.c_longlong(n), lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp), *(C.c_double(float(s)) for s in scalars),
                           out.ctypes.data_as(_dp))
    return out


def hatch(increment, stage_fraction, hatched):
    """update_fish_larvae of every element: (stage_fraction, hatched) after the call, float32 copies."""
    n = len(stage_fraction)
    s, h = f32(stage_fraction, n), f32(hatched, n)
    _lib().larvxh_hatch(C.c_longlong(n), C.c_double(increment), s.ctypes.data_as(_fp), h.ctypes.data_as(_fp))
    return s, h


def behave(z, hatched, depth, lon, lat, mode, only_hatched, z_f32, band0, band1, w_active, dt, scalars=(0.0, 0.0, 0.0)):
    """_apply_vertical_behavior of every element: (float64 z after the call, the day flag each moving element used).
    band0 / band1: (centre, half-width) of the depth or night band and of the day band."""
    n = len(z)
    z, lon, lat = f64(z, n), f64(lon, n), f64(lat, n)
    h, d = f32(hatched, n), f32(depth, n)
    day = np.zeros(n, np.uint8)
    _lib().larvxh_behave(C.c_longlong(n), h.ctypes.data_as(_fp), d.ctypes.data_as(_fp), lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp),
                        C.c_int(MODES[mode]), C.c_int(int(only_hatched)), C.c_int(int(z_f32)), *(C.c_double(float(v)) for v in tuple(band0) + tuple(band1)),
                        C.c_double(w_active), C.c_double(dt), *(C.c_double(float(s)) for s in scalars), z.ctypes.data_as(_dp),
                        day.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return z, day.astype(bool)
