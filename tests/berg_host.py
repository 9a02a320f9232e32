"""TEST INFRASTRUCTURE: ctypes access to opendrift_amd/csrc/odr_berg.hip.h compiled for the host (g++ -ffp-contract=off,
tests/hostshim in place of the HIP runtime header), see berg_host.cpp."""
import ctypes as C

import numpy as np

from host_build import f32, geod_host, host_lib

BLOCK = 256       # ODR_BLOCK (opendrift_amd/csrc/odr_kernels.hip.h): the workgroup size the sums are ordered by
ENV = ('x_sea_water_velocity', 'y_sea_water_velocity', 'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity',
       'x_wind', 'y_wind', 'sea_floor_depth_below_sea_level', 'sea_surface_height', 'sea_surface_wave_significant_height',
       'sea_ice_area_fraction', 'sea_ice_x_velocity', 'sea_ice_y_velocity')      # the order of BergEnv
COEF = dict(weight_coef=1.0, water_form_drag_coef=0.25, water_skin_drag_coef=0.0055, wind_form_drag_coef=0.8, wind_skin_drag_coef=0.0022,
            wave_drag_coef=0.3)      # the order of BergCoef, the defaults of IcebergObj
SOLVE = {0: 'ok', 1: 'error norm not finite', 2: 'step too small', 3: 'too many attempts'}
_fp, _dp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _lib():
    L = host_lib('berg_host', ('odr_berg.hip.h',))
    L.bergh_sin.restype = C.c_double
    L.bergh_sin.argtypes = [C.c_double]
    return L


def geod_move(lat, lon, east, north):
    """One move of csrc/odr_geodesic.hip.h (tests/geod_host.cpp, the host build tests/test_geod_host.py uses) from (lat, lon) by
    (east, north) metres: (lat2, lon2)."""
    _geod = geod_host()
    a = [np.ascontiguousarray(v, np.float64) for v in (lat, lon, east, north)]
    series = np.empty(len(a[0]), np.int32)
    for full in (1, 0):      # the complete solution, replaced by the series move wherever that is valid (as geod_local_move)
        la, lo = np.empty_like(a[0]), np.empty_like(a[0])
        _geod.gh_move(C.c_longlong(len(a[0])), *(v.ctypes.data_as(_dp) for v in a), C.c_int(full), la.ctypes.data_as(_dp), lo.ctypes.data_as(_dp),
                      series.ctypes.data_as(_ip))
        if full:
            lat2, lon2 = la, lo
    ok = series == 1
    lat2[ok], lon2[ok] = la[ok], lo[ok]
    return lat2, lon2


def sin(x):
    return _lib().bergh_sin(float(x))


def sincosf(x):
    """berg_sincosf_numpy of a float32 array: (sin, cos)."""
    x = np.ascontiguousarray(x, np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    _lib().bergh_sincosf(C.c_longlong(len(x)), *(a.ctypes.data_as(_fp) for a in (x, s, c)))
    return s, c


def roll_over(sail, draft, length, width):
    """roll_over of every element: float32 copies of (sail, draft, length, width) after the call."""
    n = len(sail)
    s, d, L, W = (f32(a, n) for a in (sail, draft, length, width))
    _lib().bergh_roll_over(C.c_longlong(n), *(a.ctypes.data_as(_fp) for a in (s, d, L, W)))
    return s, d, L, W


def advect(env, lat, sail, draft, length, width, moving, dt, wave_from_direction=0.0, sea_ice_thickness=0.0, wave_rad=True,
           stokes_drift=False, coriolis=True, grounding=True, lat_is_float32=False, block=BLOCK, **coef):
    """advect_iceberg up to update_positions.  env: {variable name: float32 array}.  Returns a dict: V0x, V0y, Vx, Vy (float64),
    iceb_x_velocity, iceb_y_velocity (float32), grounded, moving, attempts, rejected, status (a key of SOLVE)."""
    n = len(lat)
    e = [f32(env[k], n) for k in ENV]
    envp = (_fp * len(ENV))(*(a.ctypes.data_as(_fp) for a in e))
    lat = np.array(lat, dtype=np.float64, order='C')
    s, d, L, W = (f32(a, n) for a in (sail, draft, length, width))
    moving = np.array(moving, dtype=np.int32, order='C')
    k = dict(COEF, **coef)
    # IcebergObj declares the coefficients float32: the reference's float64 arrays hold float32 values (0.8 is 0.800000011920929)
    coefs = np.array([k[name] for name in COEF], dtype=np.float32).astype(np.float64)
    flags = np.array([wave_rad, stokes_drift, coriolis, grounding, lat_is_float32], dtype=np.int32)
    out = {name: np.zeros(n, np.float64) for name in ('V0x', 'V0y', 'Vx', 'Vy')}
    xv, yv = np.zeros(n, np.float32), np.zeros(n, np.float32)
    grounded = np.zeros(n, np.int8)
    stat = np.zeros(2, np.int32)
    rc = _lib().bergh_advect(C.c_longlong(n), envp, lat.ctypes.data_as(_dp), *(a.ctypes.data_as(_fp) for a in (s, d, L, W)),
                            moving.ctypes.data_as(_ip), coefs.ctypes.data_as(_dp), C.c_double(wave_from_direction), C.c_double(sea_ice_thickness),
                            flags.ctypes.data_as(_ip), C.c_double(dt), C.c_int(block), *(out[name].ctypes.data_as(_dp) for name in ('V0x', 'V0y', 'Vx', 'Vy')),
                            xv.ctypes.data_as(_fp), yv.ctypes.data_as(_fp), grounded.ctypes.data_as(C.POINTER(C.c_byte)), stat.ctypes.data_as(_ip))
    out.update(iceb_x_velocity=xv, iceb_y_velocity=yv, grounded=grounded, moving=moving, attempts=int(stat[0]), rejected=int(stat[1]), status=int(rc))
    return out
