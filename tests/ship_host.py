"""TEST INFRASTRUCTURE: ctypes access to opendrift_amd/csrc/odr_ship.hip.h compiled for the host (g++ -ffp-contract=off,
tests/hostshim in place of the HIP runtime header), see ship_host.cpp; and ShipDrift.update of the host build end to end, with the
two moves made by the host build of the geodesic (tests/geod_host.cpp)."""
import ctypes as C

import numpy as np

from host_build import f32, host_lib

import berg_host

TM02 = 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'
ENV = ('x_sea_water_velocity', 'y_sea_water_velocity', 'x_wind', 'y_wind', 'sea_surface_wave_stokes_drift_x_velocity',
       'sea_surface_wave_stokes_drift_y_velocity', 'sea_surface_wave_significant_height', TM02)      # the order of ShipEnv
PROPS = ('length', 'height', 'draft', 'beam', 'wind_drag_coeff', 'water_drag_coeff')                 # the floats of ShipProp
F32 = ('bl', 'dl', 'Tm', 'Hs', 'F_wind_x', 'F_wind_y', 'beta1')                                      # ShipForces
F64 = ('F_wave_b', 'beta2_b', 'F_wave', 'beta2', 'wave_dir', 'F_total', 'uw_tot', 'uw_dir', 'velocity_u', 'velocity_v')
_fp, _dp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _lib():
    return host_lib('ship_host', ('odr_ship.hip.h',))


def ratios(length, draft, beam):
    n = len(length)
    a = [f32(v, n) for v in (length, draft, beam)]
    bl, dl = np.empty(n, np.float32), np.empty(n, np.float32)
    _lib().shiph_ratios(C.c_longlong(n), *(v.ctypes.data_as(_fp) for v in a + [bl, dl]))
    return bl, dl


def forces(env, props, orientation, cls, table, hs_mode, tp_mode, wave_dir_from_stokes):
    """ship_forces of every element.  env / props: {name: float32 array} (ENV, PROPS); table [n_classes][49][2].  Returns
    {name: array} for F32 + F64."""
    n = len(cls)
    e = [f32(env[k], n) for k in ENV]
    p = [f32(props[k], n) for k in PROPS]
    table = np.ascontiguousarray(table, np.float64)
    assert table.shape[1:] == (_lib().shiph_rows(), 2) and 0 <= np.min(cls) and np.max(cls) < len(table)
    ori, cls = (np.array(a, dtype=np.int32, order='C') for a in (orientation, cls))
    out = {k: np.zeros(n, np.float32) for k in F32}
    out.update({k: np.zeros(n, np.float64) for k in F64})
    _lib().shiph_forces(C.c_longlong(n), (_fp * 8)(*(a.ctypes.data_as(_fp) for a in e)), (_fp * 6)(*(a.ctypes.data_as(_fp) for a in p)),
                       ori.ctypes.data_as(_ip), cls.ctypes.data_as(_ip), table.ctypes.data_as(_dp), C.c_int(hs_mode), C.c_int(tp_mode),
                       C.c_int(int(wave_dir_from_stokes)), (_fp * 7)(*(out[k].ctypes.data_as(_fp) for k in F32)),
                       (_dp * 10)(*(out[k].ctypes.data_as(_dp) for k in F64)))
    return out


def move_f32(lon, lat, u, v, moving, dt):
    """update_positions with float32 velocities as the device makes it (move_f32, csrc/odr_kernels.hip.h): the azimuth rounded
    to float32 degrees, the float32 speed, along the host build of the geodesic."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    az = (np.arctan2(u.astype(np.float64), v.astype(np.float64)).astype(np.float32) * (np.float32(180.0) / np.float32(3.14159274101257324)))
    rad = np.radians(az.astype(np.float64))
    s12 = np.sqrt(u * u + v * v).astype(np.float64) * np.asarray(moving, np.float64) * dt
    lat2, lon2 = berg_host.geod_move(lat, lon, s12 * np.sin(rad), s12 * np.cos(rad))
    return lon2, lat2


def move_f64(lon, lat, u, v, moving, dt):
    hd = np.asarray(moving, np.float64) * dt
    lat2, lon2 = berg_host.geod_move(lat, lon, np.asarray(u, np.float64) * hd, np.asarray(v, np.float64) * hd)
    return lon2, lat2


def update(lon, lat, moving, land, env, props, orientation, cls, table, hs_mode, tp_mode, wave_dir_from_stokes, dt):
    """ShipDrift.update of the host build: the forces dict plus lon, lat after the two moves and `stranded`."""
    r = forces(env, props, orientation, cls, table, hs_mode, tp_mode, wave_dir_from_stokes)
    lon1, lat1 = move_f32(lon, lat, env[ENV[0]], env[ENV[1]], moving, dt)
    r['lon'], r['lat'] = move_f64(lon1, lat1, r['velocity_u'], r['velocity_v'], moving, dt)
    r['stranded'] = np.asarray(land, np.float32) == 1
    return r
