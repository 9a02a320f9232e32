"""TEST INFRASTRUCTURE: ctypes access to geod_inverse and the trajectory lengths of opendrift_amd/csrc/odr_geodinv.hip.h compiled for
the host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see geodinv_host.cpp; and the metric that turns
an error of (azi1, s12) into metres at point 2."""
import ctypes as C

import numpy as np

from host_build import host_lib

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)

# Bounds: 4 x the host build's measured maximum (DESIGN.md sections 7e, 8i), all far inside the 1e-6 m pin of the oracle's own inverse.
# Measured over tests/golden/geodesic_inverse_kat.npz: |s12 - KAT| 3.73e-9 m, landing error of (azi1, s12) at point 2 3.83e-9 m --
# what rounding the stored end point to float64 accounts for.  Over tests/golden/c34_trajectory_lengths.npz against the reference's
# distances: 2.68e-9 m.
KAT_S12_BOUND_M = 4 * 3.73e-9
KAT_LANDING_BOUND_M = 4 * 3.83e-9
C34_DISTANCE_BOUND_M = 4 * 2.68e-9


def _lib():
    return host_lib('geodinv_host', ('odr_geodinv.hip.h', 'odr_geodesic.hip.h'))


def inverse(lon1, lat1, lon2, lat2):
    """(azi1, azi2, s12) of the header's geod_inverse: forward azimuths at both ends [deg], length [m]."""
    a = [np.ascontiguousarray(v, np.float64) for v in np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, np.float64))
                                                                            for v in (lon1, lat1, lon2, lat2)))]
    n = a[0].size
    out = [np.empty(a[0].shape) for _ in range(3)]
    _lib().geodinvh_inverse(C.c_longlong(n), *(v.ctypes.data_as(_dp) for v in a), *(o.ctypes.data_as(_dp) for o in out))
    return tuple(out)


def trajectory_lengths(lon, lat, dt, segments=True):
    """The signature of opendrift_amd.device.Context.trajectory_lengths, computed by the host build of the header."""
    lon, lat = np.ascontiguousarray(lon, np.float32), np.ascontiguousarray(lat, np.float32)
    ntraj, nt = lon.shape
    total = np.empty(ntraj)
    dist = np.empty((nt - 1, ntraj)) if segments else None
    speed = np.empty((nt - 1, ntraj)) if segments else None
    _lib().geodinvh_trajectory_lengths(C.c_longlong(ntraj), C.c_int(nt), lon.ctypes.data_as(_fp), lat.ctypes.data_as(_fp), C.c_double(dt),
                                      total.ctypes.data_as(_dp), *(None if o is None else o.ctypes.data_as(_dp) for o in (dist, speed)))
    return (total, dist, speed) if segments else total


def landing_error_m(azi1, s12, azi1_true, s12_true):
    """How far from point 2 the line (azi1, s12) from point 1 ends [m]: the error along the line and the error across it, which is
    the azimuth error [rad] times the reduced length -- at most a sin(s12 / a) on an ellipsoid this round, taken as that."""
    a = 6378137.0
    s12_true = np.asarray(s12_true, np.float64)
    daz = np.radians((np.asarray(azi1) - azi1_true + 180.0) % 360.0 - 180.0)
    across = np.abs(daz) * a * np.abs(np.sin(s12_true / a))
    return np.hypot(np.asarray(s12) - s12_true, across)
