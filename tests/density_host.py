"""TEST INFRASTRUCTURE: ctypes access to the bin search and the classification of opendrift_amd/csrc/odr_density.hip.h compiled for
the host (g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see density_host.cpp; the NumPy restatement of
get_density_array's contract that the tests compare with; and the error bound of a weighted map."""
import ctypes as C

import numpy as np

from host_build import host_lib

_fp, _dp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)


def _lib():
    return host_lib('density_host', ('odr_density.hip.h',))


def bins(v, edges):
    """The header's bin of every float64 value (-1: dropped)."""
    v, edges = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(edges, np.float64)
    out = np.empty(len(v), np.int32)
    _lib().densh_bin(C.c_longlong(len(v)), v.ctypes.data_as(_dp), C.c_int(len(edges)), edges.ctypes.data_as(_dp), out.ctypes.data_as(_ip))
    return out


def classes(z, status, stranded_code):
    """Bit 0: counts in H, bit 1: in H_submerged, bit 2: in H_stranded."""
    z, status = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(status, np.float32)
    out = np.empty(len(z), np.int32)
    _lib().densh_classes(C.c_longlong(len(z)), z.ctypes.data_as(_fp), status.ctypes.data_as(_fp), C.c_int(stranded_code), out.ctypes.data_as(_ip))
    return out


def density_map(lon, lat, z, status, lon_edges, lat_edges, weight=None, stranded_code=-1):
    """The signature of opendrift_amd.device.Context.density_map, computed by the host build of the header."""
    arrs = [np.ascontiguousarray(a, np.float32) for a in (lon, lat, z, status)]
    w = None if weight is None else np.ascontiguousarray(weight, np.float32)
    ntraj, nt = arrs[0].shape
    le, la = np.ascontiguousarray(lon_edges, np.float64), np.ascontiguousarray(lat_edges, np.float64)
    out = [np.zeros((nt, len(le) - 1, len(la) - 1)) for _ in range(3)]
    _lib().densh_map(C.c_longlong(ntraj), C.c_int(nt), *(a.ctypes.data_as(_fp) for a in arrs), w.ctypes.data_as(_fp) if w is not None else None,
                    C.c_int(stranded_code), C.c_int(len(le)), le.ctypes.data_as(_dp), C.c_int(len(la)), la.ctypes.data_as(_dp),
                    *(o.ctypes.data_as(_dp) for o in out))
    return tuple(out)


def searchsorted_bins(v, edges):
    """np.histogram2d's bin of every value, restated: searchsorted(edges, v, side='right') - 1, a value equal to the last edge in the
    last bin, NaN and everything outside dropped (-1)."""
    v, edges = np.asarray(v, np.float64), np.asarray(edges, np.float64)
    b = np.searchsorted(edges, v, side='right') - 1
    b[v == edges[-1]] = len(edges) - 2
    b[~((v >= edges[0]) & (v <= edges[-1]))] = -1
    return b.astype(np.int32)


def histogram2d_maps(lon, lat, z, status, lon_edges, lat_edges, weight=None, stranded_code=-1):
    """get_density_array's three maps with np.histogram2d itself, per the contract: [trajectory, time] inputs, masked entries moved
    to 1000 as in the reference (basemodel/__init__.py:4110-4144)."""
    lon, lat, z, status = (np.asarray(a, np.float32).T for a in (lon, lat, z, status))
    nt = lon.shape[0]
    out = [np.zeros((nt, len(lon_edges) - 1, len(lat_edges) - 1)) for _ in range(3)]
    masks = [z < 0, z >= 0, (status != stranded_code) if stranded_code >= 0 else None]
    for h, mask in zip(out, masks):
        if mask is None:
            continue
        lo, la = lon.copy(), lat.copy()
        lo[mask] = 1000
        la[mask] = 1000
        for i in range(nt):
            h[i] = np.histogram2d(lo[i], la[i], weights=None if weight is None else np.asarray(weight, np.float32).T[i],
                                  bins=(lon_edges, lat_edges))[0]
    return tuple(out)


def weighted_bound(lon, lat, z, status, lon_edges, lat_edges, weight, stranded_code=-1):
    """Per bin of the three weighted maps: 2 (k - 1) 2^-53 sum|w|, k the entries of the bin and sum|w| the sum of their |weights|,
    both from the inputs -- twice the bound of one recursive float64 summation, since either side of a comparison carries one."""
    k = density_map(lon, lat, z, status, lon_edges, lat_edges, None, stranded_code)
    s = density_map(lon, lat, z, status, lon_edges, lat_edges, np.abs(np.asarray(weight, np.float32)), stranded_code)
    return tuple(2.0 * np.maximum(kk - 1.0, 0.0) * 2.0 ** -53 * ss for kk, ss in zip(k, s))
