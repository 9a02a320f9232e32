"""TEST INFRASTRUCTURE: ctypes access to the routines of opendrift_amd/csrc/odr_convolve.hip.h compiled for the host (g++
-ffp-contract=off, tests/hostshim in place of the HIP runtime header), see convolve_host.cpp; the loader of golden C41 and the
comparison of a prepared level with a convolved block that the CPU and the GPU tests share."""
import ctypes as C
import os

import numpy as np

from host_build import host_lib

_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c41_reader_convolution.npz')


def _lib():
    return host_lib('convolve_host', ('odr_convolve.hip.h',))


def max_edge():
    return int(_lib().convh_max_edge())


def tile_edge():
    return int(_lib().convh_tile_edge())


def strip():
    return int(_lib().convh_strip())


def convolve(a, kernel):
    """The header's convolution of one float32 variable, [ny, nx] (over y, x) or [nz, ny, nx] (over z, y), tile by tile and strip by
    strip as the kernels walk it."""
    a = np.ascontiguousarray(a, np.float32)
    w = np.ascontiguousarray(kernel, np.float64)
    out = np.full(a.shape, -777.0, np.float32)
    if a.ndim == 2:
        _lib().convh_2d(a.ctypes.data_as(_fp), out.ctypes.data_as(_fp), C.c_int(a.shape[0]), C.c_int(a.shape[1]), C.c_int(w.shape[0]),
                        C.c_int(w.shape[1]), w.ctypes.data_as(_dp))
    else:
        _lib().convh_3d(a.ctypes.data_as(_fp), out.ctypes.data_as(_fp), C.c_int(a.shape[0]), C.c_int(a.shape[1]), C.c_int(a.shape[2]),
                        C.c_int(w.shape[0]), C.c_int(w.shape[1]), w.ctypes.data_as(_dp))
    return out


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def block_cases():
    """Part (a) of the golden: [(name, kernel argument of set_convolution_kernel, {variable: raw array}, {variable: the reference's
    convolved array})]."""
    g = golden()
    out = []
    for name in [str(s) for s in g['a_cases']]:
        k = g['a_%s_kernel' % name]
        conv = int(k) if k.ndim == 0 else k
        vs = [str(s) for s in g['a_%s_vars' % name]]
        out.append((name, conv, {v: g['a_%s_raw_%s' % (name, v)] for v in vs}, {v: g['a_%s_out_%s' % (name, v)] for v in vs}))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Equal bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8)))


def masked(conv):
    """What ReaderBlock.__init__ makes of a convolved array before anything is filled: |v| > 1e9 and non-finite values are NaN."""
    c = np.array(conv, np.float32)
    with np.errstate(invalid='ignore'):
        c[~np.isfinite(c) | (np.abs(c) > 1e9)] = np.nan
    return c


def assert_prepared_equals(prepared, conv, what=''):
    """A level read back from the device against the reference's convolved block: wherever the convolved and then masked value is
    finite the level holds its bits (the sea-floor fill and the dilation only give values to NaN cells)."""
    want = masked(conv)
    ok = np.isfinite(want)
    assert ok.any(), what
    assert prepared.shape == want.shape, (what, prepared.shape, want.shape)
    bad = bits(prepared)[ok] != bits(want)[ok]
    assert not bad.any(), '%s: %d of %d finite cells differ, first %r' % (what, bad.sum(), ok.sum(), np.argwhere(bits(prepared) != bits(want))[:3])
