"""TEST INFRASTRUCTURE: host builds of the device headers.  tests/<name>.cpp includes headers of opendrift_amd/csrc and is compiled
with g++ for the CPU (tests/hostshim in place of the HIP runtime header) into oracle/_build/<name>.so; the *_host.py modules wrap
the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'opendrift_amd', 'csrc')
SHIM = os.path.join(HERE, 'hostshim')
_libs = {}


def host_lib(name, sources, flags=('-O1', '-ffp-contract=off'), shim=True):
    """The CDLL of oracle/_build/<name>.so, built from tests/<name>.cpp when it is older than that file, than any of `sources`
    (headers of opendrift_amd/csrc) or than the shim header."""
    if name not in _libs:
        out, src = os.path.join(ROOT, 'oracle', '_build', name + '.so'), os.path.join(HERE, name + '.cpp')
        deps = [src] + [os.path.join(CSRC, s) for s in sources] + ([os.path.join(SHIM, 'hip', 'hip_runtime.h')] if shim else [])
        if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            tmp = '%s.%d' % (out, os.getpid())      # (processes that test in parallel may build the same library)
            subprocess.check_call(['g++', '-std=c++17', *flags, *(['-I', SHIM] if shim else []), '-shared', '-fPIC', '-o', tmp, src])
            os.replace(tmp, out)
        _libs[name] = C.CDLL(out)
    return _libs[name]


def geod_host():
    """tests/geod_host.cpp: the float64 routines of csrc/odr_geodesic.hip.h."""
    return host_lib('geod_host', ('odr_geodesic.hip.h',), flags=('-O1', '-ffp-contract=off', '-w'))


def f32(a, n):
    """`a` as a writable contiguous float32 array of n elements of its own (a scalar is broadcast)."""
    return np.array(np.broadcast_to(np.asarray(a, np.float32), (n,)), dtype=np.float32, order='C')


def f64(a, n):
    return np.array(np.broadcast_to(np.asarray(a, np.float64), (n,)), dtype=np.float64, order='C')
