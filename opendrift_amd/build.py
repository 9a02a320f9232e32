"""Builds libodrift_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU).

The library is one translation unit per csrc/*.hip, compiled in parallel and linked into one shared object; an object is
rebuilt when its source, any csrc/*.h or include/odrift.h changed."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
UNITS = sorted(f for f in os.listdir(CSRC) if f.endswith('.hip'))
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')) + \
    [os.path.join(os.path.dirname(HERE), 'include', 'odrift.h')]
LIB = os.path.join(HERE, 'libodrift_hip.so')
OBJDIR = os.path.join(HERE, 'build')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC',
         '-I' + os.path.join(os.path.dirname(HERE), 'include')]
# per-unit flags.  odr_mix.hip: k_vmix_col runs a thread's particle routine in a loop over the passes of its tile; the machine
# LICM pass moves the routine's literal constants and address forms out of that loop into vector registers -- it budgets against
# the register file, not against the 80 registers of the launch bounds -- and the allocator then spills them (100 .. 1 300 bytes
# of scratch memory per lane).  Without the pass every instantiation fits (tests/test_vmix_skip_resources.py).
UNIT_FLAGS = {'odr_mix.hip': ['-mllvm', '-disable-machine-licm']}


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)


def build(force=False, verbose=False, extra_flags=(), lib=LIB, objdir=OBJDIR):
    """extra_flags / lib / objdir: A/B builds of the same sources (tools/vbuild.sh)."""
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for u in UNITS:
        src = os.path.join(CSRC, u)
        obj = os.path.join(objdir, u.replace('.hip', '.o'))
        if force or _stale(obj, [src] + HEADERS):
            jobs.append([HIPCC] + FLAGS + UNIT_FLAGS.get(u, []) + list(extra_flags) + ['-c', src, '-o', obj])
    if jobs:
        def run(cmd):
            if verbose:
                print(' '.join(cmd))
            subprocess.check_call(cmd)
        with ThreadPoolExecutor(len(jobs)) as ex:
            list(ex.map(run, jobs))
    objs = [os.path.join(objdir, u.replace('.hip', '.o')) for u in UNITS]
    if jobs or _stale(lib, objs):
        cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs
        if verbose:
            print(' '.join(cmd))
        subprocess.check_call(cmd)
    return lib


if __name__ == '__main__':
    import sys
    print(build(force='--force' in sys.argv, verbose=True))


def build_variant(tag, units, extra_flags, outdir=None):
    """A/B library tools/_lib<tag>.so: only `units` are compiled with `extra_flags`, the other translation units are the
    default build's objects (tools/vbuild_tu.sh; a what-if flag usually touches one kernel family)."""
    build()
    outdir = outdir or os.path.join(os.path.dirname(HERE), 'tools')
    objdir = os.path.join(outdir, '_obj' + tag)
    os.makedirs(objdir, exist_ok=True)

    def run(u):
        obj = os.path.join(objdir, u.replace('.hip', '.o'))
        subprocess.check_call([HIPCC] + FLAGS + UNIT_FLAGS.get(u, []) + list(extra_flags) + ['-c', os.path.join(CSRC, u), '-o', obj])
        return obj
    with ThreadPoolExecutor(len(units)) as ex:
        mine = dict(zip(units, ex.map(run, units)))
    objs = [mine.get(u, os.path.join(OBJDIR, u.replace('.hip', '.o'))) for u in UNITS]
    lib = os.path.join(outdir, '_lib%s.so' % tag)
    subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs)
    return lib
