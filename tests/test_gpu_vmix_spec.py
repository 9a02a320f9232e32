"""GPU: the K-column mixing launch with C3's configuration as compile-time constants (k_vmix_col<..., VMixC3>,
csrc/odr_kernels.hip.h) computes what the launch that reads the configuration at run time computes, bit for bit -- positions,
status, moving -- and is the launch the host picks for C3's calls (odr_particles_vmix_layout_stats).  A call that differs from
that configuration in one setting (host-drawn numbers, a level cut, another sea-floor action) keeps the run-time launch."""
import numpy as np
import pytest

import bench
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu


def _fields(nz):
    f = bench.make_fields('c3', small=True)            # 8 levels
    if nz != 8:                                         # the full-size C3 field's level count on the small grid
        f = dict(f, g=synth.grid3d(nx=128, ny=96, nz=nz, nt=3, seed=0))
        f['z'] = f['g']['z']
    return f


def _run(monkeypatch, runtime, nz=8, variant=None, n=20000, steps=4):
    if runtime:
        monkeypatch.setenv('ODR_NO_VMIX_SPEC', '1')
    else:
        monkeypatch.delenv('ODR_NO_VMIX_SPEC', raising=False)
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    if variant == 'seafloor':
        ctx.set_seafloor_action('deactivate', status_code=3)
    fields = _fields(nz)
    wl = bench.Workload('c3', ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles('c3', fields, n, np.random.default_rng(3))
    P = ctx.particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    ntimes = int(wl.dt / wl.dt_mix)
    for k in range(steps):
        t = wl.time_of(k)
        if variant is None and k % 2 == 0:   # bench.Workload.step's one-call form: the step launch, then the mixing launch
            P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False,
                               seafloor=True, age_dt=wl.dt, vmix=dict(dt_mix=wl.dt_mix, step=k, vertical_advection=False))
            continue
        P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False,
                           seafloor=True, age_dt=wl.dt)
        if variant is None:                  # its guarded form (OceanDrift.run() between output times)
            assert P.scan_status_begin()
            ok = P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False, guarded=True)
            kept, _ = P.scan_status_end()
            P.compact_apply()
            if not (ok and kept == len(P)):
                P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False)
        elif variant == 'host_rng':
            u = np.random.default_rng(10 + k).random((ntimes, len(P)))
            P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False, uniforms=u)
        elif variant == 'cut':
            P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False, profile_levels=5)
        else:
            P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False)
    return P.download(), P.vmix_layout_stats()


def _same(a, b):
    assert len(a['ID']) == len(b['ID'])
    for k in ('ID', 'lon', 'lat', 'z', 'status', 'moving'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


@pytest.mark.parametrize('nz', [8, 12])
def test_static_c3_mixing_is_bit_identical_to_the_runtime_configuration(monkeypatch, nz):
    a, sa = _run(monkeypatch, runtime=False, nz=nz)
    b, sb = _run(monkeypatch, runtime=True, nz=nz)
    # step 0 samples on a time level (one K level: TL = false), steps 1-3 between two; steps 1 and 3 guarded (a guarded launch
    # whose verdict is "not all stay" is followed by the unguarded one: launches >= steps)
    assert sa['static'] >= 4 and sa['runtime'] == 0 and sa['other'] == 0, sa
    assert sb['runtime'] == sa['static'] and sb['static'] == 0 and sb['other'] == 0, sb
    _same(a, b)
    assert not np.array_equal(a['z'], bench.seed_particles('c3', _fields(nz), 20000, np.random.default_rng(3))[2][a['ID']])


@pytest.mark.parametrize('variant,expect', [('host_rng', dict(runtime=4, static=0, other=0)),
                                            ('cut', dict(runtime=0, static=0, other=4)),
                                            ('seafloor', dict(runtime=4, static=0, other=0))])
def test_other_configurations_keep_the_runtime_launch(monkeypatch, variant, expect):
    a, sa = _run(monkeypatch, runtime=False, variant=variant)
    b, sb = _run(monkeypatch, runtime=True, variant=variant)
    assert sa == expect, sa
    assert sb == expect, sb
    _same(a, b)
