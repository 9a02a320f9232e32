"""GPU: the fused step launch with the C3 group's slot layout as compile-time constants (LayoutC3, csrc/odr_field.hip.h)
computes what the launch that reads the layout from the group's descriptors computes, bit for bit -- positions, status and
the sampled environment -- and is the launch the host picks for that group (odr_particles_step_layout_stats)."""
import numpy as np
import pytest

import bench
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu
U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
W, DEPTH, LAND = 'upward_sea_water_velocity', 'sea_floor_depth_below_sea_level', 'land_binary_mask'


def _run(monkeypatch, runtime_layout, n=20000, steps=4):
    if runtime_layout:
        monkeypatch.setenv('ODR_NO_LAYOUT_SPEC', '1')
    else:
        monkeypatch.delenv('ODR_NO_LAYOUT_SPEC', raising=False)
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    fields = bench.make_fields('c3', small=True)      # synthetic.grid3d, content ids for the static 2-D fields
    wl = bench.Workload('c3', ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles('c3', fields, n, np.random.default_rng(3))
    P = ctx.particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    env = []
    for k in range(steps):   # bench.Workload.step's C3 call (RK4, coastline, sea floor, age, device-RNG mixing), without the re-sort
        P.env_coast_advect(wl.vars, wl.time_of(k), wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False,
                           seafloor=True, age_dt=wl.dt, vmix=dict(dt_mix=wl.dt_mix, step=k, vertical_advection=False))
        env.append({v: P.env_download(v).copy() for v in (U, V, W, DEPTH, LAND)})
    return P.download(), env, P.step_layout_stats()


def _equal(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_static_c3_layout_is_bit_identical_to_the_runtime_layout(monkeypatch):
    a, ea, sa = _run(monkeypatch, runtime_layout=False)
    b, eb, sb = _run(monkeypatch, runtime_layout=True)
    # step 0 samples on a time level (one level: no static-slot bits, not the C3 layout); steps 1-3 between two levels
    assert sa == dict(runtime=1, static=3), sa
    assert sb == dict(runtime=4, static=0), sb
    assert len(a['ID']) == len(b['ID'])
    for k in ('ID', 'lon', 'lat', 'z', 'status', 'moving'):
        assert _equal(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])), k
    for step, (x, y) in enumerate(zip(ea, eb)):
        for v in x:
            assert _equal(x[v], y[v]), (step, v)
