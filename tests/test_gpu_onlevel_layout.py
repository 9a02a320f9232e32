"""GPU: the fused step launch with the C3 group's static slot layout on a step whose time sits on a reader level
(LayoutC3L1, csrc/odr_field.hip.h) computes what the launch that reads the layout from the group's descriptors computes, bit
for bit -- positions, status and the sampled environment -- and is the launch the host picks on those steps
(odr_particles_step_onlevel_stats).  The launch gathers slot A at both levels of the stages' bracket, so its stage samples
use the kept records instead of fetching them again: the same floats, the same arithmetic."""
import numpy as np
import pytest

import bench
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu
U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
W, DEPTH, LAND = 'upward_sea_water_velocity', 'sea_floor_depth_below_sea_level', 'land_binary_mask'


def _run(monkeypatch, runtime_layout, n=20000, steps=8):
    if runtime_layout:
        monkeypatch.setenv('ODR_NO_LAYOUT_SPEC', '1')
    else:
        monkeypatch.delenv('ODR_NO_LAYOUT_SPEC', raising=False)
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    fields = bench.make_fields('c3', small=True)      # synthetic.grid3d: levels 0, 3600, 7200 s
    wl = bench.Workload('c3', ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles('c3', fields, n, np.random.default_rng(5))
    P = ctx.particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    env, times = [], []
    for k in range(steps):   # bench.Workload.step's C3 call (RK4, coastline, sea floor, age, device-RNG mixing), without the re-sort
        t = wl.time_of(k)
        times.append(t)
        P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False,
                           seafloor=True, age_dt=wl.dt, vmix=dict(dt_mix=wl.dt_mix, step=k, vertical_advection=False))
        env.append({v: P.env_download(v).copy() for v in (U, V, W, DEPTH, LAND)})
    out = P.download(), env, P.step_layout_stats(), P.step_onlevel_stats(), times
    P.close()
    ctx.close()
    return out


def _equal(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_onlevel_static_layout_is_bit_identical_to_the_runtime_layout(monkeypatch):
    a, ea, sa, oa, times = _run(monkeypatch, runtime_layout=False)
    b, eb, sb, ob, _ = _run(monkeypatch, runtime_layout=True)
    # steps 0 (t = 0) and 6 (t = 3600 s) sit on a level: the on-level static launch, counted with the run-time one
    on_level = [k for k, t in enumerate(times) if t % 3600.0 == 0.0]
    assert on_level == [0, 6], times
    assert oa == 2 and sa == dict(runtime=2, static=6), (oa, sa)
    assert ob == 0 and sb == dict(runtime=8, static=0), (ob, sb)
    assert len(a['ID']) == len(b['ID'])
    for k in ('ID', 'lon', 'lat', 'z', 'status', 'moving'):
        assert _equal(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])), k
    for step, (x, y) in enumerate(zip(ea, eb)):
        for v in x:
            assert _equal(x[v], y[v]), (step, v)
