"""GPU: PelagicEggDrift -- the terminal-velocity kernel (odr_egg_terminal_velocity) against the values the reference computed,
and the model run end to end against the reference's own PelagicEggDrift trajectories (golden c25,
tools/gen_golden_pelagicegg.py)."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden
from opendrift_amd import readers, synthetic as synth
from opendrift_amd._abi import OdrError
from opendrift_amd.oceandrift import OceanDrift
from opendrift_amd.pelagicegg import PelagicEggDrift

import egg_host
from test_egg_device_arithmetic import HIGH_RE_MAX_ULP, golden_inputs, ulp_distance

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
NAMES = ['x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity', 'ocean_vertical_diffusivity',
         'sea_floor_depth_below_sea_level', 'land_binary_mask', 'sea_water_temperature', 'sea_water_salinity']


def _launch(ctx, T, S, d, s):
    n = len(T)
    P = ctx.particles(n)
    P.append(np.linspace(3, 4, n), np.full(n, 60.0))
    P.env_upload('sea_water_temperature', T)
    P.env_upload('sea_water_salinity', S)
    P.set_property(0, d)
    P.set_property(1, s)
    P.egg_terminal_velocity(0, 1)
    w = P.download_f32('terminal_velocity')
    P.close()
    return w


@pytest.mark.parametrize('prefix', ['', 'k_'], ids=['celsius', 'kelvin_reader'])
def test_kernel_reproduces_the_reference_and_the_host_build(ctx, prefix):
    """Same bounds as the CPU test of the host build (tests/test_egg_device_arithmetic.py): Stokes branch and branch choice bit
    for bit, high-Reynolds branch within HIGH_RE_MAX_ULP of the reference; device and host build agree bit for bit."""
    T, S, d, s, want, want_high = golden_inputs(golden('c25_pelagicegg.npz'), prefix)
    got = _launch(ctx, T, S, d, s)
    host, high = egg_host.terminal_velocity(T, S, d, s)
    assert np.array_equal(high, want_high)
    assert np.array_equal(got[~high].view(np.uint32), want[~high].view(np.uint32))
    dist = ulp_distance(got[high], want[high])
    print('high-Reynolds branch: largest distance to the reference %d ulp' % dist.max())
    assert dist.max() <= HIGH_RE_MAX_ULP
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))


def test_entry_reports_missing_temperature_and_salinity(ctx):
    P = ctx.particles(8)
    P.append(np.linspace(3, 4, 8), np.full(8, 60.0))
    P.set_property(0, np.full(8, 0.0014, np.float32))
    P.set_property(1, np.full(8, 31.25, np.float32))
    with pytest.raises(OdrError, match='sea_water_temperature') as e:
        P.egg_terminal_velocity(0, 1)
    assert e.value.code == -4                               # ODR_ERR_STATE
    P.env_upload('sea_water_temperature', np.full(8, 8.0, np.float32))
    with pytest.raises(OdrError) as e:                      # salinity still missing
        P.egg_terminal_velocity(0, 1)
    assert e.value.code == -4
    P.env_upload('sea_water_salinity', np.full(8, 34.0, np.float32))
    with pytest.raises(OdrError) as e:                      # a property slot that was never set
        P.egg_terminal_velocity(0, 2)
    assert e.value.code == -4
    with pytest.raises(ValueError):
        P.egg_terminal_velocity(0, 9)
    P.egg_terminal_velocity(0, 1)
    assert (P.download_f32('terminal_velocity') > 0).all()  # a cod egg in 34 psu water rises
    P.close()


def _reader(g, kelvin=False):
    times = [T0 + timedelta(seconds=float(t)) for t in g['g_t']]
    arrays = {k: g['g_' + k] for k in NAMES}
    if kelvin:      # as tools/gen_golden_pelagicegg.py forms the Kelvin field
        arrays['sea_water_temperature'] = (arrays['sea_water_temperature'].astype(np.float64) + 273.15).astype(np.float32)
    return readers.GridReader(g['g_x'], g['g_y'], times, arrays, z=g['g_z'])


def _final(o, n):
    lon, lat, z, status = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1)
    for d in (o.elements, o.elements_deactivated):
        lon[d.ID], lat[d.ID], z[d.ID], status[d.ID] = d.lon, d.lat, d.z, d.status
    return lon, lat, z, status


@pytest.mark.parametrize('prefix,steps', [('', 8), ('k_', 3)], ids=['celsius', 'kelvin_reader'])
def test_run_numpy_rng_reproduces_the_reference_trajectories(prefix, steps):
    """rng='numpy': np.random is drawn in the reference's call order (random(n) once per mixing sub-step), so the run
    reproduces the reference's trajectories at the tolerances of the C3 model test (tests/test_gpu_model_api.py)."""
    g = golden('c25_pelagicegg.npz')
    o = PelagicEggDrift(loglevel=50, seed=0, rng='numpy')
    o.add_reader(_reader(g, kelvin=prefix == 'k_'))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('vertical_mixing:timestep', 60)
    n = g[prefix + 'lon'].shape[1]
    o.seed_elements(lon=g[prefix + 'lon'][0], lat=g[prefix + 'lat'][0], z=g[prefix + 'z'][0], time=T0,
                    diameter=g[prefix + 'diameter'], neutral_buoyancy_salinity=g[prefix + 'neutral_buoyancy_salinity'])
    res = o.run(time_step=600, steps=steps)
    assert o.steps_calculation == steps
    lon, lat, z, status = _final(o, n)
    print('largest differences: lon %.3g lat %.3g deg, z %.3g m' % (np.abs(lon - g[prefix + 'lon'][-1]).max(),
                                                                  np.abs(lat - g[prefix + 'lat'][-1]).max(),
                                                                  np.abs(z - g[prefix + 'z'][-1]).max()))
    assert np.abs(lon - g[prefix + 'lon'][-1]).max() < 1e-7 and np.abs(lat - g[prefix + 'lat'][-1]).max() < 1e-7
    assert np.abs(z - g[prefix + 'z'][-1]).max() < 1e-5
    assert np.array_equal(status, g[prefix + 'status'][-1])
    # the properties are element variables of the model and of its result; the four variables without a device id are not
    e = o.elements
    assert e.diameter.dtype == np.float32 and np.array_equal(e.diameter, g[prefix + 'diameter'][e.ID])
    assert e.terminal_velocity.dtype == np.float32 and (e.hatched == 0).all() and (e.density == 1028).all()
    for k in ('diameter', 'neutral_buoyancy_salinity', 'density', 'hatched', 'terminal_velocity', 'sea_water_temperature'):
        assert res[k].dtype == np.float32 and res[k].shape == (n, steps + 1)
    assert 'turbulent_kinetic_energy' not in res
    assert (np.asarray(o.environment.sea_water_temperature) < 100).all()


def _device_run(cls, n=3000, steps=6, seed=3, salinity=None, **kw):
    g = golden('c25_pelagicegg.npz')
    o = cls(loglevel=50, seed=seed, rng='device')
    o.add_reader(_reader(g))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('drift:vertical_mixing', True)
    o.set_config('drift:vertical_mixing_at_surface', True)
    o.set_config('drift:vertical_advection_at_surface', True)
    o.set_config('general:coastline_action', 'previous')
    o.set_config('vertical_mixing:timestep', 60)
    rng = np.random.default_rng(7)
    x, y = g['g_x'], g['g_y']
    lon, lat, z = rng.uniform(x[6], x[-12], n), rng.uniform(y[6], y[-7], n), rng.uniform(-40, -10, n)
    if salinity is not None:
        kw['neutral_buoyancy_salinity'] = salinity
    o.seed_elements(lon=lon, lat=lat, z=z, time=T0, **kw)
    o.run(time_step=600, steps=steps)
    return o, _final(o, n)


def test_device_rng_is_reproducible_and_the_buoyancy_acts():
    a, fa = _device_run(PelagicEggDrift)
    b, fb = _device_run(PelagicEggDrift)
    for u, v in zip(fa, fb):
        assert np.array_equal(u, v, equal_nan=True)
    c, fc = _device_run(OceanDrift)          # the same fields, mixing and draws (keyed by element ID), no buoyancy
    assert np.array_equal(fa[3], fc[3])
    assert np.abs(fa[2] - fc[2]).max() > 0.1 and (a.elements.terminal_velocity != 0).any() and (c.elements.terminal_velocity == 0).all()


def test_light_eggs_rise_and_heavy_eggs_sink():
    """neutral_buoyancy_salinity far below the ambient salinity (32 - 35.5): the egg is lighter than the water and ends above
    a control group that is neutrally buoyant at about the ambient salinity; far above: below it."""
    n = 3000
    sal = np.repeat(np.float32([20.0, 34.0, 50.0]), n // 3)
    o, (lon, lat, z, status) = _device_run(PelagicEggDrift, n=n, salinity=sal)
    ok = status == 0
    light, control, heavy = (z[ok & (sal == s)].mean() for s in (20.0, 34.0, 50.0))
    print('mean z: light %.2f, control %.2f, heavy %.2f m' % (light, control, heavy))
    assert light > control + 5 and heavy < control - 5


def test_properties_survive_compaction_and_the_periodic_sort():
    """More elements than the re-sort threshold of run(), a re-sort every second step, a coast to strand on and a domain to
    leave: every element still present carries the diameter it was seeded with."""
    n = 80000
    g = synth.grid3d(nx=48, ny=40, nz=8, nt=3, seed=1)
    X, Y = np.meshgrid(np.linspace(0, 1, 48), np.linspace(0, 1, 40))
    shape = g['x_sea_water_velocity'].shape
    g['sea_water_temperature'] = np.broadcast_to((6 + 4 * Y).astype(np.float32), shape).copy()
    g['sea_water_salinity'] = np.broadcast_to((32 + 3 * X).astype(np.float32), shape).copy()
    times = [T0 + timedelta(seconds=float(t)) for t in g['t']]
    o = PelagicEggDrift(loglevel=50, seed=1, rng='device')
    o.add_reader(readers.GridReader(g['x'], g['y'], times, {k: g[k] for k in NAMES}, z=g['z']))
    o.set_config('drift:advection_scheme', 'euler')
    o.set_config('general:coastline_action', 'stranding')
    o.set_config('environment:fallback:x_sea_water_velocity', None)      # leaving the reader's domain: missing data
    o.set_config('environment:fallback:y_sea_water_velocity', None)
    o.sort_every = 2
    rng = np.random.default_rng(5)
    lon, lat = rng.uniform(g['x'][0], g['x'][-4], n), rng.uniform(g['y'][0], g['y'][-1], n)
    diameter = rng.uniform(0.001, 0.003, n).astype(np.float32)
    o.seed_elements(lon=lon, lat=lat, z=rng.uniform(-30, -1, n), time=T0, diameter=diameter)
    o.run(time_step=900, steps=6)
    e = o.elements
    gone = o.num_elements_deactivated()
    print('deactivated', gone, 'categories', o.status_categories)
    assert gone > 0 and len(e.ID) + gone == n and len(e.ID) > 65536
    assert not (np.diff(o.P.ids()) > 0).all()                # the device order is no longer the seeding order
    assert np.array_equal(e.diameter, diameter[e.ID])
    assert (e.neutral_buoyancy_salinity == np.float32(31.25)).all() and (e.density == 1028).all()
    assert np.isfinite(e.terminal_velocity).all() and (e.terminal_velocity != 0).any()
