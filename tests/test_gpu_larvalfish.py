"""GPU: LarvalFish -- the two kernels (odr_larval_update, odr_larval_migrate) against the values the reference computed and
against the host build of the same header, and the model run end to end against the reference's own LarvalFish trajectories
(golden c27, tools/gen_golden_larvalfish.py)."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden
from opendrift_amd import readers
from opendrift_amd._abi import LARVA_PROPERTIES, OdrError
from opendrift_amd.larvalfish import LarvalFish

import larval_host
from test_larval_device_arithmetic import (DISPLACEMENT_MAX_ULP, DISPLACEMENT_SUM_SLACK_ULP, LENGTH_MAX_ULP, STAGE_MAX_ULP, STEPS, WEIGHT_MAX_ULP, bits,
                                           check_migration, check_update, golden_step, ulp_distance)

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
STAGE, HATCHED, LENGTH, WEIGHT = (LARVA_PROPERTIES.index(k) for k in ('stage_fraction', 'hatched', 'length', 'weight'))
NAMES = ['x_sea_water_velocity', 'y_sea_water_velocity', 'ocean_vertical_diffusivity', 'sea_floor_depth_below_sea_level',
         'land_binary_mask', 'sea_water_temperature', 'sea_water_salinity']


def _particles(ctx, T, stage, hatched, weight, length, z):
    n = len(T)
    P = ctx.particles(n)
    P.append(np.linspace(3, 4, n), np.full(n, 60.0), z=np.asarray(z, np.float64))
    P.env_upload('sea_water_temperature', np.ascontiguousarray(T, np.float32))
    for slot, v in ((STAGE, stage), (HATCHED, hatched), (WEIGHT, weight), (LENGTH, length)):
        P.set_property(slot, np.ascontiguousarray(v, np.float32))
    return P


def _props(P):
    return tuple(P.get_property(k) for k in (STAGE, HATCHED, WEIGHT, LENGTH))


def _both(ctx, T, stage, hatched, weight, length, z, f, dt, direction, length_for_migration=None):
    """update then migrate on the device and with the host build: ((s, h, w, L, z) device, the same of the host build,
    the host's float32 displacement).  length_for_migration: the length slot is replaced before the second launch."""
    P = _particles(ctx, T, stage, hatched, weight, length, z)
    P.larval_update(dt, STAGE, HATCHED, WEIGHT, LENGTH)
    dev = _props(P)
    hs, hh, hw, hL, _ = larval_host.update(T, dt, stage, hatched, weight, length)
    if length_for_migration is not None:
        P.set_property(LENGTH, np.ascontiguousarray(length_for_migration, np.float32))
    Lm = hL if length_for_migration is None else length_for_migration
    hm = hh if length_for_migration is None else None
    if hm is None:
        hm = P.get_property(HATCHED)
    P.larval_migrate(dt, f, direction, HATCHED, LENGTH)
    zd = P.download()['z']
    P.close()
    zh, disp = larval_host.migrate(hm, Lm, f, dt, direction, z)
    return dev + (zd,), (hs, hh, hw, hL, zh), disp


def _assert_bitwise(dev, host):
    for a, b in zip(dev[:4], host[:4]):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(dev[4], host[4])


@pytest.mark.parametrize('k', [1, 5], ids=['down', 'up'])
def test_kernels_reproduce_the_reference_and_the_host_build(ctx, k):
    """One step of each swimming direction, about 300 elements (the last wave partly filled, eggs and larvae in the same waves):
    the bounds of the CPU test of the host build (tests/test_larval_device_arithmetic.py) against the reference; device and host
    build agree bit for bit on every output.  Each launch runs from the reference's OWN input: between the two launches the
    length slot is uploaded again with the reference's length at its migration (the chain update -> migrate on the device's own
    length is what the run test covers)."""
    d = golden_step(golden('c27_larvalfish.npz'), k)
    assert d['direction'] == (-1 if k == 1 else 1) and len(d['env_T']) % 64 != 0
    # the reference's z before the migration is that of its own mixing: the update launch runs on the "before" arrays, the
    # migration launch on the reference's length after its update (mig_length) -- each launch from the reference's own input
    dev, host, disp = _both(ctx, d['env_T'], d['stage_fraction_before'], d['hatched_before'], d['weight_before'], d['length_before'],
                            d['mig_z_before'], d['f'], d['dt'], d['direction'], length_for_migration=d['mig_length'])
    ds, dw, dl = check_update(d, *dev[:4])
    dz = check_migration(d, dev[4], disp)
    print('step %d: device vs reference: stage_fraction %d ulp, weight %d ulp, length %d ulp, displacement %.2f ulp' % (k, ds, dw, dl, dz))
    assert ds <= STAGE_MAX_ULP and dw <= WEIGHT_MAX_ULP and dl <= LENGTH_MAX_ULP and dz <= DISPLACEMENT_MAX_ULP + DISPLACEMENT_SUM_SLACK_ULP
    _assert_bitwise(dev, host)


@pytest.mark.parametrize('n,kind', [(1, 'larva'), (65, 'larvae'), (64, 'eggs')])
def test_small_shapes_against_the_host_build(ctx, n, kind):
    rng = np.random.default_rng(n)
    T = rng.uniform(4, 12, n).astype(np.float32)
    z = rng.uniform(-3, -0.01, n)
    if kind == 'eggs':      # weight and length that would give NaN or infinity in the larval formulas
        hatched, weight, length = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        stage = rng.uniform(0, 0.9, n).astype(np.float32)
    else:
        hatched, length = np.ones(n, np.float32), np.zeros(n, np.float32)
        weight = np.exp(rng.uniform(np.log(0.08), np.log(50), n)).astype(np.float32)
        stage = np.ones(n, np.float32)
    dev, host, _ = _both(ctx, T, stage, hatched, weight, length, z, 0.4, 600.0, 1)
    _assert_bitwise(dev, host)
    if kind == 'eggs':      # nothing but stage_fraction is written
        assert np.array_equal(bits(dev[1]), bits(hatched)) and np.array_equal(bits(dev[2]), bits(weight))
        assert np.array_equal(bits(dev[3]), bits(length)) and np.array_equal(dev[4], z) and (dev[0] > stage).all()
    else:
        assert (dev[2] > weight).all() and (dev[3] > 4).all() and (dev[4] > z).all() and (dev[4] <= 0).all()
        assert np.array_equal(bits(dev[0]), bits(stage))


def test_entry_points_report_missing_state_and_bad_slots(ctx):
    n = 8
    P = ctx.particles(n)
    P.append(np.linspace(3, 4, n), np.full(n, 60.0), z=np.full(n, -2.0))
    for slot, v in ((STAGE, 0.5), (HATCHED, 1.0), (WEIGHT, 1.0)):
        P.set_property(slot, np.full(n, v, np.float32))
    with pytest.raises(OdrError, match='sea_water_temperature') as e:       # the temperature has not been sampled
        P.larval_update(600.0, STAGE, HATCHED, WEIGHT, LENGTH)
    assert e.value.code == -4                                               # ODR_ERR_STATE
    P.env_upload('sea_water_temperature', np.full(n, 8.0, np.float32))
    with pytest.raises(OdrError, match='slot %d' % LENGTH) as e:            # the length slot was never set
        P.larval_update(600.0, STAGE, HATCHED, WEIGHT, LENGTH)
    assert e.value.code == -4
    with pytest.raises(OdrError) as e:
        P.larval_migrate(600.0, 0.15, 1, HATCHED, LENGTH)
    assert e.value.code == -4
    P.set_property(LENGTH, np.zeros(n, np.float32))
    for bad in ((9, HATCHED, WEIGHT, LENGTH), (STAGE, -1, WEIGHT, LENGTH), (STAGE, HATCHED, WEIGHT, WEIGHT), (STAGE, STAGE, WEIGHT, LENGTH)):
        with pytest.raises(ValueError):                                     # out of [0, 9) or repeated
            P.larval_update(600.0, *bad)
    for bad in ((9, LENGTH), (HATCHED, HATCHED)):
        with pytest.raises(ValueError):
            P.larval_migrate(600.0, 0.15, 1, *bad)
    with pytest.raises(ValueError):
        P.larval_migrate(600.0, 0.15, 0, HATCHED, LENGTH)                   # direction is +1 or -1
    P.larval_update(600.0, STAGE, HATCHED, WEIGHT, LENGTH)
    P.larval_migrate(600.0, 0.15, -1, HATCHED, LENGTH)
    assert (P.get_property(LENGTH) > 4).all() and (P.download()['z'] < -2.0).all()
    P.close()


def _final(o, n):
    out = {k: np.full(n, np.nan) for k in ('lon', 'lat', 'z')}
    out['status'] = np.full(n, -1)
    for k in LARVA_PROPERTIES:
        out[k] = np.full(n, np.nan, np.float32)
    for d in (o.elements, o.elements_deactivated):
        for k in ('lon', 'lat', 'z', 'status'):
            out[k][d.ID] = getattr(d, k)
    e = o.elements
    for k in LARVA_PROPERTIES:
        out[k][e.ID] = getattr(e, k)
    return out


def test_run_numpy_rng_reproduces_the_reference_trajectories():
    """rng='numpy': np.random is drawn in the reference's call order (random(n) once per mixing sub-step), so the run reproduces
    the reference's trajectories at the tolerances of the PelagicEggDrift run test; the properties within steps x the
    single-step bound (the errors of successive steps add, the growth factor of a step is close to 1)."""
    g = golden('c27_larvalfish.npz')
    start = T0 + timedelta(seconds=float(g['start_seconds']))
    times = [start + timedelta(seconds=float(t)) for t in g['g_t']]
    o = LarvalFish(loglevel=50, seed=0, rng='numpy')
    o.add_reader(readers.GridReader(g['g_x'], g['g_y'], times, {k: g['g_' + k] for k in NAMES}, z=g['g_z']))
    for k in g.files:
        if k.startswith('c_'):
            o.set_config('environment:constant:' + k[2:], float(g[k]))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('vertical_mixing:timestep', 60)
    o.set_config('IBM:fraction_of_timestep_swimming', float(g['fraction_of_timestep_swimming']))
    n = g['lon'].shape[1]
    o.seed_elements(lon=g['lon'][0], lat=g['lat'][0], z=g['z'][0], time=start, diameter=g['diameter'],
                    neutral_buoyancy_salinity=g['neutral_buoyancy_salinity'], stage_fraction=g['seed_stage_fraction'],
                    hatched=g['seed_hatched'], weight=g['seed_weight'], length=g['seed_length'])
    res = o.run(time_step=600, steps=STEPS)
    assert o.steps_calculation == STEPS
    f = _final(o, n)
    active = g['status'][-1] == 0
    last = STEPS - 1
    assert np.array_equal(active, g['hatched_after'][last] >= 0)
    dlon, dlat, dz = (np.abs(f[k] - g[k][-1]).max() for k in ('lon', 'lat', 'z'))
    ds = ulp_distance(f['stage_fraction'][active], g['stage_fraction_after'][last][active]).max()
    dw = ulp_distance(f['weight'][active], g['weight_after'][last][active]).max()
    dl = ulp_distance(f['length'][active], g['length_after'][last][active]).max()
    print('largest differences: lon %.3g lat %.3g deg, z %.3g m; stage_fraction %d ulp, weight %d ulp, length %d ulp; %d larvae, '
          '%d of them at z = 0' % (dlon, dlat, dz, ds, dw, dl, (f['hatched'][active] == 1).sum(),
                                  ((f['hatched'] == 1) & (f['z'] == 0))[active].sum()))
    assert np.array_equal(f['status'], g['status'][-1])
    assert np.array_equal(f['hatched'][active], g['hatched_after'][last][active].astype(np.float32))
    assert dlon < 1e-7 and dlat < 1e-7 and dz < 1e-5
    assert ds <= STEPS * STAGE_MAX_ULP and dw <= STEPS * WEIGHT_MAX_ULP and dl <= STEPS * LENGTH_MAX_ULP
    assert np.array_equal((f['z'] == 0)[active], (g['z'][-1] == 0)[active])
    e = o.elements
    for k in LARVA_PROPERTIES + ['terminal_velocity']:
        assert getattr(e, k).dtype == np.float32
        assert res[k].dtype == np.float32 and res[k].shape == (n, STEPS + 1)
    assert np.array_equal(e.diameter, g['diameter'][e.ID]) and (e.survival == 1).all()
    assert np.array_equal(res['hatched'][active, -1], f['hatched'][active])


def test_stokes_profile_of_a_submerged_population_takes_its_period_from_the_wind():
    """The reference forms the wave period (and the wave height, where none is given) from the wind of EVERY element
    (physics_methods.py:893-943).  No element within wind_drift_depth of the surface: the Stokes drift of the submerged
    elements is the same as with one more element at the surface, and not that of the 'no wind' period of 8 s."""
    def run(z, wind):
        o = LarvalFish(loglevel=50, seed=0)
        for k, v in (('land_binary_mask', 0), ('sea_surface_wave_stokes_drift_x_velocity', 0.03),
                     ('sea_surface_wave_stokes_drift_y_velocity', 0.01), ('x_wind', wind), ('y_wind', 0.0)):
            o.set_config('environment:constant:' + k, v)
        o.set_config('drift:vertical_mixing', False)
        n = len(z)
        o.seed_elements(lon=np.linspace(4.0, 4.1, n), lat=np.full(n, 60.0), z=np.asarray(z, np.float64), time=T0)      # eggs: no swimming
        o.run(time_step=600, steps=2)
        e = o.elements
        assert np.array_equal(e.z, z)
        return e.lon - np.linspace(4.0, 4.1, n), e.lat - 60.0
    deep = [-2.0, -3.0, -5.0, -8.0]
    a, b, calm = run(deep, 6.0), run(deep + [0.0], 6.0), run(deep, 0.0)
    assert np.abs(a[1] - b[1][:4]).max() < 1e-12        # (the northward displacement: the seeded longitudes differ between the two)
    assert (a[1] > 0).all() and (np.diff(a[1]) < 0).all()                     # decays with depth
    assert np.abs(a[1] - calm[1]).max() > 0.05 * a[1].max()                   # the period matters at these depths
