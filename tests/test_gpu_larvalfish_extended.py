"""GPU: LarvalFishExtended -- the three entry points (odr_solar_elevation, odr_larvalx_hatch, odr_larvalx_behave) against the host
build of the same headers on random inputs, and the model run end to end against the reference's own LarvalFishExtended
trajectories (golden c31, tools/gen_golden_larvalfish_extended.py).

Bounds of the run, MEASURED on the MI355X against the golden at the end of its 48 steps and multiplied by four (DESIGN.md
section 7h): lon 1.32e-9 deg, lat 1.72e-9 deg -- the 48 Euler steps of the advection launch, the same in every case -- and z 0 m:
z is bit for bit in all four cases, with the vertical mixing on its recorded draws (case A) and in the float32 the reference
holds z in without mixing (B, C, D).  hatched is identical in every step of every case, stage_fraction at the end bit for bit."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden
from opendrift_amd import readers
from opendrift_amd._abi import LARVALX_PROPERTIES, OdrError
from opendrift_amd.larvalfish_extended import LarvalFishExtended
from opendrift_amd.oceandrift import OceanDrift, solar_time_scalars

import larvalx_host
from test_larvalx_device_arithmetic import CASES, ELEVATION_MAX_DEG, T0, bits, bits64, config

pytestmark = pytest.mark.gpu
STAGE, HATCHED = (LARVALX_PROPERTIES.index(k) for k in ('stage_fraction', 'hatched'))
NAMES = ['x_sea_water_velocity', 'y_sea_water_velocity', 'sea_floor_depth_below_sea_level', 'land_binary_mask']
SIZES = [1, 255, 257, 100003]      # a wave tail, a block tail on either side of the block size, several blocks
SOLAR = solar_time_scalars(datetime(2020, 1, 10, 11, 30))
# largest |difference| to the golden at the end of the run: (lon [deg], lat [deg], z [m]) per case, MEASURED on the MI355X
RUN_MEASURED = {case: (1.32e-9, 1.72e-9, 0.0) for case in CASES}


def _inputs(n):
    """Random elements in the region of the golden (30 W - 30 E, 55 - 80 N: the sun stays below 40 deg, where the bound of the
    elevation was measured), between 2 m above the surface and the sea floor or below it"""
    rng = np.random.default_rng(n)
    d = dict(lon=rng.uniform(-30, 30, n), lat=rng.uniform(55, 80, n), depth=rng.uniform(5, 200, n).astype(np.float32),
             hatched=(rng.uniform(0, 1, n) < 0.6).astype(np.float32), stage=rng.uniform(0, 1.2, n).astype(np.float32))
    d['z'] = -rng.uniform(-0.01, 1.1, n) * d['depth'].astype(np.float64)
    d['z'][::7] = np.float32(d['z'][::7])
    return d


def _particles(ctx, d, depth=True, slots=(STAGE, HATCHED)):
    n = len(d['lon'])
    P = ctx.particles(max(n, 1))
    if n:
        P.append(d['lon'], d['lat'], z=d['z'])
    if depth:
        P.env_upload('sea_floor_depth_below_sea_level', d['depth'])
    for slot in slots:
        P.set_property(slot, d['stage' if slot == STAGE else 'hatched'])
    return P


@pytest.mark.parametrize('n', SIZES)
def test_entry_points_against_the_host_build(ctx, n):
    d = _inputs(n)
    e_host = larvalx_host.elevation(d['lon'], d['lat'], SOLAR)
    assert np.abs(e_host).min() > 1e-9      # (no element so close to sunrise that the last place of arcsin decides its band)
    P = _particles(ctx, d)
    e = P.solar_elevation(*SOLAR)
    worst = np.abs(e - e_host).max()
    print('n = %d: solar elevation, device against the host build: %.3g deg (bound %.3g)' % (n, worst, ELEVATION_MAX_DEG))
    assert e.dtype == np.float64 and worst <= ELEVATION_MAX_DEG
    inc = (1800.0 / 86400) / 1.3
    P.larvalx_hatch(inc, STAGE, HATCHED)
    s, h = larvalx_host.hatch(inc, d['stage'], d['hatched'])
    assert np.array_equal(bits(P.get_property(STAGE)), bits(s)) and np.array_equal(bits(P.get_property(HATCHED)), bits(h))
    larva = d['hatched'] == 1
    assert np.array_equal(bits(s[larva]), bits(d['stage'][larva]))
    P.close()
    for mode, z_f32, only_hatched in (('dvm', False, True), ('dvm', True, False), ('depth', False, False), ('depth', True, True)):
        P = _particles(ctx, d)
        b0, b1 = ((-60.0, 6.0), (0.0, 0.0)) if mode == 'depth' else ((-5.0, 1.0), (-120.0, 12.0))
        P.larvalx_behave(mode, 1800.0, 0.01, b0, b1, SOLAR, active_only_hatched=only_hatched, z_is_float32=z_f32, hatched_slot=HATCHED)
        z = P.download()['z']
        P.close()
        zh, day = larvalx_host.behave(d['z'], d['hatched'], d['depth'], d['lon'], d['lat'], mode, only_hatched, z_f32, b0, b1, 0.01, 1800.0, SOLAR)
        assert np.array_equal(bits64(z), bits64(zh)), (mode, z_f32, only_hatched)
        if only_hatched:      # an egg keeps its z bits, even above the surface or below the sea floor
            assert np.array_equal(bits64(z[~larva]), bits64(d['z'][~larva]))
        if n > 1000:
            moves = larva if only_hatched else np.ones(n, bool)
            assert (z != d['z'])[moves].mean() > 0.5 and (mode == 'depth' or 0.1 < day[moves].mean() < 0.9)


def test_launch_nothing_cases_leave_z_alone(ctx):
    d = _inputs(300)
    P = _particles(ctx, d)
    for w, dt in ((0.0, 1800.0), (0.01, 0.0), (-1.0, 1800.0)):
        P.larvalx_behave('depth', dt, w, (-60.0, 6.0), active_only_hatched=False, hatched_slot=HATCHED)
        P.larvalx_behave('dvm', dt, w, (-5.0, 1.0), (-25.0, 2.5), SOLAR, hatched_slot=HATCHED)
    assert np.array_equal(bits64(P.download()['z']), bits64(d['z']))
    P.close()
    P = _particles(ctx, {k: v[:0] for k, v in d.items()})      # no element at all
    P.larvalx_hatch(0.1, STAGE, HATCHED)
    P.larvalx_behave('dvm', 1800.0, 0.01, (-5.0, 1.0), (-25.0, 2.5), SOLAR, hatched_slot=HATCHED)
    assert len(P) == 0 and len(P.solar_elevation(*SOLAR)) == 0
    P.close()


def test_entry_points_report_missing_state_and_bad_arguments(ctx):
    d = _inputs(8)
    P = _particles(ctx, d, depth=False, slots=(STAGE,))
    with pytest.raises(OdrError, match='sea_floor_depth_below_sea_level') as e:      # the depth has not been sampled
        P.larvalx_behave('depth', 1800.0, 0.01, (-60.0, 6.0), active_only_hatched=False)
    assert e.value.code == -4                                                         # ODR_ERR_STATE
    P.env_upload('sea_floor_depth_below_sea_level', d['depth'])
    with pytest.raises(OdrError, match='slot %d' % HATCHED) as e:                     # the hatched slot was never set
        P.larvalx_behave('depth', 1800.0, 0.01, (-60.0, 6.0), hatched_slot=HATCHED)
    assert e.value.code == -4
    with pytest.raises(OdrError, match='slot %d' % HATCHED) as e:
        P.larvalx_hatch(0.1, STAGE, HATCHED)
    assert e.value.code == -4
    P.larvalx_behave('depth', 1800.0, 0.01, (-60.0, 6.0), active_only_hatched=False)      # phytoplankton: the slot is not read
    P.set_property(HATCHED, d['hatched'])
    for bad in ((9, HATCHED), (STAGE, -1), (STAGE, STAGE)):
        with pytest.raises(ValueError):                                               # out of [0, 9) or repeated
            P.larvalx_hatch(0.1, *bad)
    with pytest.raises(ValueError):
        P.larvalx_hatch(np.nan, STAGE, HATCHED)
    with pytest.raises(ValueError):
        P.larvalx_behave('depth', 1800.0, 0.01, (-60.0, -1.0))                        # a negative half-width
    with pytest.raises(KeyError):
        P.larvalx_behave('none', 1800.0, 0.01, (-60.0, 6.0))                          # (no launch exists for 'none')
    P.larvalx_hatch(0.1, STAGE, HATCHED)
    P.larvalx_behave('depth', 1800.0, 0.01, (-60.0, 6.0), hatched_slot=HATCHED)
    P.close()


class _Resorted(LarvalFishExtended):
    """Re-sorts the device layout by grid cell at the start of EVERY update(), keeping the sampled environment"""
    permuted = 0

    def update(self):
        sid = next(b.sid for b in self.readers.values() if b.is_grid() and b.sid is not None)
        self.P.sort_by_cell(sid, keep_environment=True)
        self.permuted += int((np.diff(self.P.ids()) < 0).any())
        super().update()


def _run(g, case, cls, monkeypatch):
    cfg = config(g, case)
    start = T0 + timedelta(seconds=float(g['start_seconds']))
    times = [start + timedelta(seconds=float(t)) for t in g['g_t']]
    o = cls(loglevel=50, seed=0, rng='numpy')
    o.add_reader(readers.GridReader(g['g_x'], g['g_y'], times, {k: g['g_' + k] for k in NAMES}))
    o.set_config('vertical_mixing:timestep', float(g['dt_mix']))
    for k, v in cfg.items():
        if ':' in k:
            o.set_config(k, v)
    steps = g['elevation'].shape[0]
    if cfg['drift:vertical_mixing']:      # the reference's own draws, in its element order (the device layer maps them to a permuted layout)
        draws = iter(g[case + '_uniforms'].reshape(-1, g['lon'].shape[1]))
        monkeypatch.setattr(np.random, 'random', lambda size=None: next(draws))
    o.seed_elements(lon=g['lon'][0], lat=g['lat'][0], z=g['z0'], time=start, stage_fraction=g['seed_stage_fraction'],
                    hatched=np.zeros(g['lon'].shape[1], np.uint8))
    res = o.run(time_step=float(g['dt']), steps=steps)
    assert o.steps_calculation == steps
    if cfg['drift:vertical_mixing']:
        assert next(draws, None) is None      # every recorded draw was used
    return o, res, cfg


@pytest.mark.parametrize('resorted', [False, True], ids=['as seeded', 're-sorted every step'])
@pytest.mark.parametrize('case', CASES)
def test_run_reproduces_the_reference_trajectories(case, resorted, monkeypatch):
    """rng='numpy' with the reference's recorded np.random draws: every case of the golden through run(); once more with the
    elements re-sorted in every step (the run's own periodic re-sort, which needs more elements than the golden has, made
    unconditional): the two property slots travel with their elements."""
    g = golden('c31_larvalfish_extended.npz')
    o, res, cfg = _run(g, case, _Resorted if resorted else LarvalFishExtended, monkeypatch)
    n, steps = g['lon'].shape[1], g['elevation'].shape[0]
    e = o.elements
    order = np.argsort(e.ID)
    assert len(e.ID) == n and (g[case + '_status'][-1] == 0).all()
    if resorted:
        assert o.permuted >= steps // 2
    hatched = np.stack([g[case + '_hatched_before'][0]] + list(g[case + '_hatched_after'])).T      # [element, record]: as seeded, then per step
    assert res['hatched'].shape == (n, steps + 1) and np.array_equal(res['hatched'], hatched.astype(np.float32))
    z_want = g[case + '_beh_z_after'][-1]
    dlon, dlat, dz = (np.abs(np.asarray(getattr(e, k))[order] - w).max() for k, w in (('lon', g['lon'][-1]), ('lat', g['lat'][-1]), ('z', z_want)))
    ds = np.abs(bits(np.asarray(e.stage_fraction)[order]).astype(np.int64) - bits(g[case + '_stage_fraction_after'][-1]).astype(np.int64)).max()
    print('case %s%s: largest differences at the end: lon %.3g lat %.3g deg, z %.3g m, stage_fraction %d ulp; %d larvae'
          % (case, ' re-sorted' if resorted else '', dlon, dlat, dz, ds, int(np.asarray(e.hatched).sum())))
    assert ds == 0 and e.stage_fraction.dtype == np.float32 and e.hatched.dtype == np.float32
    mlon, mlat, mz = RUN_MEASURED[case]
    assert dlon <= 4 * mlon and dlat <= 4 * mlat and dz <= 4 * mz
    if not cfg['drift:vertical_mixing']:
        assert np.array_equal(bits64(np.asarray(e.z)[order]), bits64(z_want))


def test_ocean_drift_solar_elevation(ctx):
    """The public method of the base model (physics_methods.py:977-979) on a seeded, running model: the elevation of the active
    elements at the model's time, against the golden's values of the same positions and time."""
    g = golden('c31_larvalfish_extended.npz')
    k = 24
    o = OceanDrift(loglevel=50)
    o.P, o.time = ctx.particles(200), T0 + timedelta(seconds=float(g['start_seconds']) + k * float(g['dt']))
    o.P.append(g['lon'][k + 1], g['lat'][k + 1], z=np.zeros(200))
    e = o.solar_elevation()
    o.P.close()
    assert np.abs(e - g['elevation'][k]).max() <= ELEVATION_MAX_DEG and 0.1 < (e > 0).mean() < 0.9
