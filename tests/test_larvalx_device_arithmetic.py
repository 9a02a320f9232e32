"""CPU: the device arithmetic of LarvalFishExtended.update_fish_larvae, LarvalFishExtended._apply_vertical_behavior and
solar_elevation (opendrift_amd/csrc/odr_larvalx.hip.h and odr_solar.hip.h, compiled for the host by tests/larvalx_host.py) against
the values the reference itself computed (golden c31, tools/gen_golden_larvalfish_extended.py): every stored step of its four
cases, one step at a time, from the golden's "before" arrays to its "after" arrays.

hatched, stage_fraction and the day / night flag are identical; z after the behaviour step is bit for bit the golden's, given the
golden's z before it -- in float64 (case A, after the vertical mixing) and in the float32 the reference holds z in without mixing
(cases B and C), in mode depth and in mode dvm.  The solar elevation goes through sin, cos and arcsin, which neither NumPy nor
the C library round correctly.  MEASURED largest distance of the host build to the golden's float64 elevation over its 48 steps
x 200 elements: 1.42e-14 deg -- one unit in the last place of an elevation between 8 and 16 deg in size (1.8e-15) times the
amplification of arcsin, far from the zenith here (|elevation| < 40 deg).  Bound: four times that."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden

import larvalx_host
from opendrift_amd.oceandrift import solar_time_scalars

ELEVATION_MEASURED_DEG = 1.42e-14
ELEVATION_MAX_DEG = 4 * ELEVATION_MEASURED_DEG
T0 = datetime(2020, 1, 1)
CASES = 'ABCD'


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def config(g, case):
    """The configuration of a case by its config key, and what the launches derive from it"""
    cfg = {k[len(case) + 5:].replace('__', ':'): g[k][()] for k in g.files if k.startswith(case + '_cfg_')}
    cfg = {k: (v.item() if isinstance(v, np.generic) else str(v)) for k, v in cfg.items()}
    cfg['larva'] = cfg['biology:particle_type'] == 'larva'
    cfg['mode'] = cfg['biology:vertical_behavior_mode']
    cfg['increment'] = (float(g['dt']) / 86400) / cfg['egg:hatch_time_days']
    return cfg


def half_width(cfg, centre):
    return min(max(cfg['biology:dz_rel'] * abs(centre), cfg['biology:dz_min']), cfg['biology:dz_max'])


def bands(cfg):
    """((centre, half-width) of the depth or night band, the same of the day band)"""
    if cfg['mode'] == 'depth':
        c = cfg['biology:z_pref']
        return (c, half_width(cfg, c)), (0.0, 0.0)
    n, d = cfg['biology:z_night'], cfg['biology:z_day']
    return (n, half_width(cfg, n)), (d, half_width(cfg, d))


def step_time(g, k):
    return T0 + timedelta(seconds=float(g['start_seconds']) + k * float(g['dt']))


def golden_step(g, case, k):
    """Inputs and the reference's outputs of both methods in step k of a case (every element is present in every step)"""
    d = {name: g['%s_%s' % (case, name)][k] for name in ('stage_fraction_before', 'stage_fraction_after', 'hatched_before', 'hatched_after',
                                                       'beh_z_before', 'beh_z_after', 'beh_hatched')}
    d['lon'], d['lat'] = g['lon'][k + 1], g['lat'][k + 1]      # the behaviour step follows the advection; nothing moves after it
    d['elevation'], d['depth'], d['dt'] = g['elevation'][k], g['depth'][k], float(g['dt'])
    d['z_f32'] = bool(g[case + '_z_is_float32'][k])
    d['solar'] = solar_time_scalars(step_time(g, k))
    return d


def host_behave(d, cfg, z=None):
    b0, b1 = bands(cfg)
    return larvalx_host.behave(d['beh_z_before'] if z is None else z, d['beh_hatched'], d['depth'], d['lon'], d['lat'], cfg['mode'], cfg['larva'],
                               d['z_f32'], b0, b1, cfg['biology:w_active'], d['dt'], d['solar'])


def test_golden_covers_what_the_tests_rely_on():
    g = golden('c31_larvalfish_extended.npz')
    assert [(config(g, c)['biology:particle_type'], config(g, c)['mode'], config(g, c)['drift:vertical_mixing']) for c in CASES] == \
        [('larva', 'dvm', True), ('larva', 'depth', False), ('phytoplankton', 'dvm', False), ('larva', 'none', False)]
    day = (g['elevation'] > 0).mean(axis=1)
    assert ((day >= 0.1) & (day <= 0.9)).sum() >= 3                                   # (a)
    assert np.abs(g['elevation']).min() >= 1e-6                                      # (f)
    assert not g['A_z_is_float32'].any() and g['B_z_is_float32'].all() and g['C_z_is_float32'].all()
    which = set()
    for c in 'ABC':
        cfg = config(g, c)
        for centre, hw in bands(cfg)[:1 if cfg['mode'] == 'depth' else 2]:
            which.add('dz_min' if hw == cfg['biology:dz_min'] else 'dz_max' if hw == cfg['biology:dz_max'] else 'dz_rel')
        stage = np.concatenate([g[c + '_stage_fraction_before'], g[c + '_stage_fraction_after']]).astype(np.float64)
        assert (np.abs(stage - 1.0) >= 1e-5).all()                                   # (f)
    assert which == {'dz_min', 'dz_rel', 'dz_max'}
    hatching = (g['A_hatched_before'] == 0) & (g['A_hatched_after'] == 1)
    assert hatching.any(axis=1).sum() >= 5 and (g['A_hatched_after'][-1] == 0).mean() >= 0.1      # (e)
    assert g['elevation'].dtype == np.float64 and g['depth'].dtype == np.float32 and g['A_beh_z_after'].dtype == np.float64
    assert g['seed_stage_fraction'].dtype == np.float32 and g['A_uniforms'].shape[1] == int(g['dt'] / g['dt_mix'])


def test_solar_elevation_of_the_host_build_is_the_reference_s_within_the_measured_bound():
    g = golden('c31_larvalfish_extended.npz')
    worst = 0.0
    for k in range(g['elevation'].shape[0]):
        e = larvalx_host.elevation(g['lon'][k + 1], g['lat'][k + 1], solar_time_scalars(step_time(g, k)))
        worst = max(worst, np.abs(e - g['elevation'][k]).max())
        assert np.array_equal(e > 0, g['elevation'][k] > 0)
    print('largest distance to the reference\'s solar elevation: %.3g deg (bound %.3g)' % (worst, ELEVATION_MAX_DEG))
    assert worst <= ELEVATION_MAX_DEG


@pytest.mark.parametrize('case', CASES)
def test_host_build_of_the_device_functions_reproduces_the_reference(case):
    g = golden('c31_larvalfish_extended.npz')
    cfg = config(g, case)
    steps = g['elevation'].shape[0]
    moved = clipped = hatched_total = 0
    for k in range(steps):
        d = golden_step(g, case, k)
        if cfg['larva']:
            s, h = larvalx_host.hatch(cfg['increment'], d['stage_fraction_before'], d['hatched_before'])
            assert np.array_equal(h, d['hatched_after'].astype(np.float32))                        # the same eggs hatch
            assert np.array_equal(bits(s), bits(d['stage_fraction_after']))
            larva = d['hatched_before'] == 1                                                       # a larva's stage_fraction stays
            assert np.array_equal(bits(s[larva]), bits(d['stage_fraction_before'][larva]))
            hatched_total += int(((d['hatched_before'] == 0) & (h == 1)).sum())
        else:      # phytoplankton: the reference never touches stage_fraction
            assert np.array_equal(bits(d['stage_fraction_after']), bits(g['seed_stage_fraction']))
            assert np.array_equal(bits(d['stage_fraction_before']), bits(g['seed_stage_fraction']))
        assert np.array_equal(d['beh_hatched'], d['hatched_after'])
        if cfg['mode'] == 'none':
            assert np.array_equal(bits64(d['beh_z_before']), bits64(d['beh_z_after']))
            continue
        z, day = host_behave(d, cfg)
        moves = (d['beh_hatched'] == 1) if cfg['larva'] else np.ones(len(z), bool)
        assert np.array_equal(bits64(z), bits64(d['beh_z_after']))                                 # bit for bit, clipped ones included
        assert np.array_equal(bits64(z[~moves]), bits64(d['beh_z_before'][~moves]))
        if cfg['mode'] == 'dvm':
            assert np.array_equal(day[moves], (d['elevation'] > 0)[moves]) and not day[~moves].any()
        moved += int((z != d['beh_z_before']).sum())
        clipped += int((moves & (z == -d['depth'].astype(np.float64)) & (z != d['beh_z_before'])).sum())
    print('case %s: %d eggs hatch, %d moves, %d of them end on the sea floor' % (case, hatched_total, moved, clipped))
    if cfg['larva']:
        assert hatched_total >= 50
    if cfg['mode'] != 'none':
        assert moved >= 200      # (more moves than elements: the comparison above is not one of untouched values)


def test_hatching_threshold_and_untouched_larvae():
    """stage_fraction reaching exactly 1 hatches (>=); one float32 addition of float32(increment); a larva is not touched."""
    inc = 0.25
    s, h = larvalx_host.hatch(inc, [0.75, 0.7499999, 0.5, 3.0, np.nan], [0, 0, 0, 1, 1])
    assert h.tolist() == [1, 0, 0, 1, 1] and s[0] == 1 and s[1] < 1 and s[2] == 0.75 and s[3] == 3 and np.isnan(s[4])
    inc = (1800.0 / 86400) / 1.3
    s, h = larvalx_host.hatch(inc, np.float32([0.3]), [0])
    assert s[0] == np.float32(0.3) + np.float32(inc)


def test_band_target_step_limit_and_clips():
    """Mode depth around -10 +- 1 with 0.5 m per step: below, inside and above the band; the surface and the sea floor."""
    z0 = np.float64([-20.0, -11.2, -10.5, -9.0, -8.7, -0.2, -12.5])
    depth = np.float32([100, 100, 100, 100, 100, 100, 11.3])
    kw = dict(hatched=np.ones(7), depth=depth, lon=np.zeros(7), lat=np.zeros(7), mode='depth', only_hatched=True, band0=(-10.0, 1.0),
              band1=(0.0, 0.0), w_active=0.001, dt=500.0)
    z, day = larvalx_host.behave(z0, z_f32=False, **kw)
    assert np.array_equal(z, [-19.5, -11.0, -10.5, -9.0, -9.0, -0.7, -float(np.float32(11.3))]) and not day.any()
    z32, _ = larvalx_host.behave(z0, z_f32=True, **kw)
    assert np.array_equal(z32, np.float32(z).astype(np.float64)) and not np.array_equal(z32, z)
    # nothing moves: w_active = 0 and dt = 0 leave even an element above the surface or below the sea floor alone (:246-247)
    for w, dt in ((0.0, 500.0), (0.001, 0.0)):
        zz, _ = larvalx_host.behave([0.5, -200.0], np.ones(2), [100, 100], [0, 0], [0, 0], 'depth', True, False, (-10.0, 1.0), (0.0, 0.0), w, dt)
        assert np.array_equal(zz, [0.5, -200.0])
    zz, _ = larvalx_host.behave([0.5, -200.0, -10.0], [1, 1, 0], [100, 100, 5], [0, 0, 0], [0, 0, 0], 'depth', True, False, (-10.0, 1.0), (0.0, 0.0), 0.001, 500.0)
    assert np.array_equal(zz, [0.0, -100.0, -10.0])      # the clips apply to an element inside its band too; an egg keeps its z
    zz, _ = larvalx_host.behave([-10.0], [0], [5], [0], [0], 'depth', False, False, (-10.0, 1.0), (0.0, 0.0), 0.001, 500.0)
    assert zz[0] == -5.0                                  # phytoplankton: hatched is not read


def test_day_and_night_bands_follow_the_sun_of_the_element():
    """Noon UTC on 21 June: day at Greenwich, night at the date line; 60 N."""
    solar = solar_time_scalars(datetime(2020, 6, 21, 12))
    lon, lat = np.float64([0.0, 180.0]), np.float64([60.0, 60.0])
    e = larvalx_host.elevation(lon, lat, solar)
    assert 53 < e[0] < 55 and -7 < e[1] < -5      # (90 - 60 +- the declination, 24.15 deg by this formula)
    z, day = larvalx_host.behave([-15.0, -15.0], [1, 1], [100, 100], lon, lat, 'dvm', True, False, (-5.0, 1.0), (-25.0, 2.5), 0.003, 1800.0, solar)
    assert day.tolist() == [True, False] and np.array_equal(z, [-20.4, -9.6])
