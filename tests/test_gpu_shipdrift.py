"""GPU: ShipDrift -- the kernel of odr_ship_drift against the host build of the same header, and the model run end to end against
the reference's own ShipDrift trajectories (golden c29, tools/gen_golden_shipdrift.py).

Device against host build: status, moving, stranding and the elements that do not move are exact; the float64 intermediates and
the positions are within DEVICE_BOUND, which is the largest difference measured on an MI355X (DEVICE_MEASURED, printed again by
every run) plus one ulp of the compared quantity -- the device library's exp / atan2 / cos / sin and the host's libm differ in the
last place, and a last place of the float64 exp can move the float32 rounding of a spectrum value."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from opendrift_amd import readers
from opendrift_amd._abi import SHIP_PROPERTIES, OdrError
from opendrift_amd.device import Particles
from opendrift_amd.shipdrift import ShipDrift

import ship_host
from test_ship_device_arithmetic import ABSOLUTE, POSITION_STEP_BOUND_DEG, RELATIVE, STEPS, WFORCE, bits, g, records, table  # noqa: F401

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
DT = 3600.0
EPS = float(np.spacing(1.0))
# largest differences device - host build over the cases of test_device_agrees_with_the_host_build (relative for RELATIVE, rad,
# m/s, deg), and one ulp of the compared quantity: of 1 for a relative difference, of pi for an angle, of 2 m/s, of 64 deg
DEVICE_MEASURED = {'F_wave_b': 0.0, 'beta2_b': 0.0, 'F_wave': 0.0, 'beta2': 0.0, 'F_total': 1.25e-16, 'uw_tot': 0.0, 'wave_dir': 0.0,
                   'uw_dir': 2.23e-16, 'velocity_u': 2.23e-16, 'velocity_v': 1.12e-16, 'lon': 4.45e-16, 'lat': 0.0}
ULP = dict({k: EPS for k in RELATIVE}, wave_dir=float(np.spacing(np.pi)), uw_dir=float(np.spacing(np.pi)), velocity_u=float(np.spacing(2.0)),
           velocity_v=float(np.spacing(2.0)), lon=float(np.spacing(64.0)), lat=float(np.spacing(64.0)))
DEVICE_BOUND = {k: DEVICE_MEASURED[k] + ULP[k] for k in DEVICE_MEASURED}
# positions of a run of STEPS steps against the golden: four times the bound of one step from the CPU replay
# (tests/test_ship_device_arithmetic.py: 4 x the 4.41e-9 deg measured there), 7.1e-8 deg
RUN_POSITION_BOUND_DEG = 4 * POSITION_STEP_BOUND_DEG
assert RUN_POSITION_BOUND_DEG < 1e-6


def _case(g, n, n_classes, from_wind):
    """n element-steps of the golden's case (b) with n_classes classes; from n = 63 on a calm element, one on land, one that does
    not move."""
    d = records(g, n, seed=n)
    d['cls'] = (d['cls'] % n_classes).astype(np.int32)
    d['moving'] = np.ones(n, np.int32)
    d['land'] = np.array(d['land'], np.float32)
    if n >= 63:
        d['env']['x_wind'][1] = d['env']['y_wind'][1] = 0.0
        d['land'][2] = 1.0
        d['moving'][3::7] = 0
        if not from_wind:
            d['env'][ship_host.TM02][4] = 0.0      # a ship the period's reader does not cover: no waves, not NaN
    d['modes'] = dict(hs_mode=1, tp_mode=3, wave_dir_from_stokes=False) if from_wind else dict(hs_mode=0, tp_mode=0, wave_dir_from_stokes=True)
    return d


def _device(ctx, d, tab, stranded_code=5, **kw):
    n = len(d['lon'])
    ctx.slot_aliases[ship_host.TM02] = 13      # Tm02 in the peak period's slot, as ShipDrift's own context has it
    P = ctx.particles(n)
    P.append(d['lon'], d['lat'], z=np.zeros(n), moving=d['moving'])
    for k in ship_host.ENV:
        P.env_upload(k, np.ascontiguousarray(d['env'][k], np.float32))
    P.env_upload('land_binary_mask', d['land'])
    for slot, k in enumerate(ship_host.PROPS):
        P.set_property(slot, np.ascontiguousarray(d['props'][k], np.float32))
    P.set_property(6, d['orientation'].astype(np.float32))
    P.set_property(7, d['cls'].astype(np.float32))
    T = P.ship_table(tab)
    out = P.ship_drift(DT, T, stranded_code=stranded_code, intermediates=True, **dict(d['modes'], **kw))
    out.update(P.download())
    T.close()
    P.close()
    return out


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('n_classes,from_wind', [(1, True), (5, False)])
def test_device_agrees_with_the_host_build(ctx, g, table, n, n_classes, from_wind):
    """A single element, a wave tail (63, 65), a full wave, two workgroups (257); one class and five; waves and their direction
    from the wind, and from the sampled variables."""
    d = _case(g, n, n_classes, from_wind)
    tab = table[:n_classes]
    dev = _device(ctx, d, tab)
    r = ship_host.update(d['lon'], d['lat'], d['moving'], d['land'], d['env'], d['props'], d['orientation'], d['cls'], tab, dt=DT, **d['modes'])
    worst = {}
    for k in RELATIVE:
        worst[k] = (np.abs(dev[k] - r[k]) / np.maximum(np.abs(r[k]), np.finfo(np.float64).tiny)).max()      # (0 where both are 0: a calm sea)
    for k in ABSOLUTE + ('lon', 'lat'):
        worst[k] = np.abs(dev[k] - r[k]).max()
    print('n = %d, %d classes, %s: device - host build' % (n, n_classes, 'wind' if from_wind else 'reader'),
          ' '.join('%s %.3g' % kv for kv in worst.items()))
    # exact: who strands, with which status, who stands still
    assert np.array_equal(dev['status'], np.where(r['stranded'], 5, 0))
    assert np.array_equal(dev['moving'], np.where(r['stranded'], 0, d['moving']))
    still = d['moving'] == 0
    assert np.array_equal(dev['lon'][still], d['lon'][still]) and np.array_equal(dev['lat'][still], d['lat'][still])
    assert (dev['lon'][~still] != d['lon'][~still]).all()
    if n >= 63:
        assert r['stranded'][2] and still[3] and r['F_wind_x'][1] == 0 and np.isfinite(dev['uw_tot']).all()
        assert (r['Tm'] < np.float32(5.7)).any() and (r['Tm'] > np.float32(8.55)).any() and \
            ((r['Tm'] >= np.float32(5.7)) & (r['Tm'] <= np.float32(8.55))).any()
        assert len(set(d['cls'].tolist())) == n_classes
        if not from_wind:
            assert dev['F_wave'][4] == 0 and dev['beta2'][4] == 0 and np.isfinite(dev['uw_tot'][4]) and np.isfinite(dev['lon'][4])
    for k, v in worst.items():
        assert v <= DEVICE_BOUND[k], (k, v, DEVICE_BOUND[k])


def test_the_class_index_selects_the_table(ctx, g, table):
    """Five classes against the same elements with every index 0: the integrals differ by far more than any bound wherever the
    class is another one, and not at all where it is class 0."""
    d = _case(g, 65, 5, False)
    a = _device(ctx, d, table[:5])
    b = _device(ctx, dict(d, cls=np.zeros(65, np.int32)), table[:5])
    same = d['cls'] == 0
    assert np.array_equal(bits(a['F_wave'][same]), bits(b['F_wave'][same])) and same.any()
    other = ~same
    other[4] = False      # (the ship without a period has no waves with either table)
    assert a['F_wave'][4] == 0 and b['F_wave'][4] == 0 and other.sum() > 30
    assert (np.abs(a['F_wave'][other] / b['F_wave'][other] - 1) > 1e-3).all()


def _final(o, n):
    out = {k: np.full(n, np.nan) for k in ('lon', 'lat')}
    out['status'] = np.full(n, -1)
    for d in (o.elements, o.elements_deactivated):
        for k in ('lon', 'lat', 'status'):
            out[k][d.ID] = getattr(d, k)
    return out


def _run(g, case, tiles=1, rng='numpy', sort_every=None, seed_calls=1):
    """The golden's run of `case`; tiles > 1: `tiles` copies of its population, element ID i a copy of the golden's i % 300;
    seed_calls = 2: the population seeded in two calls (the second adds classes)."""
    c = case + '_'
    times = [T0 + timedelta(seconds=float(t)) for t in g[c + 'g_t']]
    fields = {k[len(c) + 2:]: np.repeat(g[k][None], len(times), axis=0) for k in g.files if k.startswith(c + 'g_') and k[len(c) + 2:] not in 'xyt'}
    o = ShipDrift(loglevel=50, seed=0, rng=rng, wforce=WFORCE)      # (horizontal_diffusivity is 0: nothing is drawn)
    o.add_reader(readers.GridReader(g[c + 'g_x'], g[c + 'g_y'], times, fields))
    o.set_config('environment:constant:horizontal_diffusivity', 0.0)
    if case == 'b':
        o.set_config('general:coastline_action', 'none')
    n = g[c + 'lon'].shape[1] * tiles
    pop = dict(lon=np.tile(g[c + 'lon'][0], tiles), lat=np.tile(g[c + 'lat'][0], tiles),
               **{k: np.tile(g[c + 'seed_' + k], tiles) for k in ('length', 'height', 'draft', 'beam')})
    if seed_calls == 1:
        o.seed_elements(time=T0, **pop)
    else:
        cut = 4      # (an even number of elements: the alternating orientation of the second call starts at 0 again)
        o.seed_elements(time=T0, **{k: v[:cut] for k, v in pop.items()})
        first = len(o.ship_classes)
        o.seed_elements(time=T0, **{k: v[cut:] for k, v in pop.items()})
        assert 0 < first < len(o.ship_classes) == 8
    if sort_every is not None:
        o.sort_every = sort_every
    o.run(time_step=float(g['dt']), steps=STEPS)
    assert o.steps_calculation == STEPS
    return o, _final(o, n)


@pytest.mark.parametrize('case', ['a', 'b'])
def test_run_reproduces_the_reference_trajectories(g, case):
    o, f = _run(g, case)
    c = case + '_'
    dlon, dlat = (np.nanmax(np.abs(f[k] - g[c + k][-1])) for k in ('lon', 'lat'))
    print('case %s: largest differences from the golden after %d steps: lon %.3g lat %.3g deg; status categories %s'
          % (case, STEPS, dlon, dlat, o.status_categories))
    assert o.status_categories == list(g[c + 'status_categories'])
    assert np.array_equal(f['status'], g[c + 'status'][-1])
    assert dlon <= RUN_POSITION_BOUND_DEG and dlat <= RUN_POSITION_BOUND_DEG
    e = o.elements
    for k in SHIP_PROPERTIES[:6]:      # the properties are carried unchanged
        assert np.array_equal(bits(np.asarray(getattr(e, k), np.float32)), bits(g[c + k][STEPS - 1][e.ID])), k
    assert np.array_equal(np.asarray(e.orientation), g[c + 'orientation'][STEPS - 1][e.ID])
    if case == 'b':
        assert (f['status'] == 1).sum() >= 3


def test_run_with_a_resort_every_step_and_with_two_seed_calls_matches_the_plain_run(g, monkeypatch):
    """Case (b) three times on the device RNG lane (the one that re-sorts; nothing is drawn): as it is; 250 copies of the
    population (75 000 elements, 67 000 at the end: above the 65 536 from which run() re-sorts) with a re-sort in EVERY step, so that the device
    order is no longer the seeding order; seeded in two calls, the second adding classes and re-numbering none.  By ID, all
    three give the same bits."""
    _, plain = _run(g, 'b', rng='device')
    tiles = 250
    sorts, sort_by_cell = [], Particles.sort_by_cell
    monkeypatch.setattr(Particles, 'sort_by_cell', lambda P, *a, **k: (sorts.append(len(P)), sort_by_cell(P, *a, **k))[1])
    o, f = _run(g, 'b', tiles=tiles, rng='device', sort_every=1)
    assert len(sorts) == STEPS and min(sorts) > 65536
    ids = o.P.ids()
    assert not (np.diff(ids) > 0).all()      # sorted by grid cell: no longer the seeding order
    _, two = _run(g, 'b', rng='device', seed_calls=2)
    for k in ('lon', 'lat', 'status'):
        assert np.array_equal(f[k], np.tile(plain[k], tiles), equal_nan=True), k
        assert np.array_equal(two[k], plain[k], equal_nan=True), k
    assert (plain['status'] == 1).sum() >= 3


def test_entry_points_report_bad_arguments_and_missing_state(ctx, table):
    n = 8
    P = ctx.particles(n)
    P.append(np.linspace(4, 4.5, n), np.full(n, 60.5), z=np.zeros(n))
    T = P.ship_table(table[:2])
    with pytest.raises(ValueError):
        P.ship_table(table[:, :48])
    bad = table[:1].copy()
    bad[0, 3, 1] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        P.ship_table(bad)
    for slot, v in enumerate((80.0, 8.0, 4.0, 10.0, 0.8, 1.4, 1.0)):
        P.set_property(slot, np.full(n, v, np.float32))
    up = lambda k, v: P.env_upload(k, np.full(n, v, np.float32))      # noqa: E731
    with pytest.raises(OdrError, match='current') as e:                     # nothing has been sampled: the current comes first
        P.ship_drift(DT, T, check_classes=False)
    assert e.value.code == -4
    up('x_sea_water_velocity', 0.1)
    up('y_sea_water_velocity', 0.0)
    with pytest.raises(OdrError, match='wind') as e:                        # the wind has not been sampled
        P.ship_drift(DT, T, check_classes=False)
    assert e.value.code == -4                                               # ODR_ERR_STATE
    up('x_wind', 8.0)
    up('y_wind', 1.0)
    with pytest.raises(OdrError, match='land_binary_mask') as e:
        P.ship_drift(DT, T, check_classes=False)
    assert e.value.code == -4
    up('land_binary_mask', 0.0)
    with pytest.raises(OdrError, match='slot 7') as e:                      # the class slot was never set
        P.ship_drift(DT, T, check_classes=False)
    assert e.value.code == -4
    P.set_property(7, np.float32([0, 1, 0, 1, 0, 1, 0, 2]))
    with pytest.raises(ValueError, match='2 classes'):                      # an index past the table: found by the binding
        P.ship_drift(DT, T)
    P.set_property(7, np.float32([0, 1, 0, 1, 0, 1, 0, 1]))
    with pytest.raises(OdrError, match='Stokes') as e:
        P.ship_drift(DT, T, wave_dir_from_stokes=True)
    assert e.value.code == -4
    with pytest.raises(OdrError, match='Hs/Tp') as e:
        P.ship_drift(DT, T, hs_mode=0, tp_mode=0)
    assert e.value.code == -4
    with pytest.raises(ValueError):
        P.ship_drift(float('nan'), T)
    with pytest.raises(ValueError):
        P.ship_drift(DT, T, class_slot=9, check_classes=False)
    with pytest.raises(ValueError):
        P.ship_drift(DT, T, beam_slot=2)                                    # a slot given twice
    with pytest.raises(ValueError):
        P.ship_drift(DT, T, tp_mode=1)
    with pytest.raises(ValueError, match='stranded_code'):
        P.ship_drift(DT, T, stranded_code=0)                                # would set moving = 0 and leave the element active
    assert T.n_classes == 2
    before = P.download()
    P.ship_drift(DT, T)
    after = P.download()
    assert (after['lon'] > before['lon']).all() and (after['status'] == 0).all()
    T.close()
    P.close()


def test_a_block_with_tm02_is_refused_unless_the_context_opted_in(ctx):
    """Context.slot_aliases is empty on every context but ShipDrift's: a reader's Tm02 fails with a KeyError that names it, as
    before; with the alias, a block that also holds the peak period raises instead of letting one replace the other."""
    from opendrift_amd.shipdrift import TM02, TP
    sid = ctx.add_grid(np.linspace(3, 5, 5), np.linspace(60, 61, 4))
    a = np.zeros((4, 5), np.float32)
    with pytest.raises(KeyError, match='second_frequency_moment'):
        ctx.upload_block(sid, 0, 0.0, {'x_wind': a, TM02: a})
    ctx.slot_aliases[TM02] = 13
    with pytest.raises(ValueError, match='same device id'):
        ctx.upload_block(sid, 0, 0.0, {TP: a, TM02: a})
    ctx.upload_block(sid, 0, 0.0, {'x_wind': a, TM02: a})
