"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c27_larvalfish.npz from the REFERENCE ITSELF.

The reference's own LarvalFish (opendrift/models/larvalfish.py) runs through oracle/refshim.py + oracle/refdriver.py on the
fields of golden C25 (tools/gen_golden_pelagicegg.py: the C3-shaped 3-D grid plus stratified float32 temperature, about
4 - 12 deg C, and salinity) with a small constant Stokes drift (constant wave height and wind for its profile): RK4,
dt = 600 s, vertical_mixing:timestep = 60 s, 300 elements, 9 steps from 11:30 UTC, so that the larvae swim down in the first
three steps (hour < 12) and up in the last six.

The population is mixed: a third larvae (hatched = 1) with weights of 0.08 - 50 mg near the surface, a third eggs whose
stage_fraction lies so close below 1 that they hatch during the run, a third eggs that do not hatch.

Stored per step, by element ID (NaN / -1 where an element is no longer present): the live float64 lon / lat / z and the
status; the float32 sea_water_temperature of the step; stage_fraction, hatched, weight, length before and after
update_fish_larvae; z and length before and z after larvae_vertical_migration with the direction used; the
np.random.random draws of the mixing sub-steps in the order drawn.

Conditions on the INPUT, asserted here so that the golden cannot hide a failure:
  (a) at least 20 % of the eggs hatch during the run and at least 20 % do not;
  (b) both swimming directions occur in at least two steps each;
  (c) at least 10 % of the larvae are clamped at z = 0 in some step;
  (d) no stage_fraction lies within 1e-4 of 1 after any step (a last-place difference in exp cannot move a hatching to another
      step).  One step adds 3e-4 - 1e-3, so random seeds land inside that band: the run is repeated with the start value
      of every offending egg moved, until none is left (the trajectories do not depend on stage_fraction before hatching);
  (e) every stored value of a present element is finite.

    python tools/gen_golden_larvalfish.py
"""
import os
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from oracle import gen_golden as gg  # noqa: E402
from oracle.refdriver import RefStepper, RecordingRandom  # noqa: E402
from opendrift.models.larvalfish import LarvalFish  # noqa: E402
import gen_golden_pelagicegg as c25  # noqa: E402

START = gg.T0 + timedelta(hours=11, minutes=30)
CONSTANTS = {'sea_surface_wave_stokes_drift_x_velocity': 0.03, 'sea_surface_wave_stokes_drift_y_velocity': 0.01,
             'sea_surface_wave_significant_height': 1.2, 'x_wind': 5.0, 'y_wind': 2.0}
STAGE_MARGIN = 1e-4
SWIM_FRACTION = 0.4        # (not the default of 0.15: the run shows that the configured value reaches the kernel)
PROPS = ('stage_fraction', 'hatched', 'weight', 'length')
NAMES = tuple(k for k in c25.NAMES if k != 'upward_sea_water_velocity')      # (not a variable of LarvalFish: not stored)


def population(g, N, seed):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(g['x'][4], g['x'][-5], N)
    lat = rng.uniform(g['y'][4], g['y'][-5], N)
    kind = np.arange(N) % 3                      # 0: larva, 1: egg that hatches during the run, 2: egg that does not
    z = np.where(kind == 0, rng.uniform(-6, -0.1, N), rng.uniform(-40, -1, N))
    hatched = (kind == 0).astype(np.uint8)
    weight = np.where(kind == 0, np.exp(rng.uniform(np.log(0.08), np.log(50.0), N)), 0.08).astype(np.float32)
    stage = np.where(kind == 1, rng.uniform(0.9962, 0.9997, N), rng.uniform(0.0, 0.9, N)).astype(np.float32)
    stage[kind == 0] = 1.0
    diameter = rng.uniform(0.001, 0.0018, N).astype(np.float32)
    salinity = rng.uniform(30.5, 33.5, N).astype(np.float32)
    # every property the physics reads is seeded as an ARRAY: the reference turns a property left at its scalar default into a
    # float64 array when the elements are released (elements.py:219-222), whatever dtype the element type declares
    return dict(lon=lon, lat=lat, z=z, hatched=hatched, weight=weight, stage_fraction=stage, length=np.zeros(N, np.float32),
                diameter=diameter, neutral_buoyancy_salinity=salinity)


def case(g, pop, steps):
    N = len(pop['lon'])
    times = [START + timedelta(seconds=float(t)) for t in g['t']]
    o = LarvalFish(loglevel=50)
    o.set_config('general:use_auto_landmask', False)
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: g[k] for k in NAMES}, z=g['z']))
    for k, v in CONSTANTS.items():
        o.set_config('environment:constant:%s' % k, v)
    o.set_config('vertical_mixing:timestep', 60)
    assert o.get_config('vertical_mixing:diffusivitymodel') == 'environment' and o.get_config('drift:vertical_mixing') is True
    assert o.get_config('vertical_mixing:TSprofiles') is False and o.get_config('drift:stokes_drift') is True
    assert o.get_config('IBM:fraction_of_timestep_swimming') == 0.15
    o.set_config('IBM:fraction_of_timestep_swimming', SWIM_FRACTION)
    f = o.get_config('IBM:fraction_of_timestep_swimming')
    np.random.seed(0)
    o.seed_elements(time=START, **pop)

    # ---- recording wrappers around the reference's own methods (instance attributes: the class is untouched)
    rec = {}
    ref_update, ref_migrate = o.update_fish_larvae, o.larvae_vertical_migration

    def snapshot():
        e = o.elements
        assert e.stage_fraction.dtype == np.float32 and e.weight.dtype == np.float32 and e.length.dtype == np.float32
        assert e.hatched.dtype == np.uint8
        return {k: np.array(getattr(e, k), copy=True) for k in PROPS}

    def update_fish_larvae():
        rec['ID'] = np.asarray(o.elements.ID, dtype=int)
        assert o.environment.sea_water_temperature.dtype == np.float32
        rec['T'] = np.array(o.environment.sea_water_temperature, copy=True)
        rec['before'] = snapshot()
        ref_update()
        rec['after'] = snapshot()

    def larvae_vertical_migration():
        assert np.array_equal(rec['ID'], np.asarray(o.elements.ID, dtype=int))
        rec['direction'] = -1 if o.time.hour < 12 else 1
        rec['mig'] = dict(z_before=np.array(o.elements.z, dtype=np.float64), length=np.array(o.elements.length, copy=True),
                          hatched=np.array(o.elements.hatched, copy=True))
        ref_migrate()
        assert o.elements.z.dtype == np.float64      # float64 z + float32 displacement: a float64 sum
        rec['mig']['z_after'] = np.array(o.elements.z, dtype=np.float64)

    o.update_fish_larvae, o.larvae_vertical_migration = update_fish_larvae, larvae_vertical_migration

    st = RefStepper(o, 600.0, steps)
    out = {k: np.full((steps + 1, N), np.nan) for k in ('lon', 'lat', 'z')}
    out['status'] = np.full((steps + 1, N), -1, np.int32)
    sch = o.elements_scheduled
    out['lon'][0], out['lat'][0], out['z'][0], out['status'][0] = sch.lon, sch.lat, np.atleast_1d(sch.z) * np.ones(N), 0
    out['env_T'] = np.full((steps, N), np.nan, np.float32)
    for k in PROPS:
        for when in ('before', 'after'):
            out['%s_%s' % (k, when)] = np.full((steps, N), -1 if k == 'hatched' else np.nan, np.int8 if k == 'hatched' else np.float32)
    out['mig_z_before'], out['mig_z_after'] = np.full((steps, N), np.nan), np.full((steps, N), np.nan)
    out['mig_length'] = np.full((steps, N), np.nan, np.float32)
    out['mig_hatched'] = np.full((steps, N), -1, np.int8)
    out['direction'] = np.zeros(steps, np.int32)
    out['uniforms'] = np.full((steps, 10, N), np.nan)
    out['n_active'] = np.zeros(steps, np.int32)
    for s in range(steps):
        with RecordingRandom() as rr:
            st.step()
        assert all(d[0] == 'random' for d in rr.draws) and len(rr.draws) == 10
        ID = rec['ID']
        assert all(len(d[1]) == len(ID) for d in rr.draws)
        out['uniforms'][s, :, :len(ID)] = np.stack([d[1] for d in rr.draws])     # in the order of the active elements, as drawn
        out['n_active'][s] = len(ID)
        out['lon'][s + 1], out['lat'][s + 1], out['z'][s + 1], out['status'][s + 1] = st.state()
        out['env_T'][s, ID] = rec['T']
        for k in PROPS:
            out[k + '_before'][s, ID], out[k + '_after'][s, ID] = rec['before'][k], rec['after'][k]
        m = rec['mig']
        out['mig_z_before'][s, ID], out['mig_z_after'][s, ID] = m['z_before'], m['z_after']
        out['mig_length'][s, ID], out['mig_hatched'][s, ID] = m['length'], m['hatched']
        out['direction'][s] = rec['direction']
    for k in ('diameter', 'neutral_buoyancy_salinity'):
        out[k] = pop[k]
    for k in ('stage_fraction', 'hatched', 'weight', 'length'):      # as seeded (an element deactivated at once is in no step)
        out['seed_' + k] = np.array(pop[k], copy=True)
    out['fraction_of_timestep_swimming'] = f
    return out


def check(out):
    """The conditions (a) - (e); returns the stage_fraction values that violate (d): (step, ID, value)"""
    present = out['hatched_before'] >= 0
    egg0 = out['hatched_before'][0] == 0
    hatches = egg0 & (out['hatched_after'] == 1).any(axis=0)
    last = np.array([out['hatched_after'][:, i][present[:, i]][-1] if present[:, i].any() else -1 for i in range(present.shape[1])])
    stays = egg0 & (last == 0)
    fa, fb = hatches.sum() / egg0.sum(), stays.sum() / egg0.sum()
    d = out['direction']
    larva = (out['mig_hatched'] == 1)
    clamped = [((out['mig_z_after'][s] == 0) & larva[s] & (out['mig_z_before'][s] < 0)).sum() / max(1, larva[s].sum())
               for s in range(len(d))]
    print('eggs that hatch %.3f, that do not %.3f | directions %s | share of the larvae clamped at z = 0 per step %s'
          % (fa, fb, d.tolist(), ' '.join('%.2f' % c for c in clamped)))
    assert fa >= 0.2 and fb >= 0.2, '(a)'
    assert (d == -1).sum() >= 2 and (d == 1).sum() >= 2, '(b)'
    assert max(clamped) >= 0.1, '(c)'
    for k, v in out.items():      # (e)
        if k.startswith(('stage_fraction_', 'weight_', 'length_', 'env_T', 'mig_length')):
            assert np.isfinite(v[present]).all(), k
        if k.startswith('mig_z'):
            assert np.isfinite(v[present]).all(), k
    known = out['status'] >= 0
    for k in ('lon', 'lat', 'z'):
        assert np.isfinite(out[k][known]).all(), k
    for s_, n_ in enumerate(out['n_active']):
        assert np.isfinite(out['uniforms'][s_, :, :n_]).all() and np.isnan(out['uniforms'][s_, :, n_:]).all(), 'uniforms'
    sf = out['stage_fraction_after']
    egg_then = present & (out['hatched_before'] == 0)         # (a larva's stage_fraction is never read again)
    bad = egg_then & (np.abs(sf.astype(np.float64) - 1.0) < STAGE_MARGIN)
    return [(s, i, float(sf[s, i])) for s, i in zip(*np.nonzero(bad))]


def main(N=300, steps=9, seed=27):
    g = c25.fields()
    pop = population(g, N, seed)
    for attempt in range(20):
        out = case(g, pop, steps)
        bad = check(out)
        print('attempt %d: %d stage_fraction values within %g of 1' % (attempt, len(bad), STAGE_MARGIN))
        if not bad:
            break
        for s, i, v in bad:      # move the start value so that this value lands 1.6e-4 below 1 (the next step adds >= 3e-4)
            pop['stage_fraction'][i] = np.float32(pop['stage_fraction'][i] - (v - 1.0) - 1.6e-4)
    else:
        raise AssertionError('(d)')
    assert (pop['stage_fraction'][pop['hatched'] == 0] < 1 - STAGE_MARGIN).all()
    gc = c25.fields()
    assert all(np.array_equal(g[k], gc[k], equal_nan=True) for k in g)
    path = os.path.join(gg.GOLD, 'c27_larvalfish.npz')
    np.savez_compressed(path, dt=600.0, dt_mix=60.0, start_seconds=(START - gg.T0).total_seconds(),
                        **{('c_' + k): v for k, v in CONSTANTS.items()}, **{('g_' + k): v for k, v in g.items() if k != 'upward_sea_water_velocity'}, **out)
    print(path, os.path.getsize(path), 'bytes (c25: %d)' % os.path.getsize(os.path.join(gg.GOLD, 'c25_pelagicegg.npz')))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(gg.GOLD, 'c25_pelagicegg.npz'))


if __name__ == '__main__':
    main()
