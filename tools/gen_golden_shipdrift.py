"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c29_shipdrift.npz and tests/golden/wforce.dat from the REFERENCE ITSELF.

The reference's own ShipDrift (opendrift/models/shipdrift.py, Soergaard & Vada 1998) runs through oracle/refshim.py +
oracle/refdriver.py on a small lon/lat grid in the North Sea.  300 ships, 6 steps of 3600 s, horizontal_diffusivity 0, fields
constant in time (stored once).  Two cases:

  (a) no reader for wave height, wave period or Stokes drift: all three fall back to 0, calculate_missing_environment_variables
      (physics_methods.py:856-883) fills height and period from the wind before update() runs, and update() takes the wind
      direction as wave direction (shipdrift.py:304-308).  The wind speed is >= 1 m/s everywhere.  (A wind of exactly 0 would NOT
      give a period of 0: _wave_frequency, physics_methods.py:908-916, starts from omega = 5 and overwrites it only where the wind
      speed is > 0, so the period there is 2 pi / 5 s and the height 0 -- the spectrum is 0 and the ship moves with wind force 0.
      Case (a) keeps away from it only so that every ship has waves.)
  (b) wave height, Tm02 and Stokes drift from the reader: the wave direction is the Stokes direction.  The wind is exactly 0 on a
      patch of nodes (wind force 0, not NaN: shipdrift.py:244-245), there is a land patch, and general:coastline_action is 'none',
      so that an element on land reaches the model's own stranding (:342) instead of the base class's.

The ships come from eight hulls (length, beam, draft), which give eight classes of the clipped ratios (beam/length, draft/length)
-- among them one below and one above each of the four clip limits of :223-227 -- with a height of its own for every ship (so
that the wind drag coefficient takes all three branches of :188-191) and alternating orientation.

Stored per step, by element ID (NaN / -1 where an element is not present): the live float64 lon / lat and status after the
step; the float32 environment update() saw; the locals of ShipDrift.update when it returns -- Tm, Hs, bl, dl, F_wind_x,
F_wind_y, F_wave_b (before the period factors), F_wave, beta2, beta1, wave_dir, F_total, uw_tot, uw_dir, velocity_u,
velocity_v -- and beta2 before the period factors (taken by a line tracer where `longperiod` is assigned; the reference is not
edited); per class the 49 values of the two interpolators (recorded by wrapping them on the instance).  The dtype of every
stored intermediate is asserted (DTYPES below): that is the dtype ladder csrc/odr_ship.hip.h restates.

Conditions asserted here so that the golden cannot hide a failure:
  (1) at least 5 classes; at least one beam/length and one draft/length clipped at each end;
  (2) both orientations hold at least 30 % of the ships;
  (3) each period class (< 5.7, 5.7 - 8.55, > 8.55) holds at least 10 % of the elements in some step of (b);
  (4) at least 3 elements with a wind speed of exactly 0 in (b);
  (5) at least 3 elements end `ship stranded`, at least 80 % never do;
  (6) every stored value of a present element is finite.

    python tools/gen_golden_shipdrift.py
"""
import inspect
import os
import shutil
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from oracle import gen_golden as gg  # noqa: E402
from oracle.refdriver import RefStepper  # noqa: E402
import opendrift.models.shipdrift as ref_shipdrift  # noqa: E402
from opendrift.models.shipdrift import ShipDrift  # noqa: E402

DT, STEPS, N = 3600.0, 6, 300
TM02 = 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'
ENV = ('x_sea_water_velocity', 'y_sea_water_velocity', 'x_wind', 'y_wind', 'land_binary_mask',
       'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity',
       'sea_surface_wave_significant_height', TM02)
WAVES = ENV[5:]
DIMS = ('length', 'height', 'draft', 'beam', 'wind_drag_coeff', 'water_drag_coeff')
# the locals of update() that are stored, with the dtype NumPy gives them
DTYPES = {'Tm': np.float32, 'Hs': np.float32, 'bl': np.float32, 'dl': np.float32, 'F_wind_x': np.float32, 'F_wind_y': np.float32,
          'scale1': np.float32, 'beta1': np.float32, 'F_wave_b': np.float64, 'F_wave': np.float64, 'beta2': np.float64,
          'wave_dir': np.float64, 'F_total': np.float64, 'uw_tot': np.float64, 'uw_dir': np.float64, 'velocity_u': np.float64,
          'velocity_v': np.float64}
NOMI = 49          # spectrum points below ommin3 = 7
# (length, beam, draft): beam/length, draft/length
HULLS = ((80., 10., 4.),        # 0.125  0.05       the element defaults
         (100., 11., 2.),       # 0.11   0.02       both clipped from below
         (60., 12., 5.),        # 0.2    0.0833     both clipped from above
         (120., 18., 6.),       # 0.15   0.05
         (150., 24., 4.5),      # 0.16   0.03
         (40., 5.6, 2.6),       # 0.14   0.065
         (200., 23., 15.),      # 0.115  0.075      beam from below, draft from above
         (90., 17., 2.),        # 0.189  0.0222     beam from above, draft from below
         )


def fields(case):
    x = np.linspace(2.0, 6.0, 81)
    y = np.linspace(59.5, 61.5, 65)
    t = np.arange(STEPS + 2) * DT
    lon, lat = np.meshgrid(x, y)
    X, Y = (lon - 3.0) / 2.0, lat - 60.0           # 0 .. 1 over the box the ships are seeded in
    Xc, Yc = np.clip(X, 0, 1), np.clip(Y, 0, 1)
    g = {}
    g['x_sea_water_velocity'] = 0.25 * np.sin(2 * np.pi * Y) + 0.1
    g['y_sea_water_velocity'] = 0.2 * np.cos(2 * np.pi * X) - 0.05
    g['x_wind'] = 7.0 + 6.0 * np.cos(np.pi * Y)            # 1 .. 13
    g['y_wind'] = -4.0 + 9.0 * Xc
    g['land_binary_mask'] = np.zeros(lon.shape)
    if case == 'b':
        calm = (lon > 3.39) & (lon < 3.66) & (lat > 60.18) & (lat < 60.36)
        g['x_wind'][calm] = 0.0
        g['y_wind'][calm] = 0.0
        g['land_binary_mask'][(lon > 4.19) & (lon < 4.51) & (lat > 60.55) & (lat < 60.76)] = 1.0
        g['sea_surface_wave_significant_height'] = 0.4 + 3.2 * Yc * (0.3 + 0.7 * Xc)
        g[TM02] = 3.5 + 7.5 * Xc
        g['sea_surface_wave_stokes_drift_x_velocity'] = 0.06 * np.cos(np.pi * X) + 0.01
        g['sea_surface_wave_stokes_drift_y_velocity'] = 0.05 * np.sin(2 * np.pi * Y) - 0.02
    g = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in g.items()}
    g.update(x=x, y=y, t=t)
    return g


def population(g, seed):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(3.3, 4.7, N)
    lat = rng.uniform(60.15, 60.85, N)
    k = np.arange(N) // 2 % len(HULLS)            # (orientation alternates with the ID: every hull gets both)
    # a few ships inside the patch of zero wind and inside the land patch of case (b)
    lon[:6], lat[:6] = rng.uniform(3.46, 3.59, 6), rng.uniform(60.23, 60.31, 6)
    lon[6:12], lat[6:12] = rng.uniform(4.26, 4.44, 6), rng.uniform(60.6, 60.71, 6)
    hull = np.array(HULLS)[k]
    height = hull[:, 2] + rng.uniform(1.0, 50.0, N)      # exposed height 1 .. 50 m: all three branches of the wind drag coefficient
    return dict(lon=lon, lat=lat, length=hull[:, 0], beam=hull[:, 1], draft=hull[:, 2], height=height)


class UpdateTracer:
    """The locals of ShipDrift.update when it returns, and beta2 where `longperiod` is assigned (before the period factors)."""

    def __init__(self):
        src, first = inspect.getsourcelines(ShipDrift.update)
        at = [first + i for i, line in enumerate(src) if line.strip().startswith('longperiod =')]
        assert len(at) == 1
        self.line, self.code = at[0], ShipDrift.update.__code__
        self.locals, self.beta2_b = None, None

    def __call__(self, frame, event, arg):
        if event == 'call' and frame.f_code is self.code:
            return self.local
        return None

    def local(self, frame, event, arg):
        if event == 'line' and frame.f_lineno == self.line:
            self.beta2_b = np.array(frame.f_locals['beta2'], copy=True)
        elif event == 'return':
            self.locals = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in frame.f_locals.items()}
        return self.local


def case(name, g, pop):
    times = [gg.T0 + timedelta(seconds=float(t)) for t in g['t']]
    one = np.ones((len(times), 1, 1), np.float32)
    o = ShipDrift(loglevel=50)
    o.set_config('general:use_auto_landmask', False)
    o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: one * v for k, v in g.items() if k not in 'xyt'}))
    o.set_config('environment:constant:horizontal_diffusivity', 0.0)
    if name == 'b':
        o.set_config('general:coastline_action', 'none')
    assert o.get_config('seed:orientation') == 'random' and o.get_config('drift:max_speed') == 2
    o.seed_elements(time=gg.T0, number=N, **pop)      # (seed_elements sizes Cf and Cd by `number`, :159-162)

    tables = {}     # (bl, dl) as float64 -> [49][2]

    def recording(which, interpolator):
        def call(omi, bl, dl):
            r = interpolator(omi, bl, dl)
            assert r.dtype == np.float64 and r.shape == bl.shape and bl.dtype == np.float32 and dl.dtype == np.float32
            k = int(round((omi - 2.25) / ((12.0 - 2.25) / 99)))
            assert 0 <= k < NOMI and omi == 2.25 + k * ((12.0 - 2.25) / 99)
            for b, d, v in zip(bl.astype(np.float64), dl.astype(np.float64), r):
                t = tables.setdefault((b, d), np.full((NOMI, 2), np.nan))
                assert np.isnan(t[k, which]) or t[k, which] == v      # a function of the class alone
                t[k, which] = v
            return r
        return call

    o.wforce_interpolator_F = recording(0, o.wforce_interpolator_F)
    o.wforce_interpolator_D = recording(1, o.wforce_interpolator_D)
    tracer = UpdateTracer()
    rec = {}
    ref_update = o.update

    def update():
        e, env = o.elements, o.environment
        rec['ID'] = np.asarray(e.ID, dtype=int)
        for k in ENV:
            assert getattr(env, k).dtype == np.float32, k
        for k in DIMS:
            assert getattr(e, k).dtype == np.float32, k
        assert e.orientation.dtype == np.uint8
        rec['env'] = {k: np.array(getattr(env, k), copy=True) for k in ENV}
        rec['dims'] = {k: np.array(getattr(e, k), copy=True) for k in DIMS + ('orientation',)}
        sys.settrace(tracer)
        try:
            ref_update()
        finally:
            sys.settrace(None)
        L = tracer.locals
        for k, dt in DTYPES.items():
            assert L[k].dtype == dt, (k, L[k].dtype)
        assert L['s'].dtype == np.float64 and L['s'].shape == (100, len(rec['ID']))
        assert tracer.beta2_b.dtype == np.float64
        rec['locals'] = dict({k: L[k] for k in DTYPES}, beta2_b=tracer.beta2_b)

    o.update = update
    st = RefStepper(o, DT, STEPS)
    nan = lambda dtype=np.float64: np.full((STEPS, N), np.nan, dtype)      # noqa: E731
    out = {k: np.full((STEPS + 1, N), np.nan) for k in ('lon', 'lat')}
    out['status'] = np.full((STEPS + 1, N), -1, np.int32)
    sch = o.elements_scheduled
    out['lon'][0], out['lat'][0], out['status'][0] = sch.lon, sch.lat, 0
    for k in ENV:
        out['env_' + k] = nan(np.float32)
    for k in DIMS:
        out[k] = nan(np.float32)
    out['orientation'] = np.full((STEPS, N), -1, np.int8)
    for k, dt in DTYPES.items():
        out[k] = nan(dt)
    out['beta2_b'] = nan()
    for s in range(STEPS):
        st.step()
        ID = rec['ID']
        lon, lat, _, status = st.state()
        out['lon'][s + 1], out['lat'][s + 1], out['status'][s + 1] = lon, lat, status
        for k in ENV:
            out['env_' + k][s, ID] = rec['env'][k]
        for k in DIMS + ('orientation',):
            out[k][s, ID] = rec['dims'][k]
        for k in rec['locals']:
            out[k][s, ID] = rec['locals'][k]
    out['status_categories'] = np.array(o.status_categories)
    keys = sorted(tables)
    out['class_bl'], out['class_dl'] = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    out['class_table'] = np.array([tables[k] for k in keys])
    for k in ('length', 'height', 'draft', 'beam'):
        out['seed_' + k] = np.array(pop[k], dtype=np.float64)
    return out


def check(name, out):
    present = out['orientation'] >= 0
    bl, dl = out['seed_beam'] / out['seed_length'], out['seed_draft'] / out['seed_length']
    assert len(out['class_bl']) >= 5 and np.isfinite(out['class_table']).all(), '(1)'
    assert (bl < 0.12).any() and (bl > 0.18).any() and (dl < 0.025).any() and (dl > 0.07).any(), '(1)'
    f32 = np.float32
    assert out['bl'][present].min() == f32(0.121) and out['bl'][present].max() == f32(0.179), '(1)'
    assert out['dl'][present].min() == f32(0.0251) and out['dl'][present].max() == f32(0.069), '(1)'
    ori = out['orientation'][0]
    assert min((ori == 0).mean(), (ori == 1).mean()) >= 0.3, '(2)'
    Tm = out['Tm']
    periods = [np.nanmax(((Tm < f32(5.7)) & present).sum(axis=1)) / N, np.nanmax(((Tm >= f32(5.7)) & (Tm <= f32(8.55)) & present).sum(axis=1)) / N,
               np.nanmax(((Tm > f32(8.55)) & present).sum(axis=1)) / N]
    calm = present & (out['env_x_wind'] == 0) & (out['env_y_wind'] == 0)
    cat = list(out['status_categories'])
    stranded = out['status'][-1] == (cat.index('ship stranded') if 'ship stranded' in cat else -9)
    print('case %s: %d classes | period classes %s | calm element-steps %d (%d elements) | ship stranded %d | categories %s'
          % (name, len(out['class_bl']), ' '.join('%.2f' % p for p in periods), calm.sum(), calm.any(axis=0).sum(), stranded.sum(), cat))
    if name == 'a':
        assert not calm.any() and (np.hypot(out['env_x_wind'], out['env_y_wind'])[present] >= 1).all()
        assert (out['env_' + WAVES[0]][present] == 0).all() and (out['env_' + WAVES[1]][present] == 0).all()
        assert cat == ['active']
    else:
        assert min(periods) >= 0.1, '(3)'
        assert calm.any(axis=0).sum() >= 3, '(4)'
        assert (out['F_wind_x'][calm] == 0).all() and (out['F_wind_y'][calm] == 0).all()
        assert stranded.sum() >= 3 and (~stranded).mean() >= 0.8, '(5)'
        assert cat == ['active', 'ship stranded']
    for k, v in out.items():      # (6)
        if v.shape == (STEPS, N) and v.dtype.kind == 'f':
            assert np.isfinite(v[present]).all(), k
    known = out['status'] >= 0
    assert np.isfinite(out['lon'][known]).all() and np.isfinite(out['lat'][known]).all()


def main():
    data = {}
    for name in 'ab':
        g = fields(name)
        out = case(name, g, population(g, 29))
        check(name, out)
        data.update({'%s_g_%s' % (name, k): v for k, v in g.items()})
        data.update({'%s_%s' % (name, k): v for k, v in out.items()})
    assert np.array_equal(data['a_class_table'], data['b_class_table'])
    path = os.path.join(gg.GOLD, 'c29_shipdrift.npz')
    np.savez_compressed(path, dt=DT, **data)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20
    # the coefficient table the reference read: data of the reference, a fixture of the tests
    table = os.path.join(os.path.dirname(ref_shipdrift.__file__), 'wforce.dat')
    shutil.copyfile(table, os.path.join(gg.GOLD, 'wforce.dat'))


if __name__ == '__main__':
    main()
