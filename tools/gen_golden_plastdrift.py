"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c40_plastdrift.npz and tests/golden/stokes_tables.json from the REFERENCE ITSELF.

The reference's own PlastDrift (opendrift/models/plastdrift.py) runs through oracle/refshim.py + oracle/refdriver.py on a small
lon / lat grid: a current of 0.05 .. 0.3 m/s, a wind whose speed runs from exactly 0 (the four western columns) to 40 m/s in the
east -- on both sides of the parameterisation's cap of 30 m/s -- and land east of column 35.5.  No wave reader unless a case says so.

Cases:
  (a) vertical_mixing:mixingmodel = 'analytical' (the default), 300 elements with terminal velocities of 1e-4 .. 0.1 m/s, 8 steps
      of 900 s, RK4.  Stored per step and by element ID (NaN / -1 where the element is not present): the float32 x_wind, y_wind,
      Stokes x / y and wave height behind get_environment, the float32 ocean_vertical_diffusivity (K), the standard-exponential
      draws E, z behind update_particle_depth (zd) and lon, lat, z, status behind the step; end_*: the state behind the
      interact_with_coastline(final=True) that run() makes behind its loop;
  (b5, b50) (a)'s first step with drift:tabularised_stokes_drift_fetch '5000' and '50000': environment values only;
  (c1 .. c4) the decisions of environment.py:844-863 with a wave reader, one step each, environment values only:
      c1 Stokes drift > 0 from the reader (left alone), wave height 0 (replaced);
      c2 Stokes drift 0 everywhere (replaced), wave height 1.5 m (left alone);
      c3 Stokes x < 0 everywhere and y == 0 (the plain maxima are not both 0: left alone), wave height 0 (replaced);
      c4 only a wave height above 0 from the reader (left alone), the Stokes drift at its fallback (replaced);
  (d) 60 shallow elements just west of the land with general:coastline_action = 'previous' (the model's default), 8 steps; two
      more in opposite corners of the grid keep a reader that cuts its blocks to the elements' box on the whole grid.

Asserted, so that the file cannot hide a failure: every dtype claim of DESIGN.md section 7j (float32 environment and wind speed,
float64 polynomial and products, one rounding on assignment, K / terminal_velocity a float32 division widened to float64, z float64
behind the first step); np.polyval is a float64 Horner chain from the leading coefficient, bit for bit; np.random.exponential(scale,
n) == scale * np.random.standard_exponential(n) bit for bit under one generator state, and both leave the same state; a scale with
the sign bit set raises ValueError('scale < 0'); >= 10 elements of (a) above the cap, >= 10 below, some at exactly 0; z of (a)
spans more than two decades; >= 3 elements are moved back in (d).

stokes_tables.json: per fetch the coefficients np.polyfit gave the reference's two functions (physics_methods.py:488-568), read
back from its module after one call each.  The tables and the fit are the reference's; this repository holds neither.

    python tools/gen_golden_plastdrift.py
"""
import json
import os
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from oracle import gen_golden as gg  # noqa: E402
from oracle.refdriver import RefStepper  # noqa: E402
from opendrift.models import physics_methods as pm  # noqa: E402
from opendrift.models.plastdrift import PlastDrift  # noqa: E402

SX, SY = 'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity'
HS = 'sea_surface_wave_significant_height'
ENV = {'xw': 'x_wind', 'yw': 'y_wind', 'sx': SX, 'sy': SY, 'hs': HS, 'K': 'ocean_vertical_diffusivity'}
NX, NY, LAND = 40, 32, 36
DT = 900.0
FETCHES = ('5000', '25000', '50000')


def fields():
    x = np.linspace(2, 8, NX).astype(np.float32)
    y = np.linspace(59, 63, NY).astype(np.float32)
    X, Y = np.meshgrid(np.linspace(0, 1, NX), np.linspace(0, 1, NY))
    speed = np.maximum(0.0, 44 * X - 4)          # 0 in the four western columns, 40 m/s in the east
    a = 2 * Y - 1
    g = dict(x=x, y=y)
    g['x_wind'], g['y_wind'] = speed * np.cos(a), speed * np.sin(a) + 0.0      # (+ 0.0: no negative zeros in the calm columns)
    g['x_sea_water_velocity'] = 0.05 + 0.25 * Y * np.cos(2 * X)
    g['y_sea_water_velocity'] = 0.1 * np.sin(3 * X)
    g['land_binary_mask'] = (np.arange(NX)[None, :] >= LAND) * np.ones((NY, 1))
    return {k: (v if k in 'xy' else np.ascontiguousarray(v, dtype=np.float32)) for k, v in g.items()}


def wave_fields(which):
    X, Y = np.meshgrid(np.linspace(0, 1, NX), np.linspace(0, 1, NY))
    zero = 0 * X
    w = {'c1': {SX: 0.1 + 0.05 * X, SY: 0.02 + zero, HS: zero}, 'c2': {SX: zero, SY: zero, HS: 1.5 + zero},
         'c3': {SX: -0.1 - 0.05 * X, SY: zero, HS: zero}, 'c4': {HS: 1 + X * Y}}[which]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def horner64(coeff, x):
    """np.polyval on the float64 wind speed: a float64 Horner chain from the leading coefficient."""
    y = np.zeros(len(x), np.float64)
    for c in coeff:
        y = y * x + np.float64(c)
    return y


def by_id(n, ID, a, dtype=None):
    a = np.asarray(a)
    out = np.full((n,) + a.shape[1:], -1 if a.dtype.kind == 'i' else np.nan, dtype or a.dtype)
    out[ID] = a
    return out


def model(g, waves=None, fetch=None, steps=8):
    times = [gg.T0 + timedelta(seconds=float(t)) for t in np.arange(steps + 3) * DT]
    one = np.ones((len(times), 1, 1), np.float32)
    o = PlastDrift(loglevel=50)
    o.set_config('general:use_auto_landmask', False)
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('seed:ocean_only', False)
    o.set_config('general:coastline_approximation_precision', None)      # (its search reads the global landmask, not the reader)
    o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: one * v for k, v in g.items() if k not in 'xy'}))
    if waves:
        o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: one * v for k, v in waves.items()}, name='waves'))
    if fetch:
        o.set_config('drift:tabularised_stokes_drift_fetch', fetch)
    # the defaults the port mirrors
    assert o.get_config('vertical_mixing:mixingmodel') == 'analytical' and o.get_config('drift:vertical_mixing') is True
    assert o.get_config('drift:vertical_advection') is True and o.get_config('drift:use_tabularised_stokes_drift') is True
    assert o.get_config('general:coastline_action') == 'previous'
    assert o.get_config('vertical_mixing:diffusivitymodel') == 'windspeed_Sundby1983'
    assert o.get_config('drift:current_uncertainty') == 0 and o.get_config('drift:wind_uncertainty') == 0
    assert o.elements.variables['terminal_velocity']['default'] == 0.01
    assert o.elements.variables['terminal_velocity']['dtype'] == np.float32 and type(o.elements).__mro__[1].__name__ == 'Lagrangian3DArray'
    zero = {'fallback': 0}
    assert PlastDrift.required_variables == {      # plastdrift.py:44-57, what opendrift_amd/plastdrift.py restates
        'x_sea_water_velocity': zero, 'y_sea_water_velocity': zero, 'sea_surface_height': zero, SX: zero, SY: zero, HS: zero,
        'x_wind': zero, 'y_wind': zero, 'ocean_vertical_diffusivity': {'fallback': 0.02, 'profiles': True},
        'ocean_mixed_layer_thickness': {'fallback': 50}, 'sea_floor_depth_below_sea_level': {'fallback': 10000},
        'land_binary_mask': {'fallback': None}}
    assert o._config['vertical_mixing:mixingmodel']['enum'] == ['randomwalk', 'analytical']
    assert o._config['drift:tabularised_stokes_drift_fetch']['enum'] == ['5000', '25000', '50000']
    assert o._config['drift:tabularised_stokes_drift_fetch']['default'] == '25000'
    from opendrift.models.oceandrift import OceanDrift
    assert OceanDrift(loglevel=50).get_config('drift:use_tabularised_stokes_drift') is False
    return o


def check_environment(o, fetch, replaced_stokes, replaced_hs):
    """The float32 environment against the issue's reading of the arithmetic, from the reference's own coefficients."""
    e = o.environment
    xw, yw = np.asarray(e.x_wind), np.asarray(e.y_wind)
    for k in ENV.values():
        assert getattr(e, k).dtype == np.float32, k
    # get_environment hands the functions MASKED float32 arrays, and a masked array ** 2 is float64 (np.ma.power takes the exponent
    # as a 0-d int64 array, which is not a weak scalar): the wind speed is formed in float64 from the widened components
    mxw, myw = np.ma.array(xw), np.ma.array(yw)
    assert (mxw ** 2).dtype == np.float64 and (xw ** 2).dtype == np.float32
    ws = np.sqrt(xw.astype(np.float64) ** 2 + yw.astype(np.float64) ** 2)
    ws[ws > 30] = 30
    rx, ry = (np.ma.getdata(r) for r in pm.wave_stokes_drift_parameterised((mxw, myw), fetch))
    rh = np.ma.getdata(pm.wave_significant_height_parameterised((mxw, myw), fetch))
    assert rx.dtype == ry.dtype == rh.dtype == np.float64
    wf = horner64(pm.__stokes_coefficients__[fetch], ws)
    assert pm.__stokes_coefficients__[fetch].dtype == np.float64 and pm.__stokes_hs_coefficients__[fetch].dtype == np.float64
    assert np.array_equal(rx, xw.astype(np.float64) * wf) and np.array_equal(ry, yw.astype(np.float64) * wf)
    assert np.array_equal(rh, horner64(pm.__stokes_hs_coefficients__[fetch], ws))
    if replaced_stokes:
        assert np.array_equal(np.asarray(getattr(e, SX)), rx.astype(np.float32))
        assert np.array_equal(np.asarray(getattr(e, SY)), ry.astype(np.float32))
    if replaced_hs:
        assert np.array_equal(np.asarray(getattr(e, HS)), rh.astype(np.float32))


def run_case(name, g, N, steps, lon, lat, tv, waves=None, fetch=None, env_only=False, replaced=(True, True), seed=40):
    o = model(g, waves, fetch, steps)
    o.seed_elements(lon=lon, lat=lat, z=0.0, time=gg.T0, terminal_velocity=tv)
    st = RefStepper(o, DT, steps)
    assert st.n_total == N
    rec = {'back': 0}
    ref_depth, ref_coast = o.update_particle_depth, o.interact_with_coastline

    def update_particle_depth():
        K, w = o.environment.ocean_vertical_diffusivity, o.elements.terminal_velocity
        assert K.dtype == np.float32 and w.dtype == np.float32 and (K / w).dtype == np.float32
        scale = np.asarray(K / w).astype(np.float64)          # what np.random.exponential makes of its float32 argument
        n = o.num_elements_active()
        s0 = np.random.get_state()
        ref_depth()
        s1 = np.random.get_state()
        np.random.set_state(s0)
        E = np.random.standard_exponential(n)
        s2 = np.random.get_state()
        assert all(np.array_equal(u, v) for u, v in zip(s1, s2))          # both ways of drawing consume the stream alike
        z = np.asarray(o.elements.z)
        assert z.dtype == np.float64 and np.array_equal(z, -(scale * E)), 'exponential(scale, n) != scale * standard_exponential(n)'
        rec['E'], rec['zd'] = E, z.copy()

    def interact_with_coastline(*a, **kw):
        before = np.array(o.elements.lon, copy=True), np.asarray(o.elements.ID).copy()
        ref_coast(*a, **kw)
        if len(before[0]) == len(o.elements.lon):
            rec['back'] += int((before[0] != np.asarray(o.elements.lon)).sum())

    o.update_particle_depth, o.interact_with_coastline = update_particle_depth, interact_with_coastline
    out = {}
    np.random.seed(seed)
    for k in range(steps):
        st.step()
        ID = np.asarray(o.elements.ID, dtype=int)
        assert (np.diff(ID) > 0).all()
        check_environment(o, fetch or '25000', *replaced)
        for short, var in ENV.items():
            out.setdefault(short, []).append(by_id(N, ID, np.asarray(getattr(o.environment, var))))
        if env_only:
            continue
        assert o.elements.z.dtype == np.float64
        out.setdefault('E', []).append(by_id(N, ID, rec['E']))
        out.setdefault('zd', []).append(by_id(N, ID, rec['zd']))
        s_ = st.state()
        for kk, v in zip(('lon', 'lat', 'z', 'status'), s_):
            out.setdefault(kk, []).append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(lon0=lon, lat0=lat, tv=tv)
    if not env_only:
        back = rec['back']
        o.interact_with_coastline(final=True)      # what run() does behind its loop (basemodel/__init__.py:2310)
        out['end_lon'], out['end_lat'], out['end_z'], out['end_status'] = st.state()
        rec['back_at_end'] = rec['back'] - back
    if not env_only:
        out['status_categories'] = np.array(o.status_categories)
    print(name, 'active at end', o.num_elements_active(), 'moved back', rec['back'], 'of them behind the loop', rec.get('back_at_end'))
    return {name + '_' + k: v for k, v in out.items()}, rec


def negative_scale_raises():
    for bad in (np.array([1.0, -1.0]), np.array([1.0, -0.0])):
        try:
            np.random.exponential(scale=bad, size=2)
        except ValueError as e:
            assert 'scale < 0' in str(e)
        else:
            raise AssertionError('np.random.exponential accepted the scale %r' % bad)
    assert np.isnan(np.random.exponential(scale=np.array([np.nan]), size=1)).all()
    assert np.random.exponential(scale=np.array([0.0]), size=1)[0] == 0 and np.signbit(-np.random.exponential(scale=np.array([0.0]), size=1))[0]


def main():
    g = fields()
    out = {'g_' + k: v for k, v in g.items()}
    out['dt'] = np.float64(DT)
    rng = np.random.default_rng(40)
    N = 300
    lon = rng.uniform(g['x'][1], g['x'][34], N)
    lat = rng.uniform(g['y'][3], g['y'][-4], N)
    tv = np.exp(rng.uniform(np.log(1e-4), np.log(0.1), N)).astype(np.float32)
    negative_scale_raises()
    a, _ = run_case('a', g, N, 8, lon, lat, tv)
    out.update(a)
    ws = np.hypot(a['a_xw'][0].astype(np.float64), a['a_yw'][0])
    print('a: wind speed above the cap', int((ws > 30).sum()), 'below', int((ws < 30).sum()), 'exactly 0', int((ws == 0).sum()))
    assert (ws > 30).sum() >= 10 and (ws < 30).sum() >= 10 and (ws == 0).sum() >= 3
    zd = -a['a_zd'][np.isfinite(a['a_zd'])]
    print('a: depths %.3g .. %.3g m' % (zd[zd > 0].min(), zd.max()))
    assert zd.max() / zd[zd > 0].min() > 100
    assert (a['a_status'][-1] == 0).sum() >= 250
    for f, name in (('5000', 'b5'), ('50000', 'b50')):
        b, _ = run_case(name, g, N, 1, lon, lat, tv, fetch=f, env_only=True)
        out.update(b)
    n = 40
    lonc, latc = lon[:n], lat[:n]
    for name, replaced in (('c1', (False, True)), ('c2', (True, False)), ('c3', (False, True)), ('c4', (True, False))):
        w = wave_fields(name)
        c, _ = run_case(name, g, n, 1, lonc, latc, tv[:n], waves=w, env_only=True, replaced=replaced)
        for k, v in w.items():        # what the reader gave is what the environment holds where nothing was replaced
            out['%s_w_%s' % (name, {SX: 'sx', SY: 'sy', HS: 'hs'}[k])] = v
        if not replaced[0]:
            assert (c[name + '_sx'] != 0).all()
        if not replaced[1]:
            assert (c[name + '_hs'] >= 1).all()
        out.update(c)
    assert (out['c3_sx'] < 0).all() and (out['c3_sy'] == 0).all()
    nd = 60
    # where the reference's land begins at these latitudes: the easternmost of a row of probe elements that is not 'seeded_on_land'
    probe = model(g)
    plon = np.linspace(float(g['x'][LAND - 3]), float(g['x'][LAND]), 400)
    probe.seed_elements(lon=plon, lat=np.full(400, 61.0), z=0.0, time=gg.T0)
    pst = RefStepper(probe, DT, 1)
    pst.step()
    edge = float(plon[np.asarray(probe.elements.ID, dtype=int)].max())
    print('d: land begins east of %.4f degE' % edge)
    lond = edge - rng.uniform(0.001, 0.03, nd)
    latd = rng.uniform(g['y'][3], g['y'][-4], nd)
    tvd = rng.uniform(0.05, 0.1, nd).astype(np.float32)
    # Two anchors in opposite corners of the grid, the eastern one on land ('seeded_on_land' in the first step).  The reference's
    # Nearest2DInterpolator maps a position to round((x - xmin) / (xmax - xmin) * len(x)) of the BLOCK it is handed
    # (interpolators.py:32-37), so where the land begins depends on the block.  The oracle's GridReader hands out the whole grid; a
    # reader that cuts its blocks to the box the elements can reach -- the reference's file readers, and the port's GridReader --
    # hands out the same block only when that box spans the grid, which the anchors see to.
    lond = np.concatenate([lond, [float(g['x'][0]) + 0.01, float(g['x'][-1]) - 0.01]])
    latd = np.concatenate([latd, [float(g['y'][0]) + 0.01, float(g['y'][-1]) - 0.01]])
    tvd = np.concatenate([tvd, np.float32([0.05, 0.05])])
    d, rec = run_case('d', g, nd + 2, 8, lond, latd, tvd)
    assert rec['back'] >= 3, rec['back']
    assert (d['d_status'][-1][:nd + 1] == 0).all() and d['d_status'][-1][nd + 1] == 1
    out.update(d)
    path = os.path.join(gg.GOLD, 'c40_plastdrift.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000000
    tables = {f: {'stokes': [float(c) for c in pm.__stokes_coefficients__[f]], 'hs': [float(c) for c in pm.__stokes_hs_coefficients__[f]]}
              for f in FETCHES}
    for f in FETCHES:
        assert np.array_equal(np.array(json.loads(json.dumps(tables[f]))['stokes']), pm.__stokes_coefficients__[f])
        assert len(tables[f]['stokes']) == (4 if f == '5000' else 7) and len(tables[f]['hs']) == 2
    with open(os.path.join(gg.GOLD, 'stokes_tables.json'), 'w') as fh:
        json.dump(tables, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
