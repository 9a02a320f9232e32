"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c28_openberg.npz from the REFERENCE ITSELF.

The reference's own OpenBerg (opendrift/models/openberg.py) runs through oracle/refshim.py + oracle/refdriver.py on a small
lon/lat grid in the Barents Sea: current, wind and sea-ice velocity varying in space, a sea-ice fraction that ramps from 0 to 1
across the domain, a smooth sea floor of 30 - 390 m and a sea-surface height that rises from -3 m to +3 m over the run.
Constant significant wave height 2 m, wave from-direction 200 deg, sea-ice thickness 1 m, horizontal_diffusivity 0.
300 elements, 8 steps of 3600 s, default configuration (wave radiation, Coriolis, grounding, roll-over on; Stokes drift,
melting, vertical profile, sea-surface slope off).

The population mixes small bergs (length from 5 m, draft from 2 m: they make the momentum equation stiff and the solver reject
attempts) with large ones (length up to 300 m, draft up to 200 m: they ground).  A tenth of the elements is seeded stable and with a
draft within 2.5 m of the local sea floor: they ground at once and deground while the sea surface rises.

Stored per step, by element ID (NaN / -1 where an element is not present): the live float64 lon / lat, status and moving; the
float32 environment of the step; sail, draft, length, width before and after roll_over; lat and moving when advect_iceberg starts;
V0 and the result of solve_ivp (float64), the grounded flag, moving after the call; per step nfev and the error norm of every
attempt (recorded by wrapping RK45._estimate_error_norm in SciPy's module while the run lasts -- the reference is not edited).

Conditions asserted here so that the golden cannot hide a failure:
  (a) at least 10 % of the elements roll over in step 1 and at least 10 % never do;
  (b) at least 5 % ground, and at least 5 elements deground later;
  (c) each of the three ice classes (<= 0.15, between, >= 0.9) holds at least 10 % of the elements in some step;
  (d) at least two steps contain a rejected attempt;
  (e) no attempt's error norm lies within 1e-6 of 1 (the seed is re-drawn until this holds);
  (f) every stored value of a present element is finite.

    python tools/gen_golden_openberg.py
"""
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
import scipy.integrate._ivp.rk as scipy_rk  # noqa: E402
import opendrift.models.openberg as ref_openberg  # noqa: E402
from opendrift.models.openberg import OpenBerg  # noqa: E402

DT, STEPS, N = 3600.0, 8, 300
CONSTANTS = {'sea_surface_wave_significant_height': 2.0, 'sea_surface_wave_from_direction': 200.0, 'sea_ice_thickness': 1.0,
             'horizontal_diffusivity': 0.0}
ENV = ('x_sea_water_velocity', 'y_sea_water_velocity', 'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity',
       'x_wind', 'y_wind', 'sea_floor_depth_below_sea_level', 'sea_surface_height', 'sea_surface_wave_significant_height',
       'sea_ice_area_fraction', 'sea_ice_x_velocity', 'sea_ice_y_velocity', 'sea_surface_wave_from_direction', 'sea_ice_thickness')
DIMS = ('sail', 'draft', 'length', 'width')
NORM_MARGIN = 1e-6
ALPHA = 900 / 1027


def fields(nx=41, ny=37, nt=STEPS + 2):
    x = np.linspace(20.0, 24.0, nx)
    y = np.linspace(75.0, 76.2, ny)
    t = np.arange(nt) * DT
    X, Y = np.meshgrid((x - x[0]) / (x[-1] - x[0]), (y - y[0]) / (y[-1] - y[0]))
    one = np.ones((nt, 1, 1))
    g = dict(x=x, y=y, t=t)
    g['x_sea_water_velocity'] = one * (0.25 * np.sin(2 * np.pi * Y) + 0.1)
    g['y_sea_water_velocity'] = one * (0.2 * np.cos(2 * np.pi * X) - 0.05)
    g['x_wind'] = one * (6.0 + 5.0 * np.cos(np.pi * Y))
    g['y_wind'] = one * (-3.0 + 6.0 * X)
    g['sea_ice_area_fraction'] = one * np.clip(1.4 * X - 0.2, 0.0, 1.0)
    g['sea_ice_x_velocity'] = one * (0.08 * np.cos(np.pi * Y))
    g['sea_ice_y_velocity'] = one * (0.06 * np.sin(np.pi * X) - 0.02)
    g['sea_floor_depth_below_sea_level'] = one * (210.0 + 180.0 * np.sin(1.5 * np.pi * X) * np.cos(1.2 * np.pi * Y))
    ramp = (-3.0 + 6.0 * t / (STEPS * DT)).reshape(-1, 1, 1)
    g['sea_surface_height'] = ramp + 0.2 * np.sin(2 * np.pi * X) * np.ones((nt, 1, 1))
    g['land_binary_mask'] = np.zeros((nt, ny, nx))
    return {k: (v if k in 'xyt' else np.ascontiguousarray(v, dtype=np.float32)) for k, v in g.items()}


def bilinear(g, name, lon, lat, it=0):
    fx = (lon - g['x'][0]) / (g['x'][1] - g['x'][0])
    fy = (lat - g['y'][0]) / (g['y'][1] - g['y'][0])
    ix, iy = np.floor(fx).astype(int), np.floor(fy).astype(int)
    wx, wy = fx - ix, fy - iy
    a = g[name][it].astype(np.float64)
    return (a[iy, ix] * (1 - wx) + a[iy, ix + 1] * wx) * (1 - wy) + (a[iy + 1, ix] * (1 - wx) + a[iy + 1, ix + 1] * wx) * wy


def population(g, seed):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(g['x'][4], g['x'][-5], N)
    lat = rng.uniform(g['y'][4], g['y'][-5], N)
    kind = np.arange(N) % 10                     # 0: draft at the sea floor; 1 - 5: small bergs; 6 - 9: large bergs
    small = (kind >= 1) & (kind <= 5)
    length = np.where(small, rng.uniform(5, 40, N), rng.uniform(40, 300, N))
    width = length * rng.uniform(0.3, 1.0, N)
    draft = np.where(small, rng.uniform(2, 15, N), rng.uniform(15, 200, N))
    sail = draft * rng.uniform(0.08, 0.25, N)
    m = kind == 0                                # stable (width >= 0.9 H) with H alpha = local depth + (-2.5 .. 2.5) m
    H = (bilinear(g, 'sea_floor_depth_below_sea_level', lon, lat) + rng.uniform(-2.5, 2.5, N)) / ALPHA
    draft = np.where(m, H * ALPHA, draft)
    sail = np.where(m, H - H * ALPHA, sail)
    width = np.where(m, H * rng.uniform(0.9, 1.0, N), width)
    length = np.where(m, np.maximum(width * rng.uniform(1.0, 1.3, N), length), length)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    # seeded as ARRAYS: float32, the dtype the element type declares (a scalar would become a float64 array, elements.py:219-222)
    return dict(lon=lon, lat=lat, sail=f32(sail), draft=f32(draft), length=f32(length), width=f32(width))


def case(g, pop):
    times = [gg.T0 + timedelta(seconds=float(t)) for t in g['t']]
    o = OpenBerg(loglevel=50)
    o.set_config('general:use_auto_landmask', False)
    o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: v for k, v in g.items() if k not in 'xyt'}))
    for k, v in CONSTANTS.items():
        o.set_config('environment:constant:%s' % k, v)
    for k, v in (('drift:wave_rad', True), ('drift:stokes_drift', False), ('drift:coriolis', True), ('drift:sea_surface_slope', False),
                 ('drift:vertical_profile', False), ('processes:grounding', True), ('processes:roll_over', True), ('processes:melting', False)):
        assert o.get_config(k) is v, k
    o.seed_elements(time=gg.T0, **pop)

    rec = {}
    ref_roll, ref_advect, ref_solve = o.roll_over, o.advect_iceberg, ref_openberg.solve_ivp

    def dims():
        e = o.elements
        assert all(getattr(e, k).dtype == np.float32 for k in DIMS)
        return {k: np.array(getattr(e, k), copy=True) for k in DIMS}

    def roll_over():
        rec['ID'] = np.asarray(o.elements.ID, dtype=int)
        rec['before'] = dims()
        ref_roll()
        rec['after'] = dims()

    def solve_ivp(fun, t_span, y0, **kw):
        assert kw.get('vectorized') is True and set(kw) == {'args', 'vectorized', 't_eval'} and tuple(t_span) == (0, DT)
        rec['V0'] = np.array(y0, dtype=np.float64).reshape(2, -1)
        rec['norms'] = []
        sol = ref_solve(fun, t_span, y0, **kw)
        assert sol.status == 0 and sol.y.dtype == np.float64 and sol.y.shape[1] == 1
        rec['V'] = np.array(sol.y, copy=True).reshape(2, -1)
        rec['nfev'] = sol.nfev
        return sol

    def advect_iceberg():
        e, env = o.elements, o.environment
        assert np.array_equal(rec['ID'], np.asarray(e.ID, dtype=int))
        for k in ENV:
            assert getattr(env, k).dtype == np.float32, k
        for k in ('weight_coef', 'water_form_drag_coef', 'water_skin_drag_coef', 'wind_form_drag_coef', 'wind_skin_drag_coef', 'wave_drag_coef'):
            assert getattr(e, k).dtype == np.float64 and len(np.unique(getattr(e, k))) == 1, k     # seeded as scalars
        assert e.lat.dtype == (np.float32 if o.steps_calculation == 0 else np.float64)      # (elements.py:71-88)
        rec['env'] = {k: np.array(getattr(env, k), copy=True) for k in ENV}
        rec['lat'] = np.array(e.lat, copy=True)
        rec['moving_before'] = np.array(e.moving, copy=True)
        hwall = e.draft - (env.sea_floor_depth_below_sea_level + env.sea_surface_height)
        assert hwall.dtype == np.float32
        rec['grounded'] = np.array(hwall >= 0)
        ref_advect()
        rec['moving_after'] = np.array(e.moving, copy=True)
        assert np.array_equal(np.asarray(e.iceb_x_velocity) == 0, rec['grounded'] | (rec['V'][0] == 0))

    def estimate_error_norm(self, K, h, scale):
        r = ref_norm(self, K, h, scale)
        rec['norms'].append(float(r))
        return r

    o.roll_over, o.advect_iceberg = roll_over, advect_iceberg
    ref_norm = scipy_rk.RK45._estimate_error_norm
    scipy_rk.RK45._estimate_error_norm = estimate_error_norm
    ref_openberg.solve_ivp = solve_ivp
    try:
        st = RefStepper(o, DT, STEPS)
        nan = lambda dtype=np.float64: np.full((STEPS, N), np.nan, dtype)      # noqa: E731
        out = {k: np.full((STEPS + 1, N), np.nan) for k in ('lon', 'lat')}
        out['status'] = np.full((STEPS + 1, N), -1, np.int32)
        out['moving'] = np.full((STEPS + 1, N), -1, np.int32)
        sch = o.elements_scheduled
        out['lon'][0], out['lat'][0], out['status'][0], out['moving'][0] = sch.lon, sch.lat, 0, 1
        for k in ENV:
            out['env_' + k] = nan(np.float32)
        for k in DIMS:
            out[k + '_before'], out[k + '_after'] = nan(np.float32), nan(np.float32)
        out['adv_lat'] = nan()
        for k in ('V0x', 'V0y', 'Vx', 'Vy'):
            out[k] = nan()
        for k in ('grounded', 'moving_before', 'moving_after'):
            out[k] = np.full((STEPS, N), -1, np.int8)
        out['nfev'] = np.zeros(STEPS, np.int32)
        out['error_norms'] = np.full((STEPS, 256), np.nan)
        out['n_active'] = np.zeros(STEPS, np.int32)
        for s in range(STEPS):
            st.step()
            ID = rec['ID']
            out['n_active'][s] = len(ID)
            lon, lat, _, status = st.state()
            out['lon'][s + 1], out['lat'][s + 1], out['status'][s + 1] = lon, lat, status
            out['moving'][s + 1, np.asarray(o.elements.ID, dtype=int)] = o.elements.moving
            for k in ENV:
                out['env_' + k][s, ID] = rec['env'][k]
            for k in DIMS:
                out[k + '_before'][s, ID], out[k + '_after'][s, ID] = rec['before'][k], rec['after'][k]
            out['adv_lat'][s, ID] = rec['lat']
            out['V0x'][s, ID], out['V0y'][s, ID] = rec['V0']
            out['Vx'][s, ID], out['Vy'][s, ID] = rec['V']
            out['grounded'][s, ID], out['moving_before'][s, ID], out['moving_after'][s, ID] = rec['grounded'], rec['moving_before'], rec['moving_after']
            out['nfev'][s] = rec['nfev']
            assert (rec['nfev'] - 2) % 6 == 0 and (rec['nfev'] - 2) // 6 == len(rec['norms']) <= 256
            out['error_norms'][s, :len(rec['norms'])] = rec['norms']
    finally:
        scipy_rk.RK45._estimate_error_norm = ref_norm
        ref_openberg.solve_ivp = ref_solve
    for k in DIMS:
        out['seed_' + k] = np.array(pop[k], copy=True)
    return out


def check(out):
    """The conditions (a) - (f); returns the error norms that violate (e)"""
    present = out['grounded'] >= 0
    rolls = present & ((out['length_before'] != out['length_after']) | (out['width_before'] != out['width_after']))
    # (a roll-over changes length or width; ordering L >= W alone is not one)
    rolled = present & ((np.minimum(out['length_before'], out['width_before']) / (out['sail_before'] + out['draft_before'])).astype(np.float64)
                        < np.sqrt(6 * ALPHA * (1 - ALPHA)))
    assert not (rolled & ~rolls).any()
    fa, fb = rolled[0].sum() / N, (~rolled.any(axis=0)).sum() / N
    grounded = out['grounded'] == 1
    deground = (out['moving_before'] == 0) & (out['moving_after'] == 1)
    a = out['env_sea_ice_area_fraction']
    cls = [np.nanmax(((a <= np.float32(0.15)) & present).sum(axis=1)) / N, np.nanmax(((a > np.float32(0.15)) & (a < np.float32(0.9)) & present).sum(axis=1)) / N,
           np.nanmax(((a >= np.float32(0.9)) & present).sum(axis=1)) / N]
    norms = out['error_norms']
    attempts = np.isfinite(norms).sum(axis=1)
    rejected = (norms >= 1).sum(axis=1)
    print('roll over in step 1 %.3f, never %.3f | ever grounded %.3f, degroundings %d | ice classes %s | attempts %s rejected %s'
          % (fa, fb, grounded.any(axis=0).sum() / N, deground.sum(), ' '.join('%.2f' % c for c in cls), attempts.tolist(), rejected.tolist()))
    assert fa >= 0.1 and fb >= 0.1, '(a)'
    assert grounded.any(axis=0).sum() / N >= 0.05 and deground.any(axis=0).sum() >= 5, '(b)'
    assert min(cls) >= 0.1, '(c)'
    assert (rejected > 0).sum() >= 2, '(d)'
    assert np.array_equal(attempts, (out['nfev'] - 2) // 6)
    for k, v in out.items():      # (f)
        if v.shape == (STEPS, N) and v.dtype.kind == 'f':
            assert np.isfinite(v[present]).all(), k
    known = out['status'] >= 0
    assert np.isfinite(out['lon'][known]).all() and np.isfinite(out['lat'][known]).all()
    return norms[np.abs(norms - 1.0) < NORM_MARGIN]


def main():
    g = fields()
    for seed in range(28, 48):
        out = case(g, population(g, seed))
        bad = check(out)
        print('seed %d: %d error norms within %g of 1' % (seed, len(bad), NORM_MARGIN))
        if len(bad) == 0:
            break
    else:
        raise AssertionError('(e)')
    path = os.path.join(gg.GOLD, 'c28_openberg.npz')
    np.savez_compressed(path, dt=DT, seed=seed, **{('c_' + k): v for k, v in CONSTANTS.items()}, **{('g_' + k): v for k, v in g.items()}, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
