"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c39_openoil_weathering.npz from the REFERENCE ITSELF.

The reference's own OpenOil (opendrift/models/openoil/openoil.py) with weathering_model='noaa' runs through oracle/refshim.py +
oracle/refdriver.py.  adios_db is not installed: the oil is a stub that carries the component table (mass_fraction,
gnome_oil['boiling_point'], molecular_weight), bulltime, bullwinkle, emulsion_water_fraction_max and oil_water_surface_tension(), and
binds the reference's OWN vapor_pressure function (adios/oil.py:143-169).  oo.Density / oo.KinematicViscosity are replaced by the two
curves of the table form of an oil, evaluated in float64:

    rho(T) = rho_ref - k (T - T_ref)            nu(T) = nu_ref exp(B / T - B / T_ref)

Cases (a small lon / lat grid with wind 2 .. 15 m/s from west to east and 2 .. 20 degC from south to north, constant in time):
  (a) eight components, evaporation + emulsification + dispersion, 900 s steps, a third of the elements seeded below the surface;
  (b) (a)'s oil with `half_time` biodegradation on top and a continuous release over the first hour;
  (c) one component, `Adcroft` biodegradation, a two-entry max_water_fraction below Y_max for every element (it overrides Y_max);
  (d) every element older than 24 h (no evaporation) and a wave-height reader;
  (r) (a) with drift:vertical_mixing off and land east of 7.46 degE (a few elements start on it, a few more strand): the whole-run
      case.  Only the grid (g_*), the seeding, and status, z and the four masses behind every step are stored, by element ID,
      deactivated elements included: what get_oil_budget sums (:1241-1306; xarray is not installed, so the budget itself is formed
      by the test from these with the reference's masks).
The one-entry form of max_water_fraction cannot be recorded: the reference subtracts two lists there (openoil.py:879-883) and
raises TypeError.

Stored per step and by element ID (NaN / -1 where the element is not present): the state in front of oil_weathering_noaa (s0_*: the
nine weathering variables, z, age_seconds, oil_film_thickness, bulltime, the two half times, the float32 environment), the state
behind the property update (p_*), behind evaporation (e_*), emulsification (m_*), dispersion (d_*) and biodegradation (b_*) -- only
what the process can change -- with mass_components behind evaporation, dispersion and biodegradation (mc_init in front of the first
step: nothing else changes it).  e_K / b_fraction: the float32 mass transport coefficient and Adcroft's float32 fraction as
NumPy formed them in that call (its float32 pow / exp are not libm's: the tests tell the elements on which both agree).  hs_after: the float32 wave height behind the step -- what calculate_missing_environment_variables
had derived from the wind before update() ran, unchanged by the weathering.  dtype_<name>: the dtype the reference's array had behind the step; asserted against DTYPES.

Conditions asserted so that the file cannot hide a failure (case (a)): the evaporated fraction after the first step spans
0.05 .. 0.2; the water fraction after the last step spans 0.1 .. Y_max with >= 5 elements at the cap and >= 5 below; >= 5 elements
on each side of wind_speed >= 10 and >= 5 with zero breaking fraction; the emulsion viscosity grows by more than a factor of 100 for
some element; every stored value of a present element is finite; mass_oil + mass_evaporated > 0 everywhere.

    python tools/gen_golden_openoil_weathering.py
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
from opendrift.models.openoil import openoil as oo  # noqa: E402
from opendrift.models.openoil.adios import oil as adios_oil  # noqa: E402

VARS = ('mass_oil', 'mass_evaporated', 'mass_dispersed', 'mass_biodegraded', 'fraction_evaporated', 'water_fraction',
        'interfacial_area', 'density', 'viscosity')
EXTRA = ('z', 'age_seconds', 'oil_film_thickness', 'bulltime', 'biodegradation_half_time_droplet', 'biodegradation_half_time_slick')
ENV = {'xwind': 'x_wind', 'ywind': 'y_wind', 'temp': 'sea_water_temperature', 'hs': 'sea_surface_wave_significant_height',
       'tp': 'sea_surface_wave_period_at_variance_spectral_density_maximum',
       'tm02': 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'}
# what each process can change
STAGE = {'p': ('density', 'viscosity', 'fraction_evaporated'), 'e': ('mass_oil', 'mass_evaporated'),
         'm': ('interfacial_area', 'water_fraction'), 'd': ('mass_oil', 'mass_dispersed'), 'b': ('mass_oil', 'mass_biodegraded')}
# the dtypes in front of and behind every step: the element type declares the variables float32 (openoil.py:105-207), but the arrays
# the reference works on are float64 from the release on, also behind a continuous release that extends them; the environment is
# float32.  The device code follows this: float64 state, float32 environment chains.
DTYPES = {k: 'float64' for k in VARS + EXTRA[1:]}

OIL8 = dict(mass_fraction=[0.02, 0.03, 0.24, 0.13, 0.13, 0.15, 0.15, 0.15],
            boiling_point=[350., 400., 425., 520., 600., 690., 790., 900.],
            molecular_weight=[85., 105., 125., 165., 220., 300., 400., 520.],
            density=870., density_ref_temp=288.15, density_k=0.7, viscosity=2.0e-5, viscosity_ref_temp=288.15, viscosity_B=2500.,
            bullwinkle_fraction=0.1, bullwinkle_time=None, emulsion_water_fraction_max=0.7, oil_water_interfacial_tension=0.025)
OIL1 = dict(OIL8, mass_fraction=[1.0], boiling_point=[480.], molecular_weight=[140.], bullwinkle_fraction=0.02)
CASES = {
    'a': dict(N=150, steps=12, dt=900., oil=OIL8, sub=3, processes=dict(evaporation=True, emulsification=True, dispersion=True)),
    'b': dict(N=60, steps=6, dt=900., oil=OIL8, sub=3, release=3600.,
              processes=dict(evaporation=True, emulsification=True, dispersion=True, biodegradation=True), method='half_time'),
    'c': dict(N=60, steps=6, dt=900., oil=OIL1, sub=3, mwf={'temperatures': [5.0, 15.0], 'max_water_fraction': [0.5, 0.7]},
              processes=dict(evaporation=True, emulsification=True, dispersion=True, biodegradation=True), method='Adcroft'),
    'd': dict(N=60, steps=4, dt=900., oil=OIL8, sub=0, age=90000., hs=True,
              processes=dict(evaporation=True, emulsification=True, dispersion=True)),
    'r': dict(N=150, steps=12, dt=900., oil=OIL8, sub=3, mixing=False, land=36, light=True,
              processes=dict(evaporation=True, emulsification=True, dispersion=True)),
}


class Curve:
    def __init__(self, f):
        self.f = f

    def at_temp(self, T):
        return self.f(np.asarray(T, dtype=np.float64)) if np.ndim(T) else float(self.f(np.float64(T)))


def density_curve(oil):
    return Curve(lambda T: oil['density'] - oil['density_k'] * (T - oil['density_ref_temp']))


def viscosity_curve(oil):
    return Curve(lambda T: oil['viscosity'] * np.exp(oil['viscosity_B'] / T - oil['viscosity_B'] / oil['viscosity_ref_temp']))


class StubOil:
    name = 'STUB OIL'
    oil = None
    vapor_pressure = adios_oil.OpendriftOil.vapor_pressure       # the reference's own function

    def __init__(self, d):
        self.mass_fraction = np.asarray(d['mass_fraction'], dtype=np.float64)
        self.molecular_weight = np.asarray(d['molecular_weight'], dtype=np.float64)
        self.gnome_oil = {'boiling_point': list(d['boiling_point']), 'emulsion_water_fraction_max': d['emulsion_water_fraction_max']}
        self.bulltime = -999. if d['bullwinkle_time'] is None else d['bullwinkle_time']       # adios/oil.py:125-130
        self.bullwinkle = d['bullwinkle_fraction']
        self.emulsion_water_fraction_max = d['emulsion_water_fraction_max']
        self._sigma = d['oil_water_interfacial_tension']

    def oil_water_surface_tension(self):
        return self._sigma

    def valid(self):
        return True


def fields(hs, land=None):
    nx, ny = 40, 32
    x = np.linspace(2, 8, nx).astype(np.float32)
    y = np.linspace(59, 63, ny).astype(np.float32)
    X, Y = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
    g = dict(x=x, y=y)
    g['x_wind'] = 2 + 13 * X
    g['y_wind'] = 0 * X
    g['sea_water_temperature'] = 2 + 18 * Y
    g['x_sea_water_velocity'] = 0.05 * np.cos(3 * Y)
    g['y_sea_water_velocity'] = 0.05 * np.sin(3 * X)
    g['sea_water_salinity'] = 30 + 5 * X
    g['sea_floor_depth_below_sea_level'] = 100 + 50 * X
    g['ocean_mixed_layer_thickness'] = 30 + 20 * Y
    if hs:
        g['sea_surface_wave_significant_height'] = 0.5 + 2.5 * X * Y
    if land is not None:
        g['land_binary_mask'] = (np.arange(nx)[None, :] >= land) * np.ones((ny, 1))
    return {k: (v if k in 'xy' else np.ascontiguousarray(v, dtype=np.float32)) for k, v in g.items()}


def by_id(n, ID, a, dtype=None):
    a = np.asarray(a)
    out = np.full((n,) + a.shape[1:], np.nan, dtype or a.dtype)
    out[ID] = a
    return out


def case(name):
    C = CASES[name]
    N, STEPS, DT, oil = C['N'], C['steps'], C['dt'], C['oil']
    g = fields(C.get('hs', False), C.get('land'))
    times = [gg.T0 + timedelta(seconds=float(t)) for t in np.arange(STEPS + 3) * DT]
    one = np.ones((len(times), 1, 1), np.float32)
    oo.adios.get_oil_names = lambda location=None: ['STUB OIL']
    oo.Density = lambda o_: density_curve(oil)
    oo.KinematicViscosity = lambda o_: viscosity_curve(oil)
    o = oo.OpenOil(loglevel=50, weathering_model='noaa')
    o.oiltype = StubOil(oil)
    o.oil_name = 'STUB OIL'
    o.store_oil_seed_metadata = lambda **kw: None
    o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: one * v for k, v in g.items() if k not in 'xy'}))
    o.set_config('general:use_auto_landmask', False)
    if 'land' in C:
        o.set_config('seed:ocean_only', False)
    else:
        o.set_config('environment:fallback:land_binary_mask', 0)
    if C.get('mixing') is False:
        o.set_config('drift:vertical_mixing', False)
    o.set_config('drift:current_uncertainty', 0)
    o.set_config('drift:wind_uncertainty', 0)
    o.set_config('drift:stokes_drift', False)
    o.set_config('vertical_mixing:timestep', 60)
    for p in ('evaporation', 'emulsification', 'dispersion', 'biodegradation'):
        o.set_config('processes:' + p, bool(C['processes'].get(p, False)))
    if 'method' in C:
        o.set_config('biodegradation:method', C['method'])
    assert o.get_config('processes:update_oilfilm_thickness') is False
    rng = np.random.default_rng(39 + ord(name))
    lon = rng.uniform(g['x'][3], g['x'][-4], N)
    lat = rng.uniform(g['y'][3], g['y'][-4], N)
    z = np.zeros(N)
    if C['sub']:
        z[::C['sub']] = -rng.uniform(0.5, 20, len(z[::C['sub']]))
    np.random.seed(39)
    t_seed = [gg.T0, gg.T0 + timedelta(seconds=C['release'])] if 'release' in C else gg.T0
    o.seed_elements(lon=lon, lat=lat, z=z, time=t_seed, number=N, m3_per_hour=2.0, oil_film_thickness=0.001, wind_drift_factor=0.02,
                    biodegradation_half_time_droplet=0.8, biodegradation_half_time_slick=2.5)
    if 'age' in C:
        o.elements_scheduled.age_seconds = np.full(N, C['age'], np.float64)
    seeded_mass = np.array(np.atleast_1d(o.elements_scheduled.mass_oil) * np.ones(N))
    assert seeded_mass.dtype == np.float64
    st = RefStepper(o, DT, STEPS)
    assert st.n_total == N
    if 'mwf' in C:        # prepare_run reads it from max_water_fraction.json by oil name (:699-713)
        o.max_water_fraction = C['mwf']
    ncomp = len(oil['mass_fraction'])
    mc = o.noaa_mass_balance['mass_components']
    assert mc.dtype == np.float64 and mc.shape == (N, ncomp)
    out = {'mc_init': np.array(mc, copy=True), 'seeded_mass': seeded_mass}
    rec = {}

    def snap(stage, names):
        e = o.elements
        ID = np.asarray(e.ID, dtype=int)
        for k in names:
            rec.setdefault(stage + '_' + k, []).append(by_id(N, ID, getattr(e, k)))

    def snap_p():
        if rec.get('_p_done'):
            return
        rec['_p_done'] = True
        snap('p', STAGE['p'])
        rec.setdefault('p_temp', []).append(by_id(N, np.asarray(o.elements.ID, dtype=int), o.environment.sea_water_temperature))

    def wrap(method, stage, has_mc):
        ref = getattr(o, method)

        def f():
            snap_p()
            ID = np.asarray(o.elements.ID, dtype=int)
            if stage == 'e':      # the reference's own float32 mass transport coefficient of this call (NumPy's powf)
                K = oo.noaa.mass_transport_coeff(o.wind_speed())
                assert K.dtype == np.float32
                rec.setdefault('e_K', []).append(by_id(N, ID, K))
            if stage == 'b' and C.get('method') == 'Adcroft':      # Adcroft's float32 fraction as NumPy evaluates :595-602 here
                swt = o.environment.sea_water_temperature.copy()
                swt[swt > 100] -= 273.15
                fr = 1 - np.exp(-(o.time_step.total_seconds() / (3600 * 24)) / ((12) * (3**((20 - swt) / 10))))
                assert fr.dtype == np.float32
                rec.setdefault('b_fraction', []).append(by_id(N, ID, fr))
            ref()
            snap(stage, STAGE[stage])
            if has_mc:
                rec.setdefault(stage + '_mc', []).append(np.array(o.noaa_mass_balance['mass_components'], copy=True))
        setattr(o, method, f)
    wrap('evaporation_noaa', 'e', True)
    wrap('emulsification_noaa', 'm', False)
    wrap('disperse_noaa', 'd', True)
    if C['processes'].get('biodegradation'):
        wrap('biodegradation', 'b', True)
    ref_noaa = o.oil_weathering_noaa

    def noaa():
        e = o.elements
        ID = np.asarray(e.ID, dtype=int)
        assert (np.diff(ID) > 0).all()
        snap('s0', VARS + EXTRA)
        for k in DTYPES:
            assert str(getattr(e, k).dtype) == DTYPES[k], (k, getattr(e, k).dtype)
        present = np.zeros(N, bool)
        present[ID] = True
        rec.setdefault('s0_present', []).append(present)
        for k, v in ENV.items():
            rec.setdefault('s0_env_' + k, []).append(by_id(N, ID, getattr(o.environment, v)))
            assert getattr(o.environment, v).dtype == np.float32
        rec['_p_done'] = False
        ref_noaa()
        for k in DTYPES:
            assert str(getattr(e, k).dtype) == DTYPES[k], (k, getattr(e, k).dtype)
        rec.setdefault('hs_after', []).append(by_id(N, ID, o.environment.sea_surface_wave_significant_height))
    o.oil_weathering_noaa = noaa
    status, zz = [], []
    for k in range(STEPS):
        st.step()
        s_ = st.state()
        status.append(s_[3])
        zz.append(s_[2])
        for kk in VARS[:4]:     # the masses behind the whole step, deactivated elements included (the budget counts them)
            full = np.full(N, np.nan)
            for arr in (o.elements, o.elements_deactivated):
                if len(arr):
                    full[np.atleast_1d(arr.ID).astype(int)] = getattr(arr, kk)
            rec.setdefault('end_' + kk, []).append(full)
    for k, v in rec.items():
        if not k.startswith('_'):
            assert len(v) == STEPS, (k, len(v))
            out[k] = np.stack(v)
    out['end_status'], out['end_z'] = np.stack(status), np.stack(zz)
    for k in DTYPES:
        out['dtype_' + k] = np.array(DTYPES[k])
    P = out['s0_present']
    for k, v in out.items():     # every stored value of a present element is finite
        if v.dtype.kind == 'f' and v.shape[:2] == P.shape and k.split('_')[0] in ('s0', 'p', 'e', 'm', 'd', 'b') and 'env_' not in k:
            assert np.isfinite(v[P]).all(), k
    assert ((out['s0_mass_oil'] + out['s0_mass_evaporated'])[P] > 0).all()
    cfg = dict(dt=DT, sea_water_density=float(o.sea_water_density()), ncomp=ncomp, method=C.get('method', ''),
               **{'process_' + p: bool(C['processes'].get(p, False)) for p in ('evaporation', 'emulsification', 'dispersion', 'biodegradation')})
    for k, v in oil.items():
        cfg['oil_' + k] = np.nan if v is None else v
    if 'mwf' in C:
        cfg['mwf_temperatures'], cfg['mwf_max_water_fraction'] = C['mwf']['temperatures'], C['mwf']['max_water_fraction']
    out.update({k: np.asarray(v) for k, v in cfg.items()})
    out['lon'], out['lat'], out['z_seed'] = lon, lat, z
    if C.get('light'):
        out = {k: v for k, v in out.items() if k.split('_')[0] not in ('s0', 'p', 'e', 'm', 'd', 'b', 'hs', 'mc')}
        out.update({'g_' + k: v for k, v in g.items()})
        print(name, 'stranded per step', [(int((s_ == o.status_categories.index('stranded')).sum()) if 'stranded' in o.status_categories else 0)
                                          for s_ in out['end_status']], o.status_categories)
        out['status_categories'] = np.array(o.status_categories)
        return {name + '_' + k: v for k, v in out.items()}
    if name == 'a':
        fe, wf = out['p_fraction_evaporated'][1], out['m_water_fraction'][-1]
        surf0 = out['s0_z'][0] == 0
        print('a: fraction evaporated after step 1', np.nanmin(fe[surf0]), np.nanmax(fe[surf0]), 'water fraction at end', np.nanmin(wf),
              np.nanmax(wf))
        assert np.nanmin(fe[surf0]) <= 0.05 and np.nanmax(fe[surf0]) >= 0.2
        Y = oil['emulsion_water_fraction_max']
        cap = np.isclose(wf, Y, rtol=1e-6)
        assert cap.sum() >= 5 and (wf[~cap & np.isfinite(wf)] < Y).sum() >= 5 and np.nanmin(wf) <= 0.1
        ws = np.hypot(out['s0_env_xwind'][0], out['s0_env_ywind'][0])
        assert (ws >= 10).sum() >= 5 and (ws < 10).sum() >= 5 and (ws <= 5).sum() >= 5
        growth = np.nanmax(out['p_viscosity'][-1] / out['p_viscosity'][0])
        print('a: emulsion viscosity growth', growth)
        assert growth > 100
    print(name, 'present at end', int(P[-1].sum()), 'surface', int((out['s0_z'][-1] == 0).sum()), 'mass_total drift',
          float(abs(sum(np.nansum(out['end_' + k][-1]) for k in VARS[:4]) / seeded_mass.astype(np.float64).sum() - 1)))
    return {name + '_' + k: v for k, v in out.items()}


def main():
    out = {}
    for name in CASES:
        out.update(case(name))
    path = os.path.join(gg.GOLD, 'c39_openoil_weathering.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main()
