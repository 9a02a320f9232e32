"""TEST INFRASTRUCTURE: a plain `OpenOil()` run -- no `weathering_model` -- in its DEFAULT configuration (current uncertainty 0.05 in
the main sample and in every Runge-Kutta stage, wind uncertainty 0.5, Stokes drift, vertical mixing with the oil physics) on the
scenario of golden c14: its reader fields, seed positions, depths and film thicknesses, 'runge-kutta4', vertical_mixing:timestep 60,
as oracle/gen_golden_noise.py configures the reference.  Used by tests/test_gpu_openoil_plain_run.py and by
tools/gen_golden_openoil_plain_run.py, which records the run (golden c40) on the commit in front of the weathering."""
from datetime import datetime, timedelta

import numpy as np

T0 = datetime(2020, 1, 1)
NAMES = ('x_wind', 'y_wind', 'ocean_mixed_layer_thickness', 'sea_floor_depth_below_sea_level', 'x_sea_water_velocity',
         'y_sea_water_velocity', 'sea_water_temperature', 'sea_water_salinity')
STEPS = 6
RNGS = ('device', 'numpy')


def plain_run(OpenOil, readers, g, rng):
    """{name: array}: the result buffer (float32 [element, output time]) and, by element ID, the final float64 state, the oil's
    property slots and the sampled environment of the last step."""
    np.random.seed(0)           # the droplet diameters of the elements seeded below the surface; every draw of rng='numpy'
    o = OpenOil(loglevel=50, seed=0, rng=rng)
    times = [T0 + timedelta(seconds=float(t)) for t in g['g_t']]
    o.add_reader(readers.GridReader(g['g_x'], g['g_y'], times, {k: g['g_' + k] for k in NAMES}))
    o.set_config('general:use_auto_landmask', False)
    o.set_config('environment:fallback:land_binary_mask', 0)
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('vertical_mixing:timestep', float(g['dt_mix']))
    # OpenOil's defaults, untouched (openoil.py:493-499)
    assert o.get_config('drift:current_uncertainty') == 0.05 and o.get_config('drift:wind_uncertainty') == 0.5
    assert o.get_config('drift:vertical_mixing') is True and o.get_config('drift:stokes_drift') is True
    for p in ('evaporation', 'emulsification', 'dispersion'):
        assert o.get_config('processes:' + p) is False
    n = g['lon'].shape[1]
    o.seed_elements(lon=g['lon'][0], lat=g['lat'][0], z=g['z'][0], time=T0, m3_per_hour=7., oil_film_thickness=g['film'],
                    oil_type={'density': float(g['oil_density']), 'viscosity': float(g['oil_viscosity']),
                              'oil_water_interfacial_tension': float(g['interfacial_tension'])})
    o.run(time_step=float(g['dt']), steps=STEPS)
    out = {'result_' + k: np.array(o.result[k]) for k in ('lon', 'lat', 'z', 'status')}
    out['categories'] = np.array(o.status_categories)
    for k in ('lon', 'lat', 'z'):
        out[k] = np.full(n, np.nan)
    out['status'] = np.full(n, -1)
    for d in (o.elements, o.elements_deactivated):
        ids = np.asarray(d.ID)
        for k in ('lon', 'lat', 'z'):
            out[k][ids] = getattr(d, k)
        out['status'][ids] = d.status
    e = o.elements
    for name in o.aux_properties:
        out['property_' + name] = np.full(n, np.nan, np.float32)
        out['property_' + name][e.ID] = getattr(e, name)
    env = o.environment                                       # (with the noise of the last step's main sample in it)
    for name in ('x_wind', 'x_sea_water_velocity', 'sea_water_temperature'):
        out['env_' + name] = np.full(n, np.nan, np.float32)
        out['env_' + name][o.P.ids()] = getattr(env, name)
    return o, out
