"""CPU: the public surface of OpenOil's NOAA weathering -- the opt-in rule both ways, the table form of an oil and its limits, the
seeded mass, every refusal by name, and that a backward run launches nothing."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from opendrift_amd import _abi
from opendrift_amd.device import weathering_table
from opendrift_amd.openoil import OpenOil

T0 = datetime(2020, 1, 1)
OIL = dict(mass_fraction=[0.2, 0.3, 0.5], boiling_point=[380., 480., 700.], molecular_weight=[90., 150., 350.], density=870., density_k=0.7,
           viscosity=2e-5, viscosity_B=2500., bullwinkle_fraction=0.1, bullwinkle_time=None, emulsion_water_fraction_max=0.8,
           oil_water_interfacial_tension=0.025)


def test_without_the_keyword_nothing_changes():
    o = OpenOil(loglevel=50)
    for p in ('evaporation', 'emulsification', 'dispersion'):
        assert o.get_config('processes:' + p) is False
        with pytest.raises(NotImplementedError, match="weathering_model='noaa'"):
            o.set_config('processes:' + p, True)
    for key in ('processes:biodegradation', 'biodegradation:method', 'seed:m3_per_hour', 'processes:update_oilfilm_thickness'):
        assert key not in o._config
    o.seed_elements(lon=4., lat=60., time=T0, number=10, m3_per_hour=5., oil_type={'density': 900., 'viscosity': 0.01})
    assert o._weather_sched is None and (o._sched['density'] == np.float32(900.)).all()
    for k in ('bulltime', 'biodegradation_half_time_droplet', 'biodegradation_half_time_slick'):     # no such element properties
        with pytest.raises(TypeError, match='Redundant arguments.*' + k):
            o.seed_elements(lon=4., lat=60., time=T0, number=10, **{k: 1.})
    assert o.num_elements_total() == 10
    with pytest.raises(ValueError, match='Unknown oil properties'):
        o.set_oiltype({'density': 900., 'pour_point': 3.})
    with pytest.raises(ValueError, match='ADIOS'):
        o.set_oiltype('GENERIC BUNKER C')
    with pytest.raises(NotImplementedError):
        o.get_oil_budget()


def test_the_keyword_turns_the_reference_defaults_on():
    o = OpenOil(loglevel=50, weathering_model='noaa')
    assert [o.get_config('processes:' + p) for p in ('evaporation', 'emulsification', 'dispersion', 'biodegradation')] == [True, True, True, False]
    assert o.get_config('biodegradation:method') == 'Adcroft' and o.get_config('seed:m3_per_hour') == 1
    assert o.get_config('processes:update_oilfilm_thickness') is False
    o.set_config('processes:biodegradation', True)
    o.set_config('biodegradation:method', 'half_time')
    o.set_oiltype(OIL)
    assert o._weathering_processes() == ['properties', 'evaporation', 'emulsification', 'dispersion', 'half_time']
    with pytest.raises(ValueError, match='Weathering model unknown'):
        OpenOil(loglevel=50, weathering_model='basic')
    with pytest.raises(ValueError, match='ADIOS'):
        o.set_oiltype('GENERIC BUNKER C')


def test_the_oil_is_a_table():
    o = OpenOil(loglevel=50, weathering_model='noaa')
    with pytest.raises(ValueError, match='mass_fraction'):
        o.set_oiltype({'density': 900., 'viscosity': 0.01, 'oil_water_interfacial_tension': 0.03})
    with pytest.raises(ValueError, match='lengths'):
        o.set_oiltype(dict(OIL, boiling_point=[380., 480.]))
    with pytest.raises(ValueError, match='Unknown oil properties'):
        o.set_oiltype(dict(OIL, pour_point=3.))
    n = _abi.OIL_MAXCOMP + 1
    with pytest.raises(ValueError, match='ODR_OIL_MAXCOMP'):
        o.set_oiltype(dict(OIL, mass_fraction=[1. / n] * n, boiling_point=list(np.linspace(350, 900, n)), molecular_weight=[100.] * n))
    with pytest.raises(ValueError, match='one or two entries'):
        o.set_oiltype(dict(OIL, max_water_fraction={'temperatures': [1., 2., 3.], 'max_water_fraction': [.1, .2, .3]}))
    o.set_oiltype(dict(OIL, mass_fraction=[1. / 32] * 32, boiling_point=list(np.linspace(350, 900, 32)), molecular_weight=[100.] * 32))
    o.set_oiltype(OIL)
    assert o.oiltype['density_ref_temp'] == 288.15 and o.oiltype['viscosity_ref_temp'] == 288.15
    # the curves: constants with the defaults, the documented forms otherwise
    assert o.oil_density_at(285.) == 870. - 0.7 * (285. - 288.15)
    assert o.oil_viscosity_at(285.) == 2e-5 * np.exp(2500. / 285. - 2500. / 288.15)
    o.set_oiltype(dict(OIL, density_k=0., viscosity_B=0.))
    assert o.oil_density_at(np.array([270., 300.])).tolist() == [870., 870.] and o.oil_viscosity_at(300.) == 2e-5


def test_component_constants_are_the_vapor_pressure_of_the_reference_formula():
    t = weathering_table(OIL, 1027.)
    bp = np.array(OIL['boiling_point'])
    comp = np.array(t.comp[:]).reshape(4, _abi.OIL_MAXCOMP)
    C = 0.19 * bp - 18
    T = 283.15
    ln = (8.75 + 1.987 * np.log(bp)) * (bp - C)**2 / (0.97 * 1.987 * bp) * (1. / (bp - C) - 1. / (T - C))
    np.testing.assert_allclose(comp[0, :3] * (comp[2, :3] - 1. / (T - comp[1, :3])), ln, rtol=1e-14)
    assert (comp[3, :3] == np.array(OIL['molecular_weight']) / 1000.).all() and (comp[:3, 3:] == 0).all()
    assert t.ncomp == 3 and t.bulltime == -999. and t.bullwinkle == 0.1 and t.y_max == 0.8 and t.mwf_n == 0 and t.sea_water_density == 1027.
    t = weathering_table(dict(OIL, bullwinkle_time=3600., max_water_fraction={'temperatures': [5., 15.], 'max_water_fraction': [.5, .7]}), 1027.)
    assert t.bulltime == 3600. and t.mwf_n == 2 and list(t.mwf_t) == [5., 15.] and list(t.mwf_w) == [.5, .7]


def test_seeded_mass_instantaneous_and_continuous():
    o = OpenOil(loglevel=50, weathering_model='noaa')
    o.seed_elements(lon=4., lat=60., time=T0, number=100, m3_per_hour=2., oil_type=OIL)
    rho = 870. - 0.7 * (285. - 288.15)
    assert (o._weather_sched['mass_oil'] == np.float32(2. * 1. / 100 * rho)).all() and (o._weather_sched['density'] == np.float32(rho)).all()
    assert o._weather_sched['mass_oil'].dtype == np.float64        # float64 of the float32 the schedule holds, like the reference's arrays
    assert (o._sched['density'] == np.float32(rho)).all()
    assert (o._sched['viscosity'] == np.float32(2e-5 * np.exp(2500. / 285. - 2500. / 288.15))).all()
    # a continuous release over three hours, with the element properties of the reference's Oil type
    o.seed_elements(lon=4., lat=60., time=[T0, T0 + timedelta(hours=3)], number=50, m3_per_hour=2., bulltime=7200.,
                    biodegradation_half_time_droplet=0.5, biodegradation_half_time_slick=2.)
    w = o._weather_sched
    assert len(w['mass_oil']) == 150 == o.num_elements_total()
    assert (w['mass_oil'][100:] == np.float32(2. * 3. / 50 * rho)).all() and (w['bulltime'][:100] == 0).all() and (w['bulltime'][100:] == 7200.).all()
    assert (w['biodegradation_half_time_droplet'] == [1.] * 100 + [.5] * 50).all()
    assert (w['biodegradation_half_time_slick'] == [3.] * 100 + [2.] * 50).all() and (w['oil_film_thickness'] == np.float32(0.001)).all()
    # seed:m3_per_hour when the keyword is absent
    o2 = OpenOil(loglevel=50, weathering_model='noaa')
    o2.set_config('seed:m3_per_hour', 4.)
    o2.seed_elements(lon=4., lat=60., time=T0, number=10, oil_type=OIL)
    assert (o2._weather_sched['mass_oil'] == np.float32(4. / 10 * rho)).all()


class _NoDevice:
    def __getattr__(self, k):
        raise AssertionError('the device was asked for ' + k)


def _seeded(**config):
    o = OpenOil(loglevel=50, weathering_model='noaa')
    for k, v in config.items():
        o.set_config(k, v)
    o.seed_elements(lon=4., lat=60., time=T0, number=10, oil_type=OIL)
    o.P = _NoDevice()
    return o


def test_every_refusal_is_by_name():
    o = _seeded(**{'processes:update_oilfilm_thickness': True})
    with pytest.raises(NotImplementedError, match='processes:update_oilfilm_thickness'):
        o.prepare_run()
    o = _seeded()
    o._world = 2
    with pytest.raises(NotImplementedError, match='sharded run'):
        o.prepare_run()
    o = _seeded()
    tm02 = 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'
    o._readers_host['waves'] = (object(), [tm02])
    with pytest.raises(NotImplementedError, match=tm02):
        o.prepare_run()
    with pytest.raises(NotImplementedError, match='TSprofiles'):
        OpenOil(loglevel=50, weathering_model='noaa').set_config('vertical_mixing:TSprofiles', True)


def test_a_backward_run_launches_nothing():
    o = _seeded()
    o.time_step = timedelta(seconds=-900)
    o.oil_weathering()
    assert o._temperature_in_kelvin is False and o.get_oil_budget() is None
    o.time_step = timedelta(seconds=900)
    with pytest.raises(AssertionError, match='oil_weather'):
        o.oil_weathering()


def test_abi_surface():
    for name, n in (('odr_oil_weathering_setup', 4), ('odr_oil_weathering_seed', 6), ('odr_oil_weather', 4), ('odr_oil_weathering_get', 4),
                    ('odr_oil_weathering_set', 4), ('odr_oil_budget', 4)):
        assert name in _abi.EXPORTS and len(_abi._SIGNATURES[name]) == n, name
    assert _abi.WEATHER_RECORD_N == 14 and len(_abi.WEATHER_RECORD) == 13
