"""CPU: the host side of OpenBerg (opendrift_amd/openberg.py) -- config keys and defaults, required_variables, seeding, and every
refusal by name.  Nothing here touches the device."""
import numpy as np
import pytest

import opendrift_amd
from opendrift_amd import _abi
from opendrift_amd.openberg import COEFFICIENTS, OpenBerg
from datetime import datetime

T0 = datetime(2020, 1, 1)


def test_exported_from_the_package_and_in_the_abi():
    assert opendrift_amd.OpenBerg is OpenBerg
    assert 'odr_berg_roll_over' in _abi.EXPORTS and 'odr_berg_advect' in _abi.EXPORTS
    assert _abi.BERG_PROPERTIES == ['sail', 'draft', 'length', 'width', 'iceb_x_velocity', 'iceb_y_velocity']
    assert _abi.NVAR == 26


def test_config_keys_and_defaults():
    o = OpenBerg(loglevel=50)
    want = {'drift:wave_rad': True, 'drift:stokes_drift': False, 'drift:coriolis': True, 'drift:sea_surface_slope': False,
            'drift:vertical_profile': False, 'processes:grounding': True, 'processes:roll_over': True, 'processes:melting': False,
            'melting:wave': True, 'melting:lateral': True, 'melting:basal': True}      # openberg.py:357-424
    for k, v in want.items():
        assert o.get_config(k) is v, k
    for k, v in (('sail', 10), ('draft', 90), ('length', 100), ('width', 30)):
        assert o.get_config('seed:' + k) == v
    for k, v in COEFFICIENTS.items():
        assert o.get_config('seed:' + k) == v
    for k in ('drift:wave_rad', 'drift:stokes_drift', 'drift:coriolis', 'processes:grounding', 'processes:roll_over'):
        o.set_config(k, not want[k])
        assert o.get_config(k) is (not want[k])


def test_required_variables():
    rv = OpenBerg.required_variables      # openberg.py:297-321
    assert len(rv) == 20
    assert rv['horizontal_diffusivity']['fallback'] == 100 and rv['sea_floor_depth_below_sea_level']['fallback'] == 10000
    for k in ('x_sea_water_velocity', 'y_sea_water_velocity', 'x_wind', 'y_wind', 'land_binary_mask'):
        assert rv[k]['fallback'] is None
    for k in ('sea_surface_height', 'sea_surface_wave_significant_height', 'sea_surface_wave_from_direction', 'sea_ice_area_fraction',
              'sea_ice_thickness', 'sea_ice_x_velocity', 'sea_ice_y_velocity', 'sea_surface_wave_stokes_drift_x_velocity',
              'sea_surface_wave_stokes_drift_y_velocity', 'sea_surface_x_slope', 'sea_surface_y_slope'):
        assert rv[k]['fallback'] == 0
    o = OpenBerg(loglevel=50)
    # sampled on the device: everything the default configuration reads that has a variable id
    assert all(v in _abi.VARIABLES for v in o.required_variables)
    assert 'sea_ice_thickness' not in o.required_variables and 'sea_surface_wave_from_direction' not in o.required_variables
    o.set_config('environment:constant:sea_ice_thickness', 1.0)
    o.set_config('environment:constant:sea_surface_wave_from_direction', 200.0)
    assert o._scalar_variable('sea_ice_thickness') == 1.0 and o._scalar_variable('sea_surface_wave_from_direction') == 200.0
    assert OpenBerg(loglevel=50)._scalar_variable('sea_ice_thickness') == 0.0


def test_seeding_with_scalars_and_arrays():
    o = OpenBerg(loglevel=50)
    o.seed_elements(lon=[20.0, 20.1, 20.2], lat=[75.0, 75.0, 75.0], time=T0, length=[50.0, 60.0, 70.0], draft=20.0)
    s = o._sched
    assert s['length'].dtype == np.float32 and np.array_equal(s['length'], np.float32([50, 60, 70]))
    assert np.array_equal(s['draft'], np.float32([20, 20, 20])) and np.array_equal(s['sail'], np.float32([10, 10, 10]))
    assert np.array_equal(s['width'], np.float32([30, 30, 30])) and (s['iceb_x_velocity'] == 0).all() and (s['z'] == 0).all()
    assert o.coefficients == {k: float(np.float32(v)) for k, v in COEFFICIENTS.items()}
    o.seed_elements(lon=[20.3], lat=[75.0], time=T0, width=[12.0])
    assert np.array_equal(o._sched['width'], np.float32([30, 30, 30, 12])) and len(o._sched['sail']) == 4
    with pytest.raises(ValueError, match='length'):
        o.seed_elements(lon=[20.0, 20.1], lat=[75.0, 75.0], time=T0, length=[1.0, 2.0, 3.0])
    o2 = OpenBerg(loglevel=50)
    o2.seed_elements(lon=[20.0, 20.1], lat=[75.0, 75.0], time=T0, wind_form_drag_coef=[0.7, 0.7], wave_drag_coef=0.2)
    assert o2.coefficients['wind_form_drag_coef'] == float(np.float32(0.7)) and o2.coefficients['wave_drag_coef'] == float(np.float32(0.2))


@pytest.mark.parametrize('key,word', [('processes:melting', 'temperature and salinity columns'), ('drift:vertical_profile', 'current columns'),
                                      ('drift:sea_surface_slope', 'no variable id')])
def test_refused_configuration(key, word):
    o = OpenBerg(loglevel=50)
    with pytest.raises(NotImplementedError, match=key) as e:
        o.set_config(key, True)
    assert word in str(e.value)
    o.set_config(key, False)


def test_refused_coefficients_that_differ_between_elements():
    o = OpenBerg(loglevel=50)
    with pytest.raises(NotImplementedError, match='water_form_drag_coef'):
        o.seed_elements(lon=[20.0, 20.1], lat=[75.0, 75.0], time=T0, water_form_drag_coef=[0.25, 0.3])
    o.seed_elements(lon=[20.0], lat=[75.0], time=T0, weight_coef=1.0)
    with pytest.raises(NotImplementedError, match='weight_coef'):
        o.seed_elements(lon=[20.0], lat=[75.0], time=T0, weight_coef=0.3)


@pytest.mark.parametrize('name', ['sea_surface_wave_from_direction', 'sea_ice_thickness'])
def test_refused_reader_for_a_scalar_variable(name):
    wanted = ['x_wind', name]

    class Reader:
        variables = wanted
        name = 'r'

        def get_variables(self, *a, **k):
            raise AssertionError
    o = OpenBerg(loglevel=50)
    with pytest.raises(NotImplementedError, match=name):
        o.add_reader(Reader())


def test_refused_sharded_run(monkeypatch):
    from opendrift_amd import distributed as D
    monkeypatch.setattr(D, 'env_world', lambda: (0, 0, 2))
    with pytest.raises(NotImplementedError, match='sharded'):
        OpenBerg(loglevel=50)
