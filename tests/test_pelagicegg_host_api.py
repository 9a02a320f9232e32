"""CPU: the host side of PelagicEggDrift (opendrift_amd/pelagicegg.py) -- what can be checked without a device: the class, its
configuration, its element properties and the C ABI entry of its kernel."""
import os
import re
from datetime import datetime

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = datetime(2020, 1, 1)
REQUIRED = {   # opendrift/models/pelagicegg.py:60-79
    'x_sea_water_velocity': 0, 'y_sea_water_velocity': 0, 'sea_surface_height': 0, 'sea_surface_wave_significant_height': 0,
    'sea_ice_area_fraction': 0, 'x_wind': 0, 'y_wind': 0, 'land_binary_mask': None, 'sea_floor_depth_below_sea_level': 100,
    'ocean_vertical_diffusivity': 0.02, 'ocean_mixed_layer_thickness': 50, 'sea_water_temperature': 10, 'sea_water_salinity': 34,
    'surface_downward_x_stress': 0, 'surface_downward_y_stress': 0, 'turbulent_kinetic_energy': 0,
    'turbulent_generic_length_scale': 0, 'upward_sea_water_velocity': 0}
DEFAULTS = {'diameter': 0.0014, 'neutral_buoyancy_salinity': 31.25, 'density': 1028., 'hatched': 0.}


def model(**kw):
    from opendrift_amd.pelagicegg import PelagicEggDrift
    return PelagicEggDrift(loglevel=50, **kw)


def test_class_and_config_defaults():
    from opendrift_amd.oceandrift import OceanDrift
    o = model()
    assert isinstance(o, OceanDrift)
    assert o.get_config('general:coastline_action') == 'previous'
    assert o.get_config('drift:vertical_mixing') is True
    assert o.get_config('drift:vertical_mixing_at_surface') is True
    assert o.get_config('drift:vertical_advection_at_surface') is True
    assert o.get_config('drift:vertical_advection') is True
    assert OceanDrift(loglevel=50).get_config('drift:vertical_mixing') is False      # (the base class keeps its own)


def test_required_variables_and_their_fallbacks():
    from opendrift_amd import _abi
    from opendrift_amd.pelagicegg import PelagicEggDrift, UNSAMPLED_VARIABLES
    assert {k: v['fallback'] for k, v in PelagicEggDrift.required_variables.items()} == REQUIRED
    o = model()
    for v, fb in REQUIRED.items():
        assert o.get_config('environment:fallback:%s' % v) == fb
        assert o.get_config('environment:constant:%s' % v) is None
    # the four without a device id: accepted, not sampled
    assert set(UNSAMPLED_VARIABLES) == set(REQUIRED) - set(_abi.VARIABLES) and len(UNSAMPLED_VARIABLES) == 4
    assert set(o.required_variables) == set(REQUIRED) - set(UNSAMPLED_VARIABLES)
    o.set_config('environment:constant:turbulent_kinetic_energy', 1e-4)
    assert _abi.NVAR == 26


def test_a_reader_offering_the_unsampled_variables_is_accepted():
    from opendrift_amd import readers
    o = model()
    o.add_reader(readers.ConstantReader({'surface_downward_x_stress': 0.1, 'turbulent_kinetic_energy': 1e-4, 'sea_water_salinity': 33.0}))
    assert o.priority_list == {'sea_water_salinity': ['reader_constant']} or list(o.priority_list) == ['sea_water_salinity']


def test_element_properties_are_float32_with_the_reference_defaults():
    o = model()
    for k, v in DEFAULTS.items():
        assert o.get_config('seed:%s' % k) == v
    assert o.aux_properties == ['diameter', 'neutral_buoyancy_salinity', 'density', 'hatched']
    o.seed_elements(lon=4.0, lat=60.0, number=5, time=T0)
    for k, v in DEFAULTS.items():
        assert o._sched[k].dtype == np.float32 and o._sched[k].shape == (5,) and (o._sched[k] == np.float32(v)).all()
    d = np.linspace(0.001, 0.002, 3)
    o.seed_elements(lon=[4.0, 4.1, 4.2], lat=[60.0, 60.0, 60.0], time=T0, diameter=d, neutral_buoyancy_salinity=33)
    assert o._sched['diameter'].dtype == np.float32 and np.array_equal(o._sched['diameter'][5:], d.astype(np.float32))
    assert (o._sched['neutral_buoyancy_salinity'][5:] == 33).all() and (o._sched['neutral_buoyancy_salinity'][:5] == np.float32(31.25)).all()
    assert len(o._sched['hatched']) == 8
    with pytest.raises(ValueError):
        o.seed_elements(lon=[4.0, 4.1, 4.2], lat=[60.0, 60.0, 60.0], time=T0, diameter=[0.001, 0.002])
    o2 = model()
    o2.set_config('seed:diameter', 0.002)
    o2.seed_elements(lon=4.0, lat=60.0, number=2, time=T0)
    assert (o2._sched['diameter'] == np.float32(0.002)).all()


def test_tsprofiles_is_refused_by_name():
    o = model()
    with pytest.raises(NotImplementedError, match='TSprofiles'):
        o.set_config('vertical_mixing:TSprofiles', True)
    o.set_config('vertical_mixing:TSprofiles', False)


def test_run_takes_the_call_by_call_lane():
    """run() chooses its lane by the methods a class overrides (oceandrift.py, run()): update() is the model's own, so neither
    the fused OceanDrift launch nor the speculated mixing launch (which needs the fused lane) is taken; the class
    does not fuse (fuse_vertical_advection), so the mixing launch does not take the vertical advection in."""
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.pelagicegg import PelagicEggDrift
    assert PelagicEggDrift.update is not OceanDrift.update
    assert PelagicEggDrift.update_terminal_velocity is not OceanDrift.update_terminal_velocity
    assert not PelagicEggDrift._fuses_vertical_advection()
    assert PelagicEggDrift.vertical_mixing is OceanDrift.vertical_mixing and PelagicEggDrift.advect_ocean_current is OceanDrift.advect_ocean_current
    assert getattr(PelagicEggDrift, 'leeway_lane_update', None) is None
    assert PelagicEggDrift(loglevel=50)._run_lane() == 'call_by_call'


def test_abi_entry_is_declared_and_bound():
    from opendrift_amd import _abi, device
    src = open(os.path.join(ROOT, 'include', 'odrift.h')).read()
    assert re.search(r'\bint odr_egg_terminal_velocity\(odr_ctx \*ctx, odr_particles \*p, int diameter_slot, int salinity_slot\);', src)
    assert 'odr_egg_terminal_velocity' in _abi._SIGNATURES and 'odr_egg_terminal_velocity' in _abi.EXPORTS
    assert len(_abi._SIGNATURES['odr_egg_terminal_velocity']) == 4
    assert callable(device.Particles.egg_terminal_velocity)
    assert _abi.EGG_PROPERTIES == ['diameter', 'neutral_buoyancy_salinity', 'density', 'hatched']
