"""CPU: the host side of LarvalFish (opendrift_amd/larvalfish.py) -- what can be checked without a device: the class, its
configuration, its element properties, the order of update() and the C ABI entries of its kernels."""
import os
import re
from datetime import datetime, timedelta

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = datetime(2020, 1, 1)
REQUIRED = {   # opendrift/models/larvalfish.py:69-84
    'x_sea_water_velocity': 0, 'y_sea_water_velocity': 0, 'sea_surface_height': 0, 'sea_surface_wave_significant_height': 0,
    'x_wind': 0, 'y_wind': 0, 'land_binary_mask': None, 'sea_floor_depth_below_sea_level': 100,
    'ocean_vertical_diffusivity': 0.01, 'ocean_mixed_layer_thickness': 50, 'sea_water_temperature': 10, 'sea_water_salinity': 34,
    'sea_surface_wave_stokes_drift_x_velocity': 0, 'sea_surface_wave_stokes_drift_y_velocity': 0}
DEFAULTS = {'diameter': 0.0014, 'neutral_buoyancy_salinity': 31.25, 'stage_fraction': 0., 'hatched': 0., 'length': 0., 'weight': 0.08,
            'survival': 1.}   # :31-52
ORDER = ['diameter', 'neutral_buoyancy_salinity', 'stage_fraction', 'hatched', 'length', 'weight', 'survival']


def model(**kw):
    from opendrift_amd.larvalfish import LarvalFish
    return LarvalFish(loglevel=50, **kw)


def test_class_and_config_defaults():
    from opendrift_amd.oceandrift import OceanDrift
    o = model()
    assert isinstance(o, OceanDrift)
    assert o.get_config('IBM:fraction_of_timestep_swimming') == 0.15
    assert o.get_config('drift:vertical_mixing') is True
    assert o.get_config('drift:vertical_mixing_at_surface') is True
    assert o.get_config('drift:vertical_advection_at_surface') is True
    assert o.get_config('general:coastline_action') == 'stranding'          # (not changed by the reference's class, :101-103)
    o.set_config('IBM:fraction_of_timestep_swimming', 1.0)
    with pytest.raises(ValueError):
        o.set_config('IBM:fraction_of_timestep_swimming', 1.5)
    assert OceanDrift(loglevel=50).get_config('drift:vertical_mixing') is False      # (the base class keeps its own)


def test_required_variables_and_their_fallbacks():
    from opendrift_amd import _abi
    from opendrift_amd.larvalfish import LarvalFish
    assert {k: v['fallback'] for k, v in LarvalFish.required_variables.items()} == REQUIRED
    for k in ('ocean_vertical_diffusivity', 'sea_water_temperature', 'sea_water_salinity'):
        assert LarvalFish.required_variables[k].get('profiles') is True
    o = model()
    for v, fb in REQUIRED.items():
        assert o.get_config('environment:fallback:%s' % v) == fb
        assert o.get_config('environment:constant:%s' % v) is None
    assert set(o.required_variables) == set(REQUIRED) and set(REQUIRED) <= set(_abi.VARIABLES)     # every one has a device id


def test_element_properties_are_float32_with_the_reference_defaults():
    o = model()
    for k, v in DEFAULTS.items():
        assert o.get_config('seed:%s' % k) == v
    assert o.aux_properties == ORDER and len(ORDER) <= 9
    o.seed_elements(lon=4.0, lat=60.0, number=5, time=T0)
    for k, v in DEFAULTS.items():
        assert o._sched[k].dtype == np.float32 and o._sched[k].shape == (5,) and (o._sched[k] == np.float32(v)).all()
    w = np.linspace(0.1, 20, 3)
    o.seed_elements(lon=[4.0, 4.1, 4.2], lat=[60.0, 60.0, 60.0], time=T0, weight=w, hatched=np.uint8([1, 0, 1]), stage_fraction=0.5)
    assert o._sched['weight'].dtype == np.float32 and np.array_equal(o._sched['weight'][5:], w.astype(np.float32))
    assert o._sched['hatched'].dtype == np.float32 and np.array_equal(o._sched['hatched'], [0, 0, 0, 0, 0, 1, 0, 1])
    assert (o._sched['stage_fraction'][5:] == 0.5).all() and (o._sched['stage_fraction'][:5] == 0).all()
    assert len(o._sched['survival']) == 8
    for k in ORDER:
        with pytest.raises(ValueError, match=k):
            o.seed_elements(lon=[4.0, 4.1, 4.2], lat=[60.0, 60.0, 60.0], time=T0, **{k: [0.5, 0.6]})
    o2 = model()
    o2.set_config('seed:weight', 2.0)
    o2.seed_elements(lon=4.0, lat=60.0, number=2, time=T0)
    assert (o2._sched['weight'] == np.float32(2.0)).all()


def test_tsprofiles_is_refused_by_name():
    o = model()
    with pytest.raises(NotImplementedError, match='TSprofiles'):
        o.set_config('vertical_mixing:TSprofiles', True)
    o.set_config('vertical_mixing:TSprofiles', False)
    with pytest.raises(NotImplementedError, match='profiles'):
        o.update_terminal_velocity(Tprofiles=np.zeros((3, 2)), Sprofiles=np.zeros((3, 2)))


class StubParticles:
    """Records the calls update() makes on the particles object"""

    def __init__(self, n):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append((name, a, kw))
        return call


def _stubbed(n, hour, monkeypatch):
    from opendrift_amd.oceandrift import OceanDrift
    o = model()
    o.set_config('IBM:fraction_of_timestep_swimming', 0.4)
    o.P = StubParticles(n)
    o.time, o.time_step = T0 + timedelta(hours=hour), timedelta(seconds=600)
    monkeypatch.setattr(type(o), 'num_elements_active', lambda self: len(self.P))
    for name in ('advect_ocean_current', 'stokes_drift', 'vertical_mixing', 'advect_wind', 'vertical_advection', 'vertical_buoyancy'):
        monkeypatch.setattr(OceanDrift, name, lambda self, *a, _n=name, **kw: self.P.calls.append((_n, a, kw)))
    monkeypatch.setattr(type(o), 'vertical_advection', lambda self, *a, **kw: self.P.calls.append(('vertical_advection', a, kw)))
    return o


@pytest.mark.parametrize('hour,direction', [(0, -1), (11.99, -1), (12, 1), (23.5, 1)])
def test_update_calls_in_the_order_of_the_reference(monkeypatch, hour, direction):
    """larvalfish.py:255-265: update_fish_larvae, advect_ocean_current, stokes_drift, update_terminal_velocity, vertical_mixing,
    larvae_vertical_migration -- no wind drift, no vertical advection; one device call each for the model's own three."""
    o = _stubbed(7, hour, monkeypatch)
    o.update()
    assert [c[0] for c in o.P.calls] == ['larval_update', 'advect_ocean_current', 'stokes_drift', 'egg_terminal_velocity',
                                        'vertical_mixing', 'larval_migrate']
    assert o.P.calls[0][1] == (600.0, 2, 3, 5, 4)            # dt, stage_fraction, hatched, weight, length
    assert o.P.calls[3][1] == (0, 1)                         # diameter, neutral_buoyancy_salinity
    assert o.P.calls[5][1] == (600.0, 0.4, direction, 3, 4)  # dt, fraction, direction, hatched, length


def test_no_model_launch_without_active_elements(monkeypatch):
    o = _stubbed(0, 3, monkeypatch)
    o.update()
    assert [c[0] for c in o.P.calls] == ['advect_ocean_current', 'stokes_drift', 'vertical_mixing']


def test_run_takes_the_call_by_call_lane():
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.larvalfish import LarvalFish
    assert LarvalFish.update is not OceanDrift.update
    assert LarvalFish.update_terminal_velocity is not OceanDrift.update_terminal_velocity
    assert not LarvalFish._fuses_vertical_advection()      # (the mixing launch must not take it in)
    assert LarvalFish.vertical_mixing is OceanDrift.vertical_mixing and LarvalFish.stokes_drift is OceanDrift.stokes_drift
    assert LarvalFish.advect_ocean_current is OceanDrift.advect_ocean_current
    assert getattr(LarvalFish, 'leeway_lane_update', None) is None
    assert LarvalFish(loglevel=50)._run_lane() == 'call_by_call'


def test_abi_entries_are_declared_and_bound():
    from opendrift_amd import _abi, device
    src = open(os.path.join(ROOT, 'include', 'odrift.h')).read()
    assert re.search(r'\bint odr_larval_update\(odr_ctx \*ctx, odr_particles \*p, int stage_fraction_slot, int hatched_slot, '
                     r'int weight_slot, int length_slot,\s+double dt_seconds\);', src)
    assert re.search(r'\bint odr_larval_migrate\(odr_ctx \*ctx, odr_particles \*p, int hatched_slot, int length_slot, '
                     r'double fraction_swimming,\s+double dt_seconds, int direction\);', src)
    m = re.search(r'enum \{ (ODR_LARVA_[^}]*)\};', src)
    names = [x.split('=')[0].strip() for x in m.group(1).split(',')]
    values = [int(x.split('=')[1]) for x in m.group(1).split(',')]
    assert names == ['ODR_LARVA_DIAMETER', 'ODR_LARVA_NEUTRAL_BUOYANCY_SALINITY', 'ODR_LARVA_STAGE_FRACTION', 'ODR_LARVA_HATCHED',
                     'ODR_LARVA_LENGTH', 'ODR_LARVA_WEIGHT', 'ODR_LARVA_SURVIVAL'] and values == list(range(7))
    for name, nargs in (('odr_larval_update', 7), ('odr_larval_migrate', 7)):
        assert name in _abi.EXPORTS and len(_abi._SIGNATURES[name]) == nargs
    assert callable(device.Particles.larval_update) and callable(device.Particles.larval_migrate)
    assert _abi.LARVA_PROPERTIES == ORDER
    for cite in ('larvalfish.py:200-231', 'larvalfish.py:233-253'):
        assert cite in src
