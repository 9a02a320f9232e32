"""CPU: the host side of LarvalFishExtended (opendrift_amd/larvalfish_extended.py) -- what can be checked without a device: the
class and its export, its configuration, its element properties, the order of update(), what it hands to its launches, the time
scalars of the solar elevation and the C ABI entries of its kernels."""
import os
import re
from datetime import datetime, timedelta

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = datetime(2020, 1, 1)
REQUIRED = {   # opendrift/models/larvalfish_extended.py:73-88
    'x_sea_water_velocity': 0, 'y_sea_water_velocity': 0, 'sea_surface_height': 0, 'sea_surface_wave_significant_height': 0,
    'x_wind': 0, 'y_wind': 0, 'land_binary_mask': None, 'sea_floor_depth_below_sea_level': 100,
    'ocean_vertical_diffusivity': 0.01, 'ocean_mixed_layer_thickness': 50, 'sea_water_temperature': 10, 'sea_water_salinity': 34,
    'sea_surface_wave_stokes_drift_x_velocity': 0, 'sea_surface_wave_stokes_drift_y_velocity': 0}
FLOATS = {   # :112-166: key: (default, min, max)
    'biology:w_active': (0.003, 0.0, 1.0), 'biology:z_pref': (-10.0, -10000, 0.0), 'biology:z_day': (-25.0, -10000, 0.0),
    'biology:z_night': (-5.0, -10000, 0.0), 'biology:dz_min': (1.0, 0.1, 100), 'biology:dz_rel': (0.1, 0.0, 1.0),
    'biology:dz_max': (15.0, 0.1, 1000), 'egg:hatch_time_days': (2.0, 0.004, 416)}
ENUMS = {'biology:particle_type': ('larva', ['larva', 'phytoplankton']), 'biology:vertical_behavior_mode': ('dvm', ['none', 'depth', 'dvm']),
         'egg:hatching_method': ('fixed_time', ['fixed_time'])}


def model(**kw):
    from opendrift_amd.larvalfish_extended import LarvalFishExtended
    return LarvalFishExtended(loglevel=50, **kw)


def test_package_export():
    import opendrift_amd
    from opendrift_amd.larvalfish_extended import LarvalFishExtended
    from opendrift_amd.oceandrift import OceanDrift
    assert opendrift_amd.LarvalFishExtended is LarvalFishExtended and issubclass(LarvalFishExtended, OceanDrift)
    with pytest.raises(AttributeError):
        opendrift_amd.NoSuchModel


def test_config_keys_defaults_ranges_and_enums():
    from opendrift_amd.oceandrift import OceanDrift
    o = model()
    assert len(FLOATS) + len(ENUMS) == 11
    for k, (default, lo, hi) in FLOATS.items():
        assert o.get_config(k) == default and o._config[k]['type'] == 'float', k
        o.set_config(k, lo)
        o.set_config(k, hi)
        for bad in (lo - 1e-3, hi + 1e-3):
            with pytest.raises(ValueError):
                o.set_config(k, bad)
    for k, (default, enum) in ENUMS.items():
        assert o.get_config(k) == default and o._config[k]['enum'] == enum, k
        for v in enum:
            o.set_config(k, v)
        with pytest.raises(ValueError):
            o.set_config(k, 'temperature')
    assert o.get_config('drift:vertical_mixing') is True
    assert o.get_config('drift:vertical_mixing_at_surface') is True
    assert o.get_config('drift:vertical_advection_at_surface') is True
    assert OceanDrift(loglevel=50).get_config('drift:vertical_mixing') is False      # (the base class keeps its own)


def test_required_variables_and_their_fallbacks():
    from opendrift_amd import _abi
    from opendrift_amd.larvalfish_extended import LarvalFishExtended
    assert {k: v['fallback'] for k, v in LarvalFishExtended.required_variables.items()} == REQUIRED
    for k in ('ocean_vertical_diffusivity', 'sea_water_temperature', 'sea_water_salinity'):
        assert LarvalFishExtended.required_variables[k].get('profiles') is True
    o = model()
    for v, fb in REQUIRED.items():
        assert o.get_config('environment:fallback:%s' % v) == fb
    assert set(o.required_variables) == set(REQUIRED) and set(REQUIRED) <= set(_abi.VARIABLES)     # every one has a device id


def test_element_properties_are_float32_seeded_as_scalars_or_arrays():
    o = model()
    assert o.aux_properties == ['stage_fraction', 'hatched']
    assert o.get_config('seed:stage_fraction') == 0.0 and o.get_config('seed:hatched') == 0.0
    o.seed_elements(lon=4.0, lat=60.0, number=5, time=T0)
    for k in o.aux_properties:
        assert o._sched[k].dtype == np.float32 and o._sched[k].shape == (5,) and (o._sched[k] == 0).all()
    s = np.linspace(0.1, 0.9, 3)
    o.seed_elements(lon=[4.0, 4.1, 4.2], lat=[60.0, 60.0, 60.0], time=T0, stage_fraction=s, hatched=np.uint8([1, 0, 1]))
    assert o._sched['stage_fraction'].dtype == np.float32 and np.array_equal(o._sched['stage_fraction'][5:], s.astype(np.float32))
    assert o._sched['hatched'].dtype == np.float32 and np.array_equal(o._sched['hatched'], [0, 0, 0, 0, 0, 1, 0, 1])
    o.seed_elements(lon=[4.0, 4.1], lat=[60.0, 60.0], time=T0, stage_fraction=0.5)
    assert (o._sched['stage_fraction'][8:] == 0.5).all() and len(o._sched['hatched']) == 10
    for k in o.aux_properties:
        with pytest.raises(ValueError, match=k):
            o.seed_elements(lon=[4.0, 4.1, 4.2], lat=[60.0, 60.0, 60.0], time=T0, **{k: [0.5, 0.6]})
    o2 = model()
    o2.set_config('seed:stage_fraction', 0.25)
    o2.seed_elements(lon=4.0, lat=60.0, number=2, time=T0)
    assert (o2._sched['stage_fraction'] == np.float32(0.25)).all()


def test_tsprofiles_refusal_is_inherited():
    from opendrift_amd.larvalfish_extended import LarvalFishExtended
    from opendrift_amd.oceandrift import OceanDrift
    assert 'set_config' not in vars(LarvalFishExtended)
    o = model()
    with pytest.raises(NotImplementedError, match='TSprofiles'):
        o.set_config('vertical_mixing:TSprofiles', True)
    o.set_config('vertical_mixing:TSprofiles', False)
    assert LarvalFishExtended.set_config is OceanDrift.set_config or LarvalFishExtended.set_config.__qualname__.split('.')[0] != 'LarvalFishExtended'


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


def _stubbed(n, monkeypatch, **config):
    from opendrift_amd.oceandrift import OceanDrift
    o = model()
    for k, v in config.items():
        o.set_config(k.replace('__', ':'), v)
    o.P = StubParticles(n)
    o.time, o.time_step = T0 + timedelta(days=9, hours=11, minutes=30), timedelta(seconds=1800)
    monkeypatch.setattr(type(o), 'num_elements_active', lambda self: len(self.P))
    for name in ('advect_ocean_current', 'stokes_drift', 'vertical_mixing', 'advect_wind', 'vertical_buoyancy'):
        monkeypatch.setattr(OceanDrift, name, lambda self, *a, _n=name, **kw: self.P.calls.append((_n, a, kw)))
    monkeypatch.setattr(type(o), 'vertical_advection', lambda self, *a, **kw: self.P.calls.append(('vertical_advection', a, kw)))
    return o


def test_update_calls_in_the_order_of_the_reference(monkeypatch):
    """larvalfish_extended.py:324-342: update_fish_larvae (larva only), advect_ocean_current, stokes_drift, vertical_mixing,
    _apply_vertical_behavior -- no wind drift, no vertical advection, no terminal velocity; one device call each for the model's own."""
    from opendrift_amd.oceandrift import solar_time_scalars
    o = _stubbed(7, monkeypatch, egg__hatch_time_days=1.3)
    o.update()
    assert [c[0] for c in o.P.calls] == ['larvalx_hatch', 'advect_ocean_current', 'stokes_drift', 'vertical_mixing', 'larvalx_behave']
    assert o.P.calls[0][1] == ((1800.0 / 86400) / 1.3, 0, 1)             # increment in float64, stage_fraction, hatched
    name, a, kw = o.P.calls[4]
    assert a == ('dvm', 1800.0, 0.003, (-5.0, 1.0), (-25.0, 2.5), solar_time_scalars(o.time))      # night band (dz_min), day band (dz_rel)
    assert kw == dict(active_only_hatched=True, z_is_float32=False, hatched_slot=1)


def test_phytoplankton_depth_mode_and_the_float32_z_of_a_run_without_mixing(monkeypatch):
    o = _stubbed(7, monkeypatch, biology__particle_type='phytoplankton', biology__vertical_behavior_mode='depth', biology__z_pref=-200.0,
                 drift__vertical_mixing=False, biology__w_active=0.02)
    o.update()
    assert [c[0] for c in o.P.calls] == ['advect_ocean_current', 'stokes_drift', 'vertical_mixing', 'larvalx_behave']      # no hatching
    name, a, kw = o.P.calls[3]
    assert a == ('depth', 1800.0, 0.02, (-200.0, 15.0))                  # dz_max sets the half-width
    assert kw == dict(active_only_hatched=False, z_is_float32=True, hatched_slot=1)


@pytest.mark.parametrize('config', [dict(biology__vertical_behavior_mode='none'), dict(biology__w_active=0.0)])
def test_no_behaviour_launch(monkeypatch, config):
    o = _stubbed(7, monkeypatch, **config)
    o.update()
    assert [c[0] for c in o.P.calls] == ['larvalx_hatch', 'advect_ocean_current', 'stokes_drift', 'vertical_mixing']


def test_no_model_launch_without_active_elements(monkeypatch):
    o = _stubbed(0, monkeypatch)
    o.update()
    assert [c[0] for c in o.P.calls] == ['advect_ocean_current', 'stokes_drift', 'vertical_mixing']


def test_run_takes_the_call_by_call_lane():
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.larvalfish_extended import LarvalFishExtended
    assert LarvalFishExtended.update is not OceanDrift.update
    assert not LarvalFishExtended._fuses_vertical_advection()      # (the mixing launch must not take it in)
    assert LarvalFishExtended.vertical_mixing is OceanDrift.vertical_mixing and LarvalFishExtended.stokes_drift is OceanDrift.stokes_drift
    assert LarvalFishExtended.advect_ocean_current is OceanDrift.advect_ocean_current
    assert getattr(LarvalFishExtended, 'leeway_lane_update', None) is None
    assert LarvalFishExtended(loglevel=50)._run_lane() == 'call_by_call'


def test_solar_elevation_is_a_method_of_the_base_model_and_its_time_scalars():
    from opendrift_amd.oceandrift import OceanDrift, solar_time_scalars
    from opendrift_amd import device
    assert callable(OceanDrift.solar_elevation) and callable(device.Particles.solar_elevation)
    d, eq, minutes = solar_time_scalars(datetime(2020, 1, 10, 11, 30, 30))
    assert all(type(v) is float for v in (d, eq, minutes)) and minutes == 11 * 60 + 30.5
    assert -23.0 < np.degrees(d) < -21.5 and -8.5 < eq < -6.5              # 10 January: the sun 22 deg south (22.6 by this formula), 7 - 8 minutes slow
    assert solar_time_scalars(datetime(2020, 1, 10, 11, 59))[1] == eq       # the equation of time takes the integer hour ...
    assert solar_time_scalars(datetime(2020, 1, 10, 12, 0))[1] != eq
    assert solar_time_scalars(datetime(2020, 1, 10, 23, 0))[0] == d         # ... and the declination the day of the year
    assert 23.4 < np.degrees(solar_time_scalars(datetime(2020, 6, 21))[0]) < 24.2


def test_abi_entries_are_declared_and_bound():
    from opendrift_amd import _abi, device
    src = open(os.path.join(ROOT, 'include', 'odrift.h')).read()
    assert re.search(r'\bint odr_solar_elevation\(odr_ctx \*ctx, odr_particles \*p, double declination_rad, double time_offset_minutes, '
                     r'double day_minutes,\s+double \*out_host\);', src)
    assert re.search(r'\bint odr_larvalx_hatch\(odr_ctx \*ctx, odr_particles \*p, int stage_fraction_slot, int hatched_slot, double increment\);', src)
    assert re.search(r'\bint odr_larvalx_behave\(odr_ctx \*ctx, odr_particles \*p, int hatched_slot, int mode, int active_only_hatched, int z_is_float32,', src)
    assert re.search(r'enum \{ ODR_LARVALX_STAGE_FRACTION = 0, ODR_LARVALX_HATCHED = 1 \};', src)
    assert re.search(r'enum \{ ODR_LARVALX_DEPTH = 1, ODR_LARVALX_DVM = 2 \};', src)
    for name, nargs in (('odr_solar_elevation', 6), ('odr_larvalx_hatch', 5), ('odr_larvalx_behave', 15)):
        assert name in _abi.EXPORTS and len(_abi._SIGNATURES[name]) == nargs
    assert callable(device.Particles.larvalx_hatch) and callable(device.Particles.larvalx_behave)
    assert _abi.LARVALX_PROPERTIES == ['stage_fraction', 'hatched'] and _abi.LARVALX_MODES == {'depth': 1, 'dvm': 2}
    assert _abi.NVAR == 26
    for cite in ('larvalfish_extended.py:292-318', 'larvalfish_extended.py:206-290', 'physics_methods.py:977-979'):
        assert cite in src
    from opendrift_amd import build
    assert 'odr_larvalx.hip' in build.UNITS
