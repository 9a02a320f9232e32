"""CPU: the host side of PlastDrift (opendrift_amd/plastdrift.py) and of drift:use_tabularised_stokes_drift on OceanDrift -- the
class and its element default, required variables, fallbacks and config defaults against the reference's (plastdrift.py:23-78,
oceandrift.py:160-165), the lane, the dispatch of update_particle_depth, where the coefficients are looked for and what is said
without them, the decisions of environment.py:844-863, and every refusal by name.  Nothing here touches the device."""
import json
import os
from datetime import datetime

import numpy as np
import pytest

import opendrift_amd
from opendrift_amd import _abi
from opendrift_amd import stokes_tables as st
from opendrift_amd.oceandrift import OceanDrift, OpenDriftSimulation
from opendrift_amd.openoil import OpenOil
from opendrift_amd.plastdrift import PlastDrift

T0 = datetime(2020, 1, 1)
TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stokes_tables.json')
SX, SY = 'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity'
HS = 'sea_surface_wave_significant_height'


@pytest.fixture(autouse=True)
def no_tables_from_the_environment(monkeypatch):
    monkeypatch.delenv(st.ENV, raising=False)
    monkeypatch.setattr(st, 'from_installed_reference', lambda: None)      # (whatever is installed where the tests run)


def test_exported_from_the_package_and_in_the_abi():
    assert opendrift_amd.PlastDrift is PlastDrift and issubclass(PlastDrift, OceanDrift)
    assert {'odr_stokes_from_wind', 'odr_plast_depth', 'odr_reduce_wave_maxima'} <= set(_abi.EXPORTS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'odrift.h')).read()
    assert 'ODR_PLAST_STOKES = %d, ODR_PLAST_HS = %d' % (_abi.PLAST_STOKES, _abi.PLAST_HS) in header


def test_element_default_required_variables_and_fallbacks():
    o = PlastDrift(loglevel=50)
    assert PlastDrift.element_properties['terminal_velocity'] == 0.01      # plastdrift.py:23-29
    o.seed_elements(lon=[4.0, 4.1], lat=[60.0, 60.0], time=T0)
    assert o._sched['terminal_velocity'].dtype == np.float32 and (o._sched['terminal_velocity'] == np.float32(0.01)).all()
    want = {'x_sea_water_velocity': 0, 'y_sea_water_velocity': 0, 'sea_surface_height': 0, SX: 0, SY: 0, HS: 0, 'x_wind': 0, 'y_wind': 0,
            'ocean_vertical_diffusivity': 0.02, 'ocean_mixed_layer_thickness': 50, 'sea_floor_depth_below_sea_level': 10000,
            'land_binary_mask': None}      # :44-57
    rv = PlastDrift.required_variables
    assert len(rv) == 12 and {k: v['fallback'] for k, v in rv.items()} == want and set(o.required_variables) == set(want)
    assert rv['ocean_vertical_diffusivity'].get('profiles') is True
    assert [k for k, v in rv.items() if v.get('profiles')] == ['ocean_vertical_diffusivity']
    for k, v in want.items():
        assert o.get_config('environment:fallback:' + k) == v


def test_config_defaults_are_the_reference_s():
    o = PlastDrift(loglevel=50)
    assert o.get_config('vertical_mixing:mixingmodel') == 'analytical'      # :66-72
    for v in ('randomwalk', 'analytical'):
        o.set_config('vertical_mixing:mixingmodel', v)
    with pytest.raises(ValueError):
        o.set_config('vertical_mixing:mixingmodel', 'implicit')
    o = PlastDrift(loglevel=50)
    assert o.get_config('drift:vertical_mixing') is True and o.get_config('drift:vertical_advection') is True      # :74-78
    assert o.get_config('drift:use_tabularised_stokes_drift') is True and o.get_config('drift:tabularised_stokes_drift_fetch') == '25000'
    assert o.get_config('general:coastline_action') == 'previous'
    assert o.get_config('vertical_mixing:diffusivitymodel') == 'windspeed_Sundby1983'


def test_oceandrift_has_the_two_keys_off_and_its_subclasses_inherit_them():
    for cls in (OceanDrift, OpenOil):
        o = cls(loglevel=50)
        assert o.get_config('drift:use_tabularised_stokes_drift') is False      # oceandrift.py:160-165
        assert o.get_config('drift:tabularised_stokes_drift_fetch') == '25000'
        for f in ('5000', '25000', '50000'):
            o.set_config('drift:tabularised_stokes_drift_fetch', f)
        with pytest.raises(ValueError):
            o.set_config('drift:tabularised_stokes_drift_fetch', '10000')
        with pytest.raises(ValueError):
            o.set_config('drift:tabularised_stokes_drift_fetch', 25000)
        assert not o._waves_from_wind()
        if cls is OceanDrift:
            o.prepare_run()      # the option off: no tables are asked for


def test_lane_is_call_by_call_with_the_option_and_answered_without_a_device(monkeypatch):
    monkeypatch.setattr(OpenDriftSimulation, 'ctx', property(lambda self: pytest.fail('_run_lane() needs no device')))
    assert PlastDrift(loglevel=50)._run_lane() == 'call_by_call'
    o = OceanDrift(loglevel=50)
    assert o._run_lane() == 'fused'
    o.set_config('drift:use_tabularised_stokes_drift', True)
    assert o._run_lane() == 'call_by_call'
    o.set_config('drift:use_tabularised_stokes_drift', False)
    assert o._run_lane() == 'fused'


class StubParticles:
    def __init__(self, maxima=(0.0, 0.0, 0.0)):
        self.calls, self.maxima = [], maxima

    def plast_depth(self, **kw):
        self.calls.append(('plast_depth', kw))

    def wave_maxima(self):
        self.calls.append(('wave_maxima', ))
        return self.maxima

    def stokes_from_wind(self, stokes, hs):
        self.calls.append(('stokes_from_wind', None if stokes is None else len(stokes), None if hs is None else len(hs)))


def stub_model(monkeypatch, cls=PlastDrift, n=5, **kw):
    o = cls(loglevel=50, stokes_tables=TABLES, **kw)
    o.P = StubParticles()
    o.steps_calculation = 7
    monkeypatch.setattr(type(o), 'num_elements_active', lambda self: n)
    for name in ('advect_ocean_current', 'stokes_drift', 'vertical_mixing', 'advect_wind', 'vertical_advection'):
        monkeypatch.setattr(OceanDrift, name, lambda self, *a, _n=name, **k: self.P.calls.append((_n, )))
    return o


def test_update_order_and_dispatch_of_the_mixing_model(monkeypatch):
    o = stub_model(monkeypatch)
    o.update()      # plastdrift.py:80-92; drift:vertical_advection is True and vertical_advection() is never called
    assert o.P.calls == [('advect_ocean_current', ), ('plast_depth', {'step': 7}), ('stokes_drift', ), ('advect_wind', )]
    o.P.calls.clear()
    o.set_config('vertical_mixing:mixingmodel', 'randomwalk')
    o.update()
    assert o.P.calls == [('advect_ocean_current', ), ('vertical_mixing', ), ('stokes_drift', ), ('advect_wind', )]
    assert PlastDrift.fuse_vertical_advection is False      # the random walk's launch does not take the vertical advection along
    o.P.calls.clear()
    o.set_config('drift:vertical_mixing', False)
    o.update_particle_depth()
    assert o.P.calls == []


def test_numpy_rng_draws_standard_exponentials_as_the_reference_consumes_the_stream(monkeypatch):
    o = stub_model(monkeypatch, rng='numpy', n=6)
    np.random.seed(3)
    o.update_particle_depth()
    (name, kw), = o.P.calls
    np.random.seed(3)
    scale = np.linspace(0.5, 3, 6)
    assert name == 'plast_depth' and np.array_equal(scale * kw['draws'], np.random.exponential(scale, 6))
    np.random.seed(3)
    np.random.exponential(scale, 6)
    after_reference = np.random.random()
    np.random.seed(3)
    o.update_particle_depth()
    assert np.random.random() == after_reference


def test_tables_are_looked_for_in_order_and_prepare_run_says_what_is_missing(monkeypatch, tmp_path):
    with pytest.raises(FileNotFoundError, match='stokes_tables=.*ODR_STOKES_TABLES.*install opendrift'):
        PlastDrift(loglevel=50).prepare_run()
    o = OceanDrift(loglevel=50)
    o.prepare_run()      # the option off: nothing is needed
    o.set_config('drift:use_tabularised_stokes_drift', True)
    with pytest.raises(FileNotFoundError, match='not shipped'):
        o.prepare_run()
    gold = json.load(open(TABLES))
    # 3. an installed opendrift
    monkeypatch.setattr(st, 'from_installed_reference', lambda: st.load({'25000': {'stokes': [3.0], 'hs': [0.0, 3.0]}}))
    o = PlastDrift(loglevel=50)
    o.prepare_run()
    assert o._stokes_tables['25000']['stokes'][0] == 3.0
    # 2. the environment variable comes before it (an .npz here)
    npz = tmp_path / 't.npz'
    np.savez(npz, stokes_25000=[2.0, 1.0], hs_25000=[0.0, 2.0])
    monkeypatch.setenv(st.ENV, str(npz))
    o = PlastDrift(loglevel=50)
    o.prepare_run()
    assert list(o._stokes_tables['25000']['stokes']) == [2.0, 1.0] and o._stokes_tables['25000']['hs'].dtype == np.float64
    # 1. the argument comes first: constructor, then set_stokes_tables
    o = PlastDrift(loglevel=50, stokes_tables=TABLES)
    o.prepare_run()
    assert np.array_equal(o._stokes_tables['25000']['stokes'], gold['25000']['stokes']) and len(o._stokes_tables['5000']['stokes']) == 4
    assert o.clone()._stokes_tables_argument == TABLES
    o = PlastDrift(loglevel=50)
    o.set_stokes_tables({'25000': {'stokes': [1.0], 'hs': [0.0, 1.0]}})
    o.prepare_run()
    assert o._stokes_tables['25000']['stokes'][0] == 1.0
    o.set_config('drift:tabularised_stokes_drift_fetch', '5000')
    with pytest.raises(KeyError, match='5000'):
        o.prepare_run()
    with pytest.raises(FileNotFoundError):
        PlastDrift(loglevel=50, stokes_tables=str(tmp_path / 'absent.json')).prepare_run()
    for bad in ({}, {'25000': {'stokes': [1.0] * 8, 'hs': [0.0, 1.0]}}, {'25000': {'stokes': [1.0]}}, {'25000': {'stokes': [np.nan], 'hs': [0., 1.]}}):
        with pytest.raises(ValueError):
            st.load(bad)


def test_the_tables_and_the_fit_are_not_in_the_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in ('opendrift_amd/stokes_tables.py', 'opendrift_amd/plastdrift.py', 'opendrift_amd/csrc/odr_plast.hip.h',
                 'opendrift_amd/csrc/odr_plast.hip'):
        src = open(os.path.join(root, path)).read()
        assert 'polyfit(' not in src and '0.0173' not in src and '0.030' not in src, path


NAMES = list(PlastDrift.required_variables)


@pytest.mark.parametrize('readers,maxima,want', [
    ({}, None, ('stokes_from_wind', 7, 2)),                                # nothing delivers waves: both, without looking
    ({SX: 1, SY: 1, HS: 1}, (0.2, 0.02, 0.0), ('stokes_from_wind', None, 2)),      # Stokes drift from a reader, wave height 0
    ({SX: 1, SY: 1, HS: 1}, (0.0, 0.0, 1.5), ('stokes_from_wind', 7, None)),       # Stokes drift 0 everywhere
    ({SX: 1, SY: 1, HS: 1}, (-0.1, 0.0, 0.0), ('stokes_from_wind', None, 2)),      # x all negative, y zero: plain maxima, not both 0
    ({HS: 1}, (0.0, 0.0, 2.0), ('stokes_from_wind', 7, None)),                   # only a wave height
    ({SX: 1, SY: 1, HS: 1}, (0.2, 0.0, 1.0), None),                               # everything delivered: nothing replaced
])
def test_decisions_of_get_environment(monkeypatch, readers, maxima, want):
    o = stub_model(monkeypatch)
    o.prepare_run()
    o.P.maxima = maxima
    o.readers = {'r': object()}
    for v in readers:
        o.priority_list[v] = ['r']
    o._parameterise_waves(NAMES)
    looked = ('wave_maxima', ) in o.P.calls
    assert looked == (maxima is not None)
    assert [c for c in o.P.calls if c[0] == 'stokes_from_wind'] == ([want] if want else [])


def test_hook_does_nothing_when_off_or_without_wind(monkeypatch):
    o = stub_model(monkeypatch, cls=OceanDrift)
    o._parameterise_waves(list(o.required_variables))
    assert o.P.calls == []
    o = stub_model(monkeypatch)
    o._parameterise_waves([v for v in NAMES if v != 'x_wind'])      # a stage call: the current only
    assert o.P.calls == []
    o.set_config('drift:tabularised_stokes_drift_fetch', '5000')
    o.prepare_run()
    o._parameterise_waves(NAMES)
    assert o.P.calls == [('stokes_from_wind', 4, 2)]
    assert not o._identically_zero(SX) and not o._identically_zero(HS)      # the movers must look: the values come from the wind
    assert OceanDrift(loglevel=50)._identically_zero(SX)


def test_refused_sharded_run(monkeypatch):
    from opendrift_amd import distributed as D
    monkeypatch.setattr(D, 'env_world', lambda: (0, 0, 2))
    with pytest.raises(NotImplementedError, match='sharded'):
        PlastDrift(loglevel=50)
    monkeypatch.setattr(D, 'init', lambda: None)
    monkeypatch.setattr(D, 'backend', lambda: 'gloo')
    o = OceanDrift(loglevel=50, device=1)
    o.set_config('drift:use_tabularised_stokes_drift', True)
    o.seed_elements(lon=[4.0], lat=[60.0], time=T0)
    with pytest.raises(NotImplementedError, match='use_tabularised_stokes_drift in a sharded run'):
        o.run(steps=1, time_step=600)


def test_negative_scale_is_a_value_error_through_the_model(monkeypatch):
    """odr_plast_depth answers a negative scale with ODR_ERR_INVALID; the binding turns that into ValueError with the library's
    message, and it leaves update_particle_depth() and update() as np.random.exponential's leaves the reference's: the movers
    behind it do not run."""
    class Lib:
        @staticmethod
        def odr_last_error():
            return b'scale < 0: ocean_vertical_diffusivity / terminal_velocity is negative for an active element'

    monkeypatch.setattr(_abi, 'load', lambda: Lib)
    for rng in ('device', 'numpy'):
        o = stub_model(monkeypatch, rng=rng)

        def plast_depth(**kw):
            o.P.calls.append(('plast_depth', sorted(kw)))
            _abi.check(-1)      # what Particles.plast_depth does with the library's return value (include/odrift.h ODR_ERR_INVALID)
        o.P.plast_depth = plast_depth
        with pytest.raises(ValueError, match='scale < 0'):
            o.update_particle_depth()
        o.P.calls.clear()
        with pytest.raises(ValueError, match='scale < 0'):
            o.update()
        assert o.P.calls == [('advect_ocean_current', ), ('plast_depth', ['draws'] if rng == 'numpy' else ['step'])]
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'opendrift_amd', 'csrc', 'odr_plast.hip')).read()
    assert 'fail(ODR_ERR_INVALID, "scale < 0' in src


def test_flag_of_a_run_is_dropped_and_the_hook_says_what_is_missing(monkeypatch):
    """_identically_zero takes the decision run() made for its steps only while that run lasts; the hook called before
    prepare_run() looks for the coefficients itself and names the three ways when there are none."""
    o = OceanDrift(loglevel=50)
    assert o._waves_on is None and o._identically_zero(SX)
    o._waves_on = True      # as inside a run with the option on
    assert not o._identically_zero(SX)
    o._waves_on = None
    o.set_config('drift:use_tabularised_stokes_drift', True)
    assert not o._identically_zero(SX)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'opendrift_amd', 'oceandrift.py')).read()
    body = src[src.index('    def run(self, time_step=None'):src.index('    def _one_launch_codes')]
    assert body.count('self._waves_on = None') == 2      # behind the loop, and where an exception leaves it
    o.P = StubParticles()
    monkeypatch.setattr(type(o), 'num_elements_active', lambda self: 3)
    with pytest.raises(FileNotFoundError, match='not shipped'):
        o._parameterise_waves(list(o.required_variables))
    o._stokes_tables_argument = TABLES
    o._parameterise_waves(list(o.required_variables))
    assert o.P.calls == [('stokes_from_wind', 7, 2)]
