"""CPU: the two method predicates of run() -- may the step's mixing launch be enqueued before the host has read the status scan
(`speculate`), may the step's collective finish behind update() (`stock_update`) -- for every model class.  They are decided by
what a class overrides and by its fuse_vertical_advection, so a model that gains or loses an override shows here.  And what run()
decides from a configured instance before its loop, without a device: the lane (_run_lane), the re-sort interval, the
speculation, the time arguments."""
import os
from datetime import datetime, timedelta

import pytest

from opendrift_amd.larvalfish import LarvalFish
from opendrift_amd.larvalfish_extended import LarvalFishExtended
from opendrift_amd.leeway import Leeway
from opendrift_amd.oceandrift import OceanDrift
from opendrift_amd.openberg import OpenBerg
from opendrift_amd.openoil import OpenOil
from opendrift_amd.pelagicegg import PelagicEggDrift
from opendrift_amd.radionuclides import RadionuclideDrift
from opendrift_amd.sedimentdrift import SedimentDrift
from opendrift_amd.shipdrift import ShipDrift

# class: (speculate's method test, stock_update)
TABLE = {OceanDrift: (True, True), OpenBerg: (True, False), ShipDrift: (True, False), OpenOil: (False, False), Leeway: (False, False),
         PelagicEggDrift: (False, False), SedimentDrift: (False, False), LarvalFish: (False, False), LarvalFishExtended: (False, False),
         RadionuclideDrift: (False, False)}


@pytest.mark.parametrize('cls', list(TABLE), ids=lambda c: c.__name__)
def test_method_predicates(cls):
    assert (cls._stock_speculation_methods(), cls._stock_update()) == TABLE[cls]


def test_a_subclass_that_overrides_vertical_advection_does_not_fuse():
    class Mine(OceanDrift):
        def vertical_advection(self):
            pass
    assert OceanDrift._fuses_vertical_advection() and not Mine._fuses_vertical_advection()
    assert not Mine._stock_speculation_methods() and not Mine._stock_update()
    for cls in (PelagicEggDrift, SedimentDrift, LarvalFish, LarvalFishExtended, RadionuclideDrift):
        assert cls.vertical_advection is OceanDrift.vertical_advection and not cls._fuses_vertical_advection()


WFORCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wforce.dat')


class _OwnEnvironment(OceanDrift):
    def get_environment(self):
        pass


def _model(cls, config=(), **kw):
    o = cls(loglevel=50, **({'wforce': WFORCE} if cls is ShipDrift else {}), **kw)
    for key, value in config:
        o.set_config(key, value)
    return o


# (class, constructor arguments, configuration): lane -- no readers, default configuration otherwise
LANES = [
    (OceanDrift, {}, (), 'fused'),
    (OceanDrift, {'rng': 'numpy'}, (), 'fused'),
    (OceanDrift, {'rng': 'numpy'}, (('drift:current_uncertainty', 0.1), ), 'call_by_call'),
    (OceanDrift, {'rng': 'numpy'}, (('drift:wind_uncertainty', 0.1), ), 'call_by_call'),
    (OceanDrift, {}, (('drift:max_age_seconds', 3600), ), 'call_by_call'),
    (OceanDrift, {}, (('general:seafloor_action', 'deactivate'), ), 'call_by_call'),
    (OceanDrift, {}, (('general:coastline_approximation_precision', 0.001), ), 'call_by_call'),
    (OceanDrift, {}, (('drift:deactivate_west_of', 3.0), ), 'call_by_call'),      # (the land mask has no fallback)
    (OceanDrift, {}, (('drift:water_column_stretching', True), ), 'call_by_call'),
    (OceanDrift, {}, (('drift:truncate_ocean_model_below_m', 50), ), 'call_by_call'),
    (Leeway, {}, (), 'leeway'),
    (Leeway, {'rng': 'numpy'}, (), 'call_by_call'),
    (Leeway, {}, (('processes:capsizing', True), ), 'call_by_call'),
    (_OwnEnvironment, {}, (), 'call_by_call'),
] + [(cls, kw, (), 'call_by_call') for cls in (OpenOil, OpenBerg, ShipDrift, PelagicEggDrift, SedimentDrift, LarvalFish,
                                               LarvalFishExtended, RadionuclideDrift) for kw in ({}, {'rng': 'numpy'})]


@pytest.mark.parametrize('cls,kw,config,lane', LANES, ids=lambda v: getattr(v, '__name__', None) or str(v))
def test_lane_of_a_configured_model(cls, kw, config, lane, monkeypatch):
    monkeypatch.delenv('ODR_RUN_UNFUSED', raising=False)
    o = _model(cls, config, **kw)
    assert o._run_lane() == lane
    monkeypatch.setenv('ODR_RUN_UNFUSED', '1')      # (read when run() starts: the same instance answers anew)
    assert o._run_lane() == 'call_by_call'
    assert o._ctx is None                           # no device context was made for the answer


def test_default_sort_interval(monkeypatch):
    monkeypatch.delenv('ODR_RUN_UNFUSED', raising=False)
    lw, o = _model(Leeway), _model(OceanDrift)
    assert lw._sort_interval(lw._run_lane()) == 48
    assert 'upward_sea_water_velocity' in o.required_variables and o._sort_interval(o._run_lane()) == 24
    o.required_variables.pop('upward_sea_water_velocity')      # (what run() does for drift:vertical_advection False)
    assert o._run_lane() == 'fused' and o._sort_interval('fused') == 16
    assert o._sort_interval('call_by_call') == 16 and _model(OpenOil)._sort_interval('call_by_call') == 16
    o.sort_every = 0
    assert o._sort_interval('fused') == 0


def test_speculation(monkeypatch):
    monkeypatch.delenv('ODR_RUN_UNFUSED', raising=False)
    monkeypatch.delenv('ODR_NO_SPECULATION', raising=False)
    assert not _model(OceanDrift)._speculates('fused')       # drift:vertical_mixing is off
    o = _model(OceanDrift, (('drift:vertical_mixing', True), ))      # no reader: calm, no Stokes drift
    assert o._run_lane() == 'fused' and o._speculates('fused') is True and not o._speculates('call_by_call')
    assert not _model(OceanDrift, (('drift:vertical_mixing', True), ), rng='numpy')._speculates('fused')
    monkeypatch.setenv('ODR_NO_SPECULATION', '1')
    assert o._speculates('fused') is False and o._ctx is None


def _seeded():
    o = _model(OceanDrift)
    o.seed_elements(lon=4.0, lat=60.0, time=datetime(2020, 1, 1))
    return o


def test_time_arguments():
    with pytest.raises(ValueError, match='Only one of'):
        _seeded()._time_arguments(600, 3, None, timedelta(hours=1), None)
    with pytest.raises(ValueError, match='must be an integer'):
        _seeded()._time_arguments(600, 3, 900, None, None)
    o = _seeded()
    assert o._time_arguments(600, None, 1800, timedelta(minutes=50), None) == (6, 3)      # rounded up to the output step
    assert o.time_step == timedelta(seconds=600) and o.time_step_output == timedelta(seconds=1800)
    assert o.expected_steps_calculation == 6
    o = _seeded()
    steps, out_every = o._time_arguments(-600, None, None, timedelta(hours=1), None)
    assert (steps, out_every) == (6, 1) and o.time_step == timedelta(seconds=-600) and o.time_step_output == o.time_step
    assert o.start_time == datetime(2020, 1, 1) and o._ctx is None
