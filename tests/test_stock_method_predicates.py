"""CPU: the two method predicates of run() -- may the step's mixing launch be enqueued before the host has read the status scan
(`speculate`), may the step's collective finish behind update() (`stock_update`) -- for every model class.  They are decided by
what a class overrides and by its fuse_vertical_advection, so a model that gains or loses an override shows here."""
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
