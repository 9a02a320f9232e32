"""CPU: the host side of RadionuclideDrift (opendrift_amd/radionuclides.py) -- what can be checked without a device: the class,
its configuration against the reference's (opendrift/models/radionuclides.py:112-208), the five species setups, the transfer rates
against the golden C30 (written by the reference), seeding with the reference's draws, what it refuses, and the C ABI entries."""
import os
import re
from datetime import datetime

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = datetime(2020, 1, 1)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'c30_radionuclides.npz')
REQUIRED = {   # :77-96
    'x_sea_water_velocity': None, 'y_sea_water_velocity': None, 'sea_surface_height': 0, 'x_wind': 0, 'y_wind': 0,
    'land_binary_mask': None, 'sea_floor_depth_below_sea_level': None, 'ocean_vertical_diffusivity': 0.0001,
    'ocean_mixed_layer_thickness': 50, 'sea_water_temperature': 10, 'sea_water_salinity': 34, 'horizontal_diffusivity': 0,
    'upward_sea_water_velocity': 0, 'conc3': 1.e-3}
FLOATS = {   # key: (default, min, max, units)    :112-198
    'radionuclide:dissolved_diameter': (0, 0, 100e-6, 'm'),
    'radionuclide:particle_diameter': (5e-6, .45e-6, 63.e-6, 'm'),
    'radionuclide:particle_diameter_uncertainty': (1e-7, 0, 100e-6, 'm'),
    'radionuclide:particle_diameter_minimum': (0.45e-6, 0, 100e-6, 'm'),
    'radionuclide:particle_diameter_maximum': (63.e-6, 0, 100e-6, 'm'),
    'seed:LMM_fraction': (.1, 0, 1, '1'),
    'seed:particle_fraction': (0.9, 0, 1, '1'),
    'seed:slowly_fraction': (0., 0, 1, '1'),
    'seed:total_release': (100.e9, 0, 1e36, 'Bq'),
    'radionuclide:transformations:Kd': (2.0, 0, 1e9, 'm3/kg'),
    'radionuclide:transformations:Dc': (1.16e-5, 0, 1e6, ''),
    'radionuclide:transformations:slow_coeff': (1.2e-7, 0, 1e6, ''),
    'radionuclide:sediment:sedmixdepth': (1, 0, 100, 'm'),
    'radionuclide:sediment:sediment_density': (2600, 0, 10000, 'kg/m3'),
    'radionuclide:sediment:effective_fraction': (0.9, 0, 1, ''),
    'radionuclide:sediment:corr_factor': (0.1, 0, 10, ''),
    'radionuclide:sediment:porosity': (0.6, 0, 1, ''),
    'radionuclide:sediment:layer_thick': (1, 0, 100, 'm'),
    'radionuclide:sediment:desorption_depth': (1, 0, 100, 'm'),
    'radionuclide:sediment:desorption_depth_uncert': (.5, 0, 100, 'm'),
    'radionuclide:sediment:resuspension_depth': (1, 0, 100, 'm'),
    'radionuclide:sediment:resuspension_depth_uncert': (.5, 0, 100, 'm'),
    'radionuclide:sediment:resuspension_critvel': (.01, 0, 1, 'm/s'),
}
BASE3 = ['LMM', 'Particle reversible', 'Sediment reversible']
SLOW, IRREV = ['Particle slowly reversible', 'Sediment slowly reversible'], ['Particle irreversible', 'Sediment irreversible']
SPECIES = {   # init_species (:233-278)
    'LMM + Rev': BASE3, 'LMM + Rev + Slow rev': BASE3 + SLOW, 'LMM + Rev + Irrev': BASE3 + IRREV,
    'LMM + Rev + Slow rev + Irrev': BASE3 + SLOW + IRREV,
    'LMM + Colloid + Rev': ['LMMcation', 'LMManion', 'Humic colloid', 'Polymer', 'Particle reversible', 'Sediment reversible']}
ISOTOPE_OF = {'LMM + Rev': '137Cs', 'LMM + Rev + Slow rev': '137Cs', 'LMM + Rev + Irrev': '137Cs', 'LMM + Rev + Slow rev + Irrev': '241Am',
              'LMM + Colloid + Rev': 'Al'}


def model(**kw):
    from opendrift_amd import RadionuclideDrift
    return RadionuclideDrift(loglevel=50, **kw)


def configured(setup, isotope=None):
    o = model()
    o.set_config('radionuclide:isotope', isotope or ISOTOPE_OF[setup])
    o.set_config('radionuclide:specie_setup', setup)
    return o


def test_class_config_keys_and_defaults():
    from opendrift_amd.oceandrift import OceanDrift
    o = model()
    assert isinstance(o, OceanDrift)
    for key, (default, lo, hi, units) in FLOATS.items():
        spec = o.get_configspec(key)[key]
        assert (spec['type'], spec['default'], spec['min'], spec['max'], spec['units']) == ('float', default, lo, hi, units), key
    spec = o.get_configspec('radionuclide:')
    assert spec['radionuclide:particlesize_distribution']['enum'] == ['normal', 'lognormal']
    assert spec['radionuclide:particlesize_distribution']['default'] == 'normal'
    assert spec['radionuclide:isotope']['enum'] == ['Al', '137Cs', '129I', '241Am', 'manual'] and spec['radionuclide:isotope']['default'] == '137Cs'
    assert spec['radionuclide:specie_setup']['enum'] == list(SPECIES) and spec['radionuclide:specie_setup']['default'] == 'LMM + Rev'
    assert spec['radionuclide:output:depthintervals']['default'] == '-25, -10., -5., -1.'
    # under 'radionuclide:': the 19 float keys above and 4 enum / str keys; the other four float keys are seed:*
    floats = [k for k in FLOATS if k.startswith('radionuclide:')]
    assert len(floats) == 19 and len(FLOATS) == 23 and len(spec) == 19 + 4
    assert set(spec) == set(floats) | {'radionuclide:particlesize_distribution', 'radionuclide:isotope', 'radionuclide:specie_setup',
                                       'radionuclide:output:depthintervals'}
    assert o.get_config('drift:vertical_mixing') is True and o.get_config('drift:vertical_mixing_at_surface') is True
    assert o.get_config('drift:vertical_advection_at_surface') is True
    with pytest.raises(ValueError):
        o.set_config('radionuclide:particle_diameter', 1e-7)      # below the minimum of 0.45e-6


def test_required_variables_and_conc3_rides_a_slot_of_this_model_only():
    from opendrift_amd import _abi
    from opendrift_amd.radionuclides import CONC3_SLOT, RadionuclideDrift
    assert {k: v['fallback'] for k, v in RadionuclideDrift.required_variables.items()} == REQUIRED and len(REQUIRED) == 14
    for v in ('ocean_vertical_diffusivity', 'sea_water_temperature', 'sea_water_salinity'):
        assert RadionuclideDrift.required_variables[v].get('profiles') is True
    o = model()
    for v, fb in REQUIRED.items():
        assert o.get_config('environment:fallback:%s' % v) == fb
    assert 'conc3' not in _abi.VARIABLES and _abi.NVAR == 26 and CONC3_SLOT == 'sea_surface_swell_wave_significant_height'
    assert CONC3_SLOT not in RadionuclideDrift.required_variables
    from opendrift_amd.device import _vid
    assert _vid('conc3', {'conc3': _abi.VARIABLES[CONC3_SLOT]}) == 22
    with pytest.raises(Exception):
        _vid('conc3', {})      # no other context resolves the name


def test_element_properties():
    from opendrift_amd import _abi
    o = model()
    assert o.aux_properties == ['diameter', 'neutral_buoyancy_salinity', 'density', 'specie'] == _abi.RADIO_PROPERTIES
    assert o.aux_defaults == {'diameter': 0., 'neutral_buoyancy_salinity': 31.25, 'density': 2650., 'specie': 0}
    assert o.get_config('seed:density') == 2650. and o.get_config('seed:neutral_buoyancy_salinity') == 31.25


@pytest.mark.parametrize('setup', list(SPECIES))
def test_species_lists_and_numbers(setup):
    o = configured(setup)
    o.check_speciation()
    o.init_species()
    assert o.name_species == SPECIES[setup] and o.nspecies == len(SPECIES[setup])
    if setup == 'LMM + Rev + Irrev':      # (no rates: see test_transfer_rates_equal_the_references)
        return
    o.init_transfer_rates()
    assert o.species_slowly_fraction == ('Slow rev' in setup) and o.species_irreversible_fraction == ('Irrev' in setup)
    for k, name in enumerate(o.name_species):
        assert o.specie_num2name(k) == name and o.specie_name2num(name) == k
    assert o.ntransformations.shape == (o.nspecies, o.nspecies) and not o.ntransformations.any()
    t = o.transfer_rates
    assert t.shape == ((4,) if setup == 'LMM + Colloid + Rev' else ()) + (o.nspecies, o.nspecies)
    for tt in (t if t.ndim == 3 else [t]):
        assert (np.diag(tt) == 0).all() and (tt >= 0).all()
    m = o.setup_members()
    assert m['nspecies'] == o.nspecies and (m['lmm'] >= 0) != (m['lmmcation'] >= 0)
    assert o.particle_species() == [k for k, n in enumerate(o.name_species) if n.startswith('Particle')]


def test_transfer_rates_equal_the_references():
    """transfer_rates and name_species of every specie setup against what the reference's own init_species / init_transfer_rates
    gave (stored in C30 as setup0 .. setup3, with the isotope each was made for), bit for bit.  The fifth, 'LMM + Rev + Irrev',
    fails in the reference (AttributeError: :579 reads num_ssrev, which that setup never sets) and is refused by name here."""
    G = np.load(GOLDEN)
    seen = []
    for k in range(4):
        setup, isotope = str(G['setup%d_name' % k]), str(G['setup%d_isotope' % k])
        o = configured(setup, isotope)
        o.set_config('radionuclide:transformations:slow_coeff', 2e-5)
        o.check_speciation()
        o.init_species()
        o.init_transfer_rates()
        assert o.name_species == list(G['setup%d_species' % k]), setup
        assert o.transfer_rates.shape == G['setup%d_rates' % k].shape and np.array_equal(o.transfer_rates, G['setup%d_rates' % k]), setup
        assert (o.transfer_rates > 0).sum() >= 4
        seen.append(setup)
    assert sorted(seen + ['LMM + Rev + Irrev']) == sorted(SPECIES)
    # the two cases of the golden run with these tables
    for case, k in (('a', 2), ('b', 3)):
        assert list(G[case + '_name_species']) == list(G['setup%d_species' % k])
    assert np.array_equal(G['b_transfer_rates'], G['setup3_rates'])
    a = configured('LMM + Rev + Slow rev + Irrev')      # 241Am: another Kd than setup2's 129I
    a.set_config('radionuclide:transformations:slow_coeff', 2e-5)
    a.init_species()
    a.init_transfer_rates()
    assert a.kd == 2.0e3 and np.array_equal(a.transfer_rates, G['a_transfer_rates'])
    b = configured('LMM + Colloid + Rev')
    b.init_species()
    b.init_transfer_rates()
    assert b.kd is None and b.salinity_intervals == [0, 1, 10, 20]
    s = configured('LMM + Rev + Irrev', '137Cs')
    s.init_species()
    with pytest.raises(NotImplementedError, match='LMM \\+ Rev \\+ Irrev'):
        s.init_transfer_rates()


@pytest.mark.parametrize('case', ['a', 'b'])
def test_seeding_draws_the_species_as_the_reference_does(case):
    """The same np.random.seed, the same fractions: the species of the golden's seeding, element by element; the particle
    species get a diameter around the mean, the dissolved ones 0 (the noise comes from an unseeded generator in the reference)."""
    G = np.load(GOLDEN)
    cfg = dict(zip(G[case + '_config_keys'].tolist(), G[case + '_config_values'].tolist()))
    o = configured('LMM + Rev + Slow rev + Irrev' if case == 'a' else 'LMM + Colloid + Rev')
    for k in ('seed:LMM_fraction', 'seed:particle_fraction', 'seed:slowly_fraction', 'radionuclide:particle_diameter',
              'radionuclide:particle_diameter_uncertainty', 'radionuclide:transformations:slow_coeff'):
        o.set_config(k, cfg[k])
    n = len(G[case + '_seed_lon'])
    np.random.seed(int(G[case + '_seed']))
    o.seed_elements(lon=G[case + '_seed_lon'], lat=G[case + '_seed_lat'], z=G[case + '_seed_z'], time=T0, number=n,
                    diameter_rng=np.random.default_rng(1))
    assert o._sched['specie'].dtype == np.float32 and np.array_equal(o._sched['specie'], G[case + '_seed_specie'])
    particle = np.isin(o._sched['specie'], o.particle_species())
    d, ref = o._sched['diameter'], G[case + '_seed_diameter']
    assert d.dtype == np.float32 and (d[~particle] == 0).all() and (ref[~particle] == 0).all()
    mean, sd = cfg['radionuclide:particle_diameter'], cfg['radionuclide:particle_diameter_uncertainty']
    assert abs(d[particle].mean() - mean) < 5 * sd / np.sqrt(particle.sum()) and abs(ref[particle].mean() - mean) < 5 * sd / np.sqrt(particle.sum())
    assert 0.5 * sd < d[particle].std() < 1.5 * sd
    assert (o._sched['density'] == np.float32(2650)).all() and (o._sched['neutral_buoyancy_salinity'] == np.float32(31.25)).all()


def test_seeding_by_specie_and_the_fraction_sum():
    o = configured('LMM + Rev')
    o.seed_elements(lon=4.0, lat=60.0, number=6, time=T0, specie=1, z=-5.)
    assert (o._sched['specie'] == 1).all() and (o._sched['diameter'] > 0).all()
    o = configured('LMM + Rev')
    with pytest.raises(ValueError, match='Illegal specie fraction combination'):
        o.seed_elements(lon=4.0, lat=60.0, number=6, time=T0, LMM_fraction=0.5, particle_fraction=0.6)
    o = configured('LMM + Rev')
    with pytest.raises(ValueError, match='specie must be in'):
        o.seed_elements(lon=4.0, lat=60.0, number=6, time=T0, specie=3)


def test_refusals_by_name():
    from opendrift_amd.radionuclides import REFUSED_SEAFLOOR_ACTIONS
    o = model()
    with pytest.raises(NotImplementedError, match="'manual'"):
        o.set_config('radionuclide:isotope', 'manual')
    with pytest.raises(NotImplementedError, match='TSprofiles'):
        o.set_config('vertical_mixing:TSprofiles', True)
    o = configured('LMM + Colloid + Rev', '137Cs')
    with pytest.raises(ValueError, match='Illegal speciation for 137Cs'):
        o.seed_elements(lon=4.0, lat=60.0, number=3, time=T0)
    o = configured('LMM + Rev')
    with pytest.raises(NotImplementedError, match='sediment'):
        o.seed_elements(lon=4.0, lat=60.0, number=3, time=T0, specie=[0, 2, 2])
    assert set(REFUSED_SEAFLOOR_ACTIONS) == {'none', 'previous'}
    for action in REFUSED_SEAFLOOR_ACTIONS:
        o = configured('LMM + Rev')
        o.set_config('general:seafloor_action', action)
        o.seed_elements(lon=4.0, lat=60.0, number=3, time=T0)
        with pytest.raises(NotImplementedError, match="'%s'" % action):      # when run() starts: nothing has touched a device yet
            o.run(time_step=600, steps=1)
        assert o._ctx is None and o.mode == 'Ready'


def test_a_sharded_run_is_refused(monkeypatch):
    from opendrift_amd import distributed as D
    monkeypatch.setattr(D, 'env_world', lambda: (1, 0, 2))
    with pytest.raises(NotImplementedError, match='sharded'):
        model()


def test_run_takes_the_call_by_call_lane():
    from opendrift_amd import RadionuclideDrift
    from opendrift_amd.oceandrift import OceanDrift
    assert RadionuclideDrift.update is not OceanDrift.update
    assert not RadionuclideDrift._fuses_vertical_advection()
    assert RadionuclideDrift._with_seafloor_action is not OceanDrift._with_seafloor_action
    assert RadionuclideDrift.vertical_mixing is OceanDrift.vertical_mixing
    assert RadionuclideDrift.interact_with_seafloor is OceanDrift.interact_with_seafloor
    assert RadionuclideDrift(loglevel=50)._run_lane() == 'call_by_call'


def test_abi_entries_are_declared_and_bound():
    from opendrift_amd import _abi, device
    src = open(os.path.join(ROOT, 'include', 'odrift.h')).read()
    for name in ('odr_radio_create', 'odr_radio_counts', 'odr_radio_destroy', 'odr_radio_speciation', 'odr_radio_terminal_velocity',
                 'odr_radio_resuspend'):
        assert re.search(r'\bint %s\(odr_ctx \*ctx' % name, src), name
        assert name in _abi._SIGNATURES and name in _abi.EXPORTS
    assert re.search(r'\bODR_SEAFLOOR_SETTLE_SPECIES = 5\b', src) and _abi.SEAFLOOR['settle_species'] == 5
    assert re.search(r'models/radionuclides\.py:728-810', src) and re.search(r'radionuclides\.py:665-721', src)
    assert re.search(r'resuspension \(:946-997\)', src) and re.search(r'radionuclides\.py:912-942', src)
    import ctypes as C
    # odr_radio_setup: 13 int32 (padded to 56 bytes), 196 + 9 doubles
    assert C.sizeof(_abi.RadioSetup) == 56 + 8 * (196 + 9)
    for name in ('radio_setup', 'radio_speciation', 'radio_terminal_velocity', 'radio_resuspend'):
        assert callable(getattr(device.Particles, name))
    assert callable(device.Context.set_seafloor_settle_species)
