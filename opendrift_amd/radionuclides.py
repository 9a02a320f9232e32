"""RadionuclideDrift on the device path: elements that carry a discrete species (dissolved, bound to particles, bound to the
sea bed, ...) which changes stochastically every step from a transfer-rate matrix.

Mirrors opendrift/models/radionuclides.py:27-1044 (Simonsen et al. 2019a, b):

  element properties (Radionuclide, :31-55): diameter, neutral_buoyancy_salinity, density, specie -- float32, in the property
  slots of odr_particles_set_property (include/odrift.h ODR_RADIO_*), carried through compaction and sort and recorded in
  `o.result`; `specie` (int32 there) is a small integer held exactly;
  required_variables with their fallbacks (:77-96), every config key of :112-208;
  check_speciation, init_species, init_kd, init_transfer_rates (:233-278, :320-342, :483-654) on the host, all five species
  setups: name_species, nspecies, transfer_rates, specie_num2name, specie_name2num;
  seed_elements (:349-479): specie= or the LMM / particle / slowly fractions drawn with np.random.rand BEFORE the positions, the
  fraction-sum ValueError, initial diameters of the particle species by set_init_diameter's arithmetic;
  update() (:1004-1038) = speciation -> terminal velocity -> vertical mixing (or vertical_buoyancy) -> resuspension ->
  advect_ocean_current -> vertical_advection, on the call-by-call lane of run():
    update_transfer_rates + update_speciation with the diameter, sorption and desorption updates = ONE launch
    (odr_radio_speciation, csrc/odr_radio.hip.h); update_terminal_velocity = ONE launch (odr_radio_terminal_velocity);
    bottom_interaction (:912-942) INSIDE the device's sea-floor check of the mixing sub-steps and of vertical_buoyancy
    (ODR_SEAFLOOR_SETTLE_SPECIES: a particle species below the floor is lifted onto it and gets moving = 0, any other species
    is only lifted), its change of species and its counters at the head of the next launch; resuspension = ONE launch
    (odr_radio_resuspend);
  ntransformations: the device's counters, read after run().

The reference's hook settles every particle with z <= Zmin in a sub-step in which some element is below the floor; the device
settles the ones that were below -- the difference sedimentdrift.py describes (an element exactly on Zmin without having been
below).

terminal_velocity.  The reference re-evaluates W * moving at the top of every mixing sub-step; the device multiplies by moving
inside the walk, so the trajectories agree, but the STORED terminal_velocity of an element that settled during the step is W
here and 0 there.  The reference's value is float64 where `density` was not given at seeding (the default seeds a float64
array); the device holds float32.

conc3 (suspended-matter concentration) has no device id of its own: on this model's device context it rides the slot of
sea_surface_swell_wave_significant_height, which only the windsea_swell Stokes profile reads and this model has no Stokes drift
(Context.slot_aliases, set by RadionuclideDrift.ctx).  No other model's context resolves the name.

Random numbers.  The reference draws u2 and the normals compacted over the affected elements only, and the diameter noise from
an UNSEEDED np.random.default_rng() (:297): a run can never consume the stream as the reference does -- the situation of
OpenOil's intrusion depths (openoil.py).  rng='numpy' draws, per step, random(n) twice and normal(n) twice for the speciation,
random(n) once per mixing sub-step, normal(n) twice for the resuspension; rng='device' uses Philox streams keyed by (ID, step).
Exact parity with the reference is tested at kernel level, with its recorded draws scattered to their elements.

Not built, refused by name: radionuclide:isotope 'manual' (the reference itself fails with KeyError in
check_speciation), the specie setup 'LMM + Rev + Irrev' (the reference fails with AttributeError in init_transfer_rates: its
irreversible species are fed from slowly reversible ones, which the setup lacks), vertical_mixing:TSprofiles, seeding that mixes
sediment with other species (the reference calls exit()), a sharded run (the counters would need a reduction), general:seafloor_action 'none' / 'previous', a lognormal size distribution
with a dissolved diameter > 0 under rng='numpy'.  The density maps and the GUI post-processing (:1050-1774) are out of scope.
"""
import logging

import numpy as np

from . import _abi
from .config import CONFIG_LEVEL_ADVANCED, CONFIG_LEVEL_BASIC, CONFIG_LEVEL_ESSENTIAL
from .oceandrift import OceanDrift, OpenDriftSimulation

logger = logging.getLogger(__name__)

CONC3_SLOT = 'sea_surface_swell_wave_significant_height'
REFUSED_SEAFLOOR_ACTIONS = ('none', 'previous')
SPECIE_SETUPS = ['LMM + Rev', 'LMM + Rev + Slow rev', 'LMM + Rev + Irrev', 'LMM + Rev + Slow rev + Irrev', 'LMM + Colloid + Rev']
LEGAL_SPECIES = {      # check_speciation (:324-334)
    '137Cs': SPECIE_SETUPS[:4],
    '129I': ['LMM + Rev', 'LMM + Rev + Slow rev + Irrev'],
    '241Am': ['LMM + Rev', 'LMM + Rev + Slow rev', 'LMM + Rev + Slow rev + Irrev'],
    'Al': ['LMM + Colloid + Rev'],
}
KD_VALUES = {'137Cs': 4.0e0, '129I': 7.0e-2, '241Am': 2.0e3, 'Al': None}      # IAEA (2004) (:488-492)
SALINITY_INTERVALS = [0, 1, 10, 20]      # :597


def species_names(setup):
    """init_species (:233-278): (name_species, slowly fraction enabled, irreversible fraction enabled)."""
    s, names = setup.casefold(), []
    if 'lmm + rev' in s:
        names += ['LMM', 'Particle reversible', 'Sediment reversible']
    slow, irrev = '+ slow rev' in s, '+ irrev' in s
    if slow:
        names += ['Particle slowly reversible', 'Sediment slowly reversible']
    if irrev:
        names += ['Particle irreversible', 'Sediment irreversible']
    if s == 'lmm + colloid + rev':
        names += ['LMMcation', 'LMManion', 'Humic colloid', 'Polymer', 'Particle reversible', 'Sediment reversible']
    return names, slow, irrev


AL_RATES = (      # 'LMM + Colloid + Rev' (:602-644; Simonsen et al. 2019b), one row per salinity interval of SALINITY_INTERVALS:
    # LMMcation -> Humic colloid, -> Particle reversible, -> Polymer [1/s]; Humic colloid -> LMMcation [Dc], -> Particle reversible [1/s];
    # Particle reversible -> LMMcation [Dc]; Sediment reversible -> LMMcation [Dc]; Polymer -> Particle reversible [1/s]
    (1.2e-5, 4.e-6, None, .3, 2.e-6, .3, .03, None),      # (no polymer below 1 psu)
    (1.e-5, 3.e-6, 1.2e-4, 7., 4.e-6, .5, .05, 2.4e-5),
    (8.e-6, 2.e-6, 1.4e-4, 7., 6.e-6, .6, .06, 6.e-5),
    (6.e-6, 1.8e-6, 1.5e-4, 7., 1.e-5, .8, .08, 8.e-5))


def transfer_rates(setup, isotope, names, kd, cfg):
    """The rates of init_transfer_rates (:512-654) in 1/s as {(from, to): rate} by species name, laid out as [nspecies, nspecies]
    ([4, nspecies, nspecies] for 'LMM + Colloid + Rev').  cfg(key): the configuration value.  Each product is formed in the
    reference's order of factors, so that the values equal the reference's bit for bit (golden C30)."""
    s = setup.casefold()
    Dc = cfg('radionuclide:transformations:Dc')
    slow = cfg('radionuclide:transformations:slow_coeff')
    sed = lambda k: cfg('radionuclide:sediment:' + k)      # noqa: E731
    LMM, P, S = 'LMM', 'Particle reversible', 'Sediment reversible'
    PS, SS, PI, SI = 'Particle slowly reversible', 'Sediment slowly reversible', 'Particle irreversible', 'Sediment irreversible'
    tables = [{}]
    if 'lmm + rev' in s:      # :540-554 (Simonsen et al. 2019a, the reversible fraction only); 1e-3 kg/m3 of suspended matter
        tables[0].update({
            (LMM, P): Dc * kd * 1.e-3,
            (P, LMM): Dc,
            (LMM, S): Dc * kd * sed('sedmixdepth') * sed('sediment_density') * (1. - sed('porosity')) * sed('effective_fraction')
            * sed('corr_factor') / sed('layer_thick'),
            (S, LMM): Dc * sed('corr_factor')})
    if '+ slow rev' in s:      # :562-570
        tables[0].update({(S, SS): slow, (P, PS): slow, (SS, S): slow * .1, (PS, P): slow * .1})
    if '+ irrev' in s:      # :574-580
        if '+ slow rev' not in s:      # (the reference reads self.num_ssrev, which only '+ Slow rev' sets: AttributeError, :579)
            raise NotImplementedError("the transfer rates of '%s' are not defined: the irreversible species are fed from the slowly "
                                      "reversible ones, which this setup lacks -- the reference itself fails on it" % setup)
        tables[0].update({(SS, SI): slow, (PS, PI): slow})
    if s == 'lmm + colloid + rev' and isotope.casefold() == 'al':
        C, A, H, POL = 'LMMcation', 'LMManion', 'Humic colloid', 'Polymer'
        tables = []
        for c_h, c_p, c_pol, h_c, h_p, p_c, s_c, pol_p in AL_RATES:
            t = {(C, H): c_h, (C, P): c_p, (H, C): h_c * Dc, (H, P): h_p, (P, C): p_c * Dc, (S, C): s_c * Dc}
            if c_pol is not None:
                t.update({(C, POL): c_pol, (A, POL): 5.e-6, (POL, A): 12. * Dc, (POL, P): pol_p})
            tables.append(t)
    T = np.zeros([len(tables), len(names), len(names)])
    for a, t in enumerate(tables):
        for (src, dst), rate in t.items():
            if src != dst:      # (no species transforms to itself: the diagonal stays 0, :649-654)
                T[a, names.index(src), names.index(dst)] = rate
    return T if len(tables) > 1 else T[0]


class RadionuclideDrift(OceanDrift):
    """opendrift/models/radionuclides.py:58-1044 (see the module docstring)."""
    aux_properties = list(_abi.RADIO_PROPERTIES)     # slot order of odr_particles_set_property
    aux_defaults = {'diameter': 0., 'neutral_buoyancy_salinity': 31.25, 'density': 2650., 'specie': 0}   # :31-43
    fuse_vertical_advection = False     # update(): resuspension and the current advection lie between the mixing and the vertical advection
    required_variables = {   # :77-96
        'x_sea_water_velocity': {'fallback': None},
        'y_sea_water_velocity': {'fallback': None},
        'sea_surface_height': {'fallback': 0},
        'x_wind': {'fallback': 0},
        'y_wind': {'fallback': 0},
        'land_binary_mask': {'fallback': None},
        'sea_floor_depth_below_sea_level': {'fallback': None},
        'ocean_vertical_diffusivity': {'fallback': 0.0001, 'profiles': True},
        'ocean_mixed_layer_thickness': {'fallback': 50},
        'sea_water_temperature': {'fallback': 10, 'profiles': True},
        'sea_water_salinity': {'fallback': 34, 'profiles': True},
        'horizontal_diffusivity': {'fallback': 0},
        'upward_sea_water_velocity': {'fallback': 0},
        'conc3': {'fallback': 1.e-3},
    }

    def __init__(self, *args, **kwargs):
        from . import distributed as D
        if D.env_world()[2] > 1:      # (before anything of the sharded machinery starts)
            raise NotImplementedError('RadionuclideDrift in a sharded run: the transformation counters would need a reduction '
                                      'over the ranks (DESIGN.md section 7g)')
        super().__init__(*args, **kwargs)
        A, B, E = CONFIG_LEVEL_ADVANCED, CONFIG_LEVEL_BASIC, CONFIG_LEVEL_ESSENTIAL

        def fl(default, lo, hi, units, level=A, description=''):
            return {'type': 'float', 'default': default, 'min': lo, 'max': hi, 'units': units, 'level': level, 'description': description}
        self._add_config({      # :112-205
            'radionuclide:dissolved_diameter': fl(0, 0, 100e-6, 'm'),
            'radionuclide:particle_diameter': fl(5e-6, .45e-6, 63.e-6, 'm', description='Mean particle diameter. Determines the settling velocity.'),
            'radionuclide:particle_diameter_uncertainty': fl(1e-7, 0, 100e-6, 'm', description='Standard deviation of particle size distribution.'),
            'radionuclide:particle_diameter_minimum': fl(0.45e-6, 0, 100e-6, 'm', description='Mimimum particle size.'),
            'radionuclide:particle_diameter_maximum': fl(63.e-6, 0, 100e-6, 'm', description='Maximum particle size.'),
            'radionuclide:particlesize_distribution': {
                'type': 'enum', 'enum': ['normal', 'lognormal'], 'default': 'normal', 'level': A,
                'description': 'Distribution of particle diameter around a mean value at seeding, NB: not at sorption!'},
            'seed:LMM_fraction': fl(.1, 0, 1, '1', E, 'Fraction of initial discharge released as LMM species'),
            'seed:particle_fraction': fl(0.9, 0, 1, '1', E, 'Fraction of initial discharge released as particle species'),
            'seed:slowly_fraction': fl(0., 0, 1, '1', E, 'Fraction of PARTICLE discharge released as slowly reversible particle species'),
            'seed:total_release': fl(100.e9, 0, 1e36, 'Bq', E, 'Total release (Bq)'),
            'radionuclide:isotope': {'type': 'enum', 'default': '137Cs', 'enum': ['Al', '137Cs', '129I', '241Am', 'manual'],
                                     'level': E, 'description': 'Isotope'},
            'radionuclide:specie_setup': {'type': 'enum', 'default': 'LMM + Rev', 'enum': list(SPECIE_SETUPS), 'level': E,
                                          'description': 'Species enabled'},
            'radionuclide:transformations:Kd': fl(2.0, 0, 1e9, 'm3/kg', B),
            'radionuclide:transformations:Dc': fl(1.16e-5, 0, 1e6, ''),
            'radionuclide:transformations:slow_coeff': fl(1.2e-7, 0, 1e6, ''),
            'radionuclide:sediment:sedmixdepth': fl(1, 0, 100, 'm'),
            'radionuclide:sediment:sediment_density': fl(2600, 0, 10000, 'kg/m3'),
            'radionuclide:sediment:effective_fraction': fl(0.9, 0, 1, ''),
            'radionuclide:sediment:corr_factor': fl(0.1, 0, 10, ''),
            'radionuclide:sediment:porosity': fl(0.6, 0, 1, ''),
            'radionuclide:sediment:layer_thick': fl(1, 0, 100, 'm'),
            'radionuclide:sediment:desorption_depth': fl(1, 0, 100, 'm'),
            'radionuclide:sediment:desorption_depth_uncert': fl(.5, 0, 100, 'm'),
            'radionuclide:sediment:resuspension_depth': fl(1, 0, 100, 'm'),
            'radionuclide:sediment:resuspension_depth_uncert': fl(.5, 0, 100, 'm'),
            'radionuclide:sediment:resuspension_critvel': fl(.01, 0, 1, 'm/s'),
            'radionuclide:output:depthintervals': {'type': 'str', 'default': '-25, -10., -5., -1.', 'min_length': 0, 'max_length': 60,
                                                   'level': E, 'description': 'Depth intervals for computation of concentration'},
        })
        del self._config['seed:specie']      # drawn or given in seed_elements, never a default of the run
        self._set_config_default('drift:vertical_mixing', True)      # :206-208
        self._set_config_default('drift:vertical_mixing_at_surface', True)
        self._set_config_default('drift:vertical_advection_at_surface', True)
        self._device_setup = None
        self._ntransformations_read = None

    def set_config(self, key, value):
        if key == 'radionuclide:isotope' and value == 'manual':
            raise NotImplementedError("radionuclide:isotope = 'manual' is not implemented: the reference itself fails on it "
                                      '(KeyError in check_speciation, radionuclides.py:337; DESIGN.md section 7g)')
        super().set_config(key, value)

    @property
    def ctx(self):
        """The device context, with conc3 riding the slot of the swell height ON THIS CONTEXT (Context.slot_aliases): nothing in
        this model's launches reads that variable.  No other model's context resolves the name."""
        c = OpenDriftSimulation.ctx.fget(self)
        c.slot_aliases['conc3'] = _abi.VARIABLES[CONC3_SLOT]
        return c

    # ------------------------------------------------------------------ species (:99-104, :233-278, :320-342, :483-654)
    def specie_num2name(self, num):
        return self.name_species[num]

    def specie_name2num(self, name):
        return self.name_species.index(name)

    def check_speciation(self):
        isotop, setup = self.get_config('radionuclide:isotope'), self.get_config('radionuclide:specie_setup')
        if setup not in LEGAL_SPECIES[isotop]:      # (the reference logs the error and calls exit())
            raise ValueError('Illegal speciation for %s: %s' % (isotop, setup))

    def init_species(self):
        self.specie_setup = self.get_config('radionuclide:specie_setup')
        self.name_species, self.species_slowly_fraction, self.species_irreversible_fraction = species_names(self.specie_setup)
        self.nspecies = len(self.name_species)

    def init_kd(self):
        self.kd = KD_VALUES[self.isotope]

    def init_transfer_rates(self):
        self.isotope = self.get_config('radionuclide:isotope')
        self.init_kd()
        self.transfer_rates = transfer_rates(self.specie_setup, self.isotope, self.name_species, self.kd, self.get_config)
        self._ntransformations_read = None
        num = lambda name: self.name_species.index(name) if name in self.name_species else -1      # noqa: E731
        self.num_lmm, self.num_prev, self.num_srev = num('LMM'), num('Particle reversible'), num('Sediment reversible')
        self.num_psrev, self.num_ssrev = num('Particle slowly reversible'), num('Sediment slowly reversible')
        self.num_pirrev, self.num_sirrev = num('Particle irreversible'), num('Sediment irreversible')
        self.num_lmmanion, self.num_lmmcation = num('LMManion'), num('LMMcation')
        self.num_humcol, self.num_polymer = num('Humic colloid'), num('Polymer')
        if self.transfer_rates.ndim == 3:
            self.salinity_intervals = list(SALINITY_INTERVALS)
        self._drop_device_setup()

    @property
    def ntransformations(self):
        """[nspecies, nspecies] transformations in -> out: the device's counters (the host waits for the device)."""
        if self._device_setup is not None:
            self._ntransformations_read = self._device_setup.counts().astype(np.float64)
        if self._ntransformations_read is None:
            return np.zeros([self.nspecies, self.nspecies])
        return self._ntransformations_read

    def _drop_device_setup(self):
        if self._device_setup is not None:
            self._ntransformations_read = self._device_setup.counts().astype(np.float64)
            self._device_setup.close()
            self._device_setup = None

    def setup_members(self):
        """The members of odr_radio_setup (device.Particles.radio_setup) for the present configuration."""
        g = self.get_config
        return dict(
            rates=self.transfer_rates, nspecies=self.nspecies, lognormal=g('radionuclide:particlesize_distribution') == 'lognormal',
            lmm=self.num_lmm, lmmcation=self.num_lmmcation, lmmanion=self.num_lmmanion, polymer=self.num_polymer,
            particle_rev=self.num_prev, sediment_rev=self.num_srev, particle_slow=self.num_psrev, sediment_slow=self.num_ssrev,
            particle_irrev=self.num_pirrev, sediment_irrev=self.num_sirrev,
            layer_thick=g('radionuclide:sediment:layer_thick'), particle_diameter=g('radionuclide:particle_diameter'),
            dissolved_diameter=g('radionuclide:dissolved_diameter'), diameter_uncertainty=g('radionuclide:particle_diameter_uncertainty'),
            desorption_depth=g('radionuclide:sediment:desorption_depth'),
            desorption_depth_uncert=g('radionuclide:sediment:desorption_depth_uncert'),
            resuspension_depth=g('radionuclide:sediment:resuspension_depth'),
            resuspension_depth_uncert=g('radionuclide:sediment:resuspension_depth_uncert'),
            resuspension_critvel=g('radionuclide:sediment:resuspension_critvel'))

    def particle_species(self):
        """The species bottom_interaction settles (:925-942)."""
        return [k for k in (self.num_prev, self.num_psrev, self.num_pirrev) if k >= 0]

    # ------------------------------------------------------------------ seeding (:281-315, :349-479)
    def set_init_diameter(self, num, idxs, diam, rng=None):
        """A float64 array of `num` diameters, 0 except at `idxs`: `diam` with the noise of the configured size distribution --
        normal: diam + N(0, uncertainty); lognormal: diam * exp(N(0, 3 uncertainty / diam)); a diameter of 0 gets none (:281-315).
        The reference's clipping to the minimum and maximum diameter assigns into a copy and does nothing: nothing is clipped here.
        rng: a np.random.Generator (the reference's is unseeded)."""
        rng = np.random.default_rng() if rng is None else rng
        sigma = self.get_config('radionuclide:particle_diameter_uncertainty') if diam > 0 else 0.
        out = np.zeros(num)
        if self.get_config('radionuclide:particlesize_distribution') == 'lognormal':
            out[idxs] = diam * rng.lognormal(0., sigma / diam * 3. if diam > 0 else 0., size=len(idxs))
        else:
            out[idxs] = diam + rng.normal(0., sigma, len(idxs))
        return out

    def seed_elements(self, lon, lat, time=None, **kwargs):
        """specie= (a number or one per element) or the fractions LMM_fraction / particle_fraction (defaults seed:*), drawn with
        np.random.rand before the positions as the reference does; diameter= the mean diameter of the particle species."""
        self.check_speciation()
        self.init_species()
        self.init_transfer_rates()
        num_elements = kwargs['number'] if kwargs.get('number') is not None else \
            (np.size(lon) if np.size(lon) > 1 else self.get_config('seed:number'))
        if 'specie' in kwargs:
            init_specie = np.broadcast_to(np.asarray(kwargs.pop('specie'), dtype=int), (num_elements,)).copy()
            particle_frac = kwargs.pop('particle_fraction', None)
            lmm_frac = kwargs.pop('LMM_fraction', None)
        else:
            particle_frac = kwargs.pop('particle_fraction', self.get_config('seed:particle_fraction'))
            lmm_frac = kwargs.pop('LMM_fraction', self.get_config('seed:LMM_fraction'))
            if not lmm_frac + particle_frac == 1.:
                raise ValueError('Illegal specie fraction combination : ' + str(lmm_frac) + ' ' + str(particle_frac))
            # the reference's draws in its order (:396-413): one uniform per element against the LMM fraction, then -- only with a
            # slowly reversible species and seed:slowly_fraction > 0 -- one per remaining element against that fraction
            dissolved = np.random.rand(num_elements) < lmm_frac
            init_specie = np.where(dissolved, self.num_lmmcation if self.num_lmmcation >= 0 else self.num_lmm, self.num_prev)
            slow_frac = self.get_config('seed:slowly_fraction')
            if slow_frac > 0 and self.num_psrev >= 0:
                others = np.flatnonzero(~dissolved)
                init_specie[others[np.random.rand(len(others)) < slow_frac]] = self.num_psrev
        if init_specie.min() < 0 or init_specie.max() >= self.nspecies:
            raise ValueError('specie must be in 0 .. %d (%s)' % (self.nspecies - 1, self.name_species))
        on_bed = init_specie == self.num_srev
        if on_bed.all():
            kwargs['z'] = 'seafloor'
        elif on_bed.any():      # (the reference prints 'SOME ELEMENTS ARE SEDIMENTS' and calls exit())
            raise NotImplementedError('seeding sediment species together with other species is not implemented: the reference '
                                      'exits on it (radionuclides.py:428-430; DESIGN.md section 7g)')
        diameter = kwargs.pop('diameter', None)
        diameter = self.get_config('radionuclide:particle_diameter') if diameter is None else diameter
        # the elements of a species whose name says 'particle', species by species as the reference orders them (:442-446): the
        # order decides which draw of the size distribution an element gets
        is_particle = np.array(['particle' in name.lower() for name in self.name_species])
        particles = np.concatenate([np.flatnonzero(init_specie == k) for k in np.flatnonzero(is_particle)] + [np.empty(0, int)]).astype(int)
        init_diam = self.set_init_diameter(num_elements, particles, diameter, kwargs.pop('diameter_rng', None))
        n_before = 0 if self._sched is None else len(self._sched['lon'])
        super().seed_elements(lon, lat, time, specie=init_specie, diameter=init_diam, **kwargs)
        n_new = len(self._sched['lon']) - n_before
        if n_new != num_elements:      # (a single draw would have been taken for every element)
            raise ValueError('%s elements were seeded, but the species were drawn for %s' % (n_new, num_elements))

    # ------------------------------------------------------------------ concentration maps (:1425-1492, :1518-1551)
    def prepare_run(self):   # :224-225
        self.depthintervals = [float(item) for item in self.get_config('radionuclide:output:depthintervals').split(',')]
        super().prepare_run()

    def get_radionuclide_density_array(self, pixelsize_m, z_array, density_proj=None, llcrnrlon=None, llcrnrlat=None, urcrnrlon=None,
                                       urcrnrlat=None, weight=None, origin_marker=None):
        """radionuclides.py:1425-1492: (H, lon_array, lat_array), H float64 [time, species, layer, x_bin, y_bin] the number of
        elements of each species in each depth layer z_array[zi] < z <= z_array[zi + 1] per pixel of pixelsize_m in density_proj
        (as in get_density_array_proj; None: the reference's '+proj=moll +ellps=WGS84 +lon_0=0.0').  z_array: strictly increasing,
        finite.  The comparisons are made in float64; an element whose z or specie is NaN counts nowhere.  lon_array, lat_array:
        the inverse projection of np.meshgrid(y_array, x_array).

        weight / origin_marker: the reference hands np.histogram2d the whole row of weights with a selection of the positions
        (:1476-1485), which NumPy rejects -- there is nothing to reproduce, so both are refused.

        Without the four corners the extremes are taken on the device over the entries whose projection is finite (the reference's
        x.min() ... need a result without NaN); a sharded run needs the corners.  Projection, classification and binning run on
        the device (odr_species_layer_map)."""
        if weight is not None or origin_marker is not None:
            raise NotImplementedError('get_radionuclide_density_array: weight / origin_marker make the reference pass np.histogram2d a '
                                      'whole row of weights with a selection of the positions (radionuclides.py:1476-1485), which NumPy '
                                      'rejects; counts only')
        result = getattr(self, 'result', None)
        if result is None:
            raise RuntimeError('get_radionuclide_density_array needs the result of run()')
        for name in ('lon', 'lat', 'z', 'specie'):
            if name not in result:
                raise KeyError('%s is not in self.result (export_variables)' % name)
        z_array = np.asarray(z_array, dtype=np.float64).ravel()
        if len(z_array) < 2 or not np.isfinite(z_array).all() or not (np.diff(z_array) > 0).all():
            raise ValueError('get_radionuclide_density_array: z_array must be finite and strictly increasing, at least two values')
        params, x_array, y_array = self._map_grid('get_radionuclide_density_array', pixelsize_m, density_proj,
                                                  '+proj=moll +ellps=WGS84 +lon_0=0.0', (llcrnrlon, llcrnrlat, urcrnrlon, urcrnrlat))
        if len(x_array) < 2 or len(y_array) < 2:
            raise ValueError('get_radionuclide_density_array: %d x %d edges' % (len(x_array), len(y_array)))
        H = self.ctx.species_layer_map(params, result['lon'], result['lat'], result['z'], result['specie'], x_array, y_array, z_array,
                                       self.nspecies)
        lon_array, lat_array = self.ctx.proj_grid_lonlat(params, x_array, y_array)
        return H, lon_array, lat_array

    def horizontal_smooth(self, a, n=0):
        """radionuclides.py:1518-1551: the mean over the (2 n + 1)^2 window of the values of `a` truncated to integers, the plane
        padded with n zeros all round; n == 0 returns `a` itself.  The sums are of integers, so the result is the reference's bit for
        bit.  Beyond the reference's 2-D input, any leading dimensions are accepted (the 5-D H) and the last two are smoothed.  On
        the device (odr_box_smooth)."""
        if n == 0:
            return a
        return self.ctx.box_smooth(a, n)

    # ------------------------------------------------------------------ the run
    def run(self, *args, **kwargs):
        action = self.get_config('general:seafloor_action', 'lift_to_seafloor')
        if action in REFUSED_SEAFLOOR_ACTIONS:      # (before anything is set up on the device)
            raise NotImplementedError("general:seafloor_action = '%s' is not implemented for RadionuclideDrift: a particle would settle "
                                      "below the sea floor (DESIGN.md section 7g); use 'lift_to_seafloor' or 'deactivate'" % action)
        if self.rng == 'numpy' and self.get_config('radionuclide:particlesize_distribution') == 'lognormal' and \
                self.get_config('radionuclide:dissolved_diameter') > 0:
            raise NotImplementedError("radionuclide:particlesize_distribution = 'lognormal' with a dissolved diameter > 0 is not "
                                      "implemented for rng='numpy': one draw per element cannot serve both widths (DESIGN.md section 7g)")
        try:
            return super().run(*args, **kwargs)
        finally:
            self._drop_device_setup()      # (keeps the counters: ntransformations)

    def _setup(self):
        if self._device_setup is None:
            self._device_setup = self.P.radio_setup(**self.setup_members())
        return self._device_setup

    def _with_seafloor_action(self, call):
        # interact_with_seafloor() 'lift_to_seafloor' followed by bottom_interaction() (oceandrift.py:364-368, :556-561): a
        # particle species settles, any other is lifted
        action = self.get_config('general:seafloor_action', 'lift_to_seafloor')
        if action != 'lift_to_seafloor' or 'sea_floor_depth_below_sea_level' not in self.priority_list:
            return super()._with_seafloor_action(call)
        self.ctx.set_seafloor_settle_species(self.aux_properties.index('specie'), self.particle_species())
        call()
        self._resolve_status()

    def bottom_interaction(self, Zmin=None):   # :912-942
        """Nothing to do here: the settling is part of the device's sea-floor check (_with_seafloor_action), the change of species
        part of the resuspension launch."""

    def _host_noise(self, n):
        """rng='numpy': the diameter noise as the reference scales it for the particle diameter (a diameter of 0 takes none)."""
        uncert, diam = self.get_config('radionuclide:particle_diameter_uncertainty'), self.get_config('radionuclide:particle_diameter')
        if self.get_config('radionuclide:particlesize_distribution') == 'lognormal':
            return np.random.lognormal(0., uncert / diam * 3., n)
        return np.random.normal(0., uncert, n)

    def update_speciation(self):   # update_transfer_rates + update_speciation (:728-810)
        n, slot = self.num_elements_active(), self.aux_properties.index
        kw = dict(specie_slot=slot('specie'), diameter_slot=slot('diameter'), step=self.steps_calculation)
        if self.rng == 'numpy':
            kw.update(u1=np.random.random(n), u2=np.random.random(n), diameter_noise=self._host_noise(n),
                      depth_noise=np.random.normal(0, self.get_config('radionuclide:sediment:desorption_depth_uncert'), n))
        self.P.radio_speciation(self._setup(), self.time_step.total_seconds(), **kw)

    def update_terminal_velocity(self, Tprofiles=None, Sprofiles=None, z_index=None):   # :665-721
        if Tprofiles is not None or Sprofiles is not None:
            raise NotImplementedError('temperature / salinity profiles in update_terminal_velocity (DESIGN.md section 7g)')
        if self.num_elements_active() > 0:
            self.P.radio_terminal_velocity(self.aux_properties.index('diameter'), self.aux_properties.index('density'))

    def resuspension(self):   # bottom_interaction's species (:912-942) + resuspension (:946-997)
        n, slot = self.num_elements_active(), self.aux_properties.index
        kw = dict(specie_slot=slot('specie'), diameter_slot=slot('diameter'), step=self.steps_calculation)
        if self.rng == 'numpy':
            kw.update(diameter_noise=self._host_noise(n),
                      depth_noise=np.random.normal(0, self.get_config('radionuclide:sediment:resuspension_depth_uncert'), n))
        self.P.radio_resuspend(self._setup(), **kw)

    def update(self):   # :1004-1038
        if self.num_elements_active() == 0:
            return
        self.update_speciation()
        self.update_terminal_velocity()
        if self.get_config('drift:vertical_mixing') is True:
            self.vertical_mixing()
        else:
            self.vertical_buoyancy()
        self.resuspension()
        self.advect_ocean_current()
        if self.get_config('drift:vertical_advection') is True:
            self.vertical_advection()
