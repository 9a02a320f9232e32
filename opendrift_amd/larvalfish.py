"""LarvalFish on the device path: pelagic eggs that hatch, and larvae that grow and swim up and down with the time of day.

Mirrors opendrift/models/larvalfish.py (Kvile et al. 2018):

  element properties (LarvalFishElement, :31-52): diameter, neutral_buoyancy_salinity, stage_fraction, hatched, length,
  weight, survival -- float32, in the property slots of odr_particles_set_property (include/odrift.h ODR_LARVA_*), carried
  through compaction and sort and recorded in `o.result`.  `hatched` is uint8 in the reference; here it is a float32 slot
  holding 0 (egg) or 1 (larva), like PelagicEggDrift's;
  required_variables with their fallbacks (:69-84: ocean_vertical_diffusivity falls back to 0.01 here), config (:92-103);
  update_terminal_velocity (:105-183) is PelagicEggDrift's line for line = ONE launch (odr_egg_terminal_velocity) with this
  model's slot numbers;
  update_fish_larvae with fish_growth (:185-231) = ONE launch over the active elements (odr_larval_update,
  csrc/odr_larval.hip.h: the reference's float32 operation order);
  larvae_vertical_migration (:233-253) = ONE launch (odr_larval_migrate); the direction comes from `self.time.hour < 12` (UTC,
  as in the reference) on the host, once per step;
  update() = update_fish_larvae -> advect_ocean_current -> stokes_drift -> update_terminal_velocity -> vertical_mixing ->
  larvae_vertical_migration (:255-265).  No wind drift, no vertical advection.

The reference works on float32 arrays where the properties were seeded as arrays; a property left at its scalar default
becomes a float64 array there when the elements are released (elements/elements.py:219-222).  This model holds every property
in the float32 the element type declares.

vertical_mixing:TSprofiles = True is not built: set_config refuses it by name, as for PelagicEggDrift.

rng='numpy' consumes np.random as the reference does: random(n) once per mixing sub-step.  A sharded run needs nothing new: both
kernels are per element and every rank reads the same clock.
"""
from . import _abi
from .config import CONFIG_LEVEL_ADVANCED
from .oceandrift import OceanDrift


class LarvalFish(OceanDrift):
    """opendrift/models/larvalfish.py:55-265 (see the module docstring)."""
    aux_properties = list(_abi.LARVA_PROPERTIES)     # slot order of odr_particles_set_property
    aux_defaults = {'diameter': 0.0014, 'neutral_buoyancy_salinity': 31.25, 'stage_fraction': 0., 'hatched': 0., 'length': 0.,
                    'weight': 0.08, 'survival': 1.}   # :31-52 (NEA cod)
    fuse_vertical_advection = False     # update(): the reference's has no vertical advection at all
    required_variables = {   # larvalfish.py:69-84
        'x_sea_water_velocity': {'fallback': 0},
        'y_sea_water_velocity': {'fallback': 0},
        'sea_surface_height': {'fallback': 0},
        'sea_surface_wave_significant_height': {'fallback': 0},
        'x_wind': {'fallback': 0},
        'y_wind': {'fallback': 0},
        'land_binary_mask': {'fallback': None},
        'sea_floor_depth_below_sea_level': {'fallback': 100},
        'ocean_vertical_diffusivity': {'fallback': 0.01, 'profiles': True},
        'ocean_mixed_layer_thickness': {'fallback': 50},
        'sea_water_temperature': {'fallback': 10, 'profiles': True},
        'sea_water_salinity': {'fallback': 34, 'profiles': True},
        'sea_surface_wave_stokes_drift_x_velocity': {'fallback': 0},
        'sea_surface_wave_stokes_drift_y_velocity': {'fallback': 0},
    }

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._add_config({     # :92-99
            'IBM:fraction_of_timestep_swimming': {'type': 'float', 'default': 0.15, 'min': 0.0, 'max': 1.0, 'units': 'fraction',
                                                  'description': 'Fraction of timestep swimming', 'level': CONFIG_LEVEL_ADVANCED}})
        self._set_config_default('drift:vertical_mixing', True)      # :101-103
        self._set_config_default('drift:vertical_mixing_at_surface', True)
        self._set_config_default('drift:vertical_advection_at_surface', True)

    def update_terminal_velocity(self, Tprofiles=None, Sprofiles=None, z_index=None):   # :105-183
        if Tprofiles is not None or Sprofiles is not None:
            raise NotImplementedError('temperature / salinity profiles in update_terminal_velocity (DESIGN.md section 7d)')
        if self.num_elements_active() > 0:
            self.P.egg_terminal_velocity(self.aux_properties.index('diameter'),
                                         self.aux_properties.index('neutral_buoyancy_salinity'))

    def update_fish_larvae(self):   # :200-231 (the early return without larvae there is logging only)
        if self.num_elements_active() > 0:
            slot = self.aux_properties.index
            self.P.larval_update(self.time_step.total_seconds(), slot('stage_fraction'), slot('hatched'), slot('weight'), slot('length'))

    def larvae_vertical_migration(self):   # :233-253
        if self.num_elements_active() > 0:
            # UTC hours, as in the reference: down while the light is increasing, up while it is decreasing
            direction = -1 if self.time.hour < 12 else 1
            self.P.larval_migrate(self.time_step.total_seconds(), self.get_config('IBM:fraction_of_timestep_swimming'), direction,
                                  self.aux_properties.index('hatched'), self.aux_properties.index('length'))

    def update(self):   # :255-265
        self.update_fish_larvae()
        self.advect_ocean_current()
        self.stokes_drift()
        self.update_terminal_velocity()
        self.vertical_mixing()
        self.larvae_vertical_migration()
