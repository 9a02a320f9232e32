"""PelagicEggDrift on the device path: buoyant particles (fish eggs) whose terminal velocity follows from the temperature and
salinity of the water around them.

Mirrors opendrift/models/pelagicegg.py:

  element properties (PelagicEgg, :26-42): diameter, neutral_buoyancy_salinity, density, hatched -- float32, in the property
  slots of odr_particles_set_property (include/odrift.h ODR_EGG_*), carried through compaction and sort and recorded in
  `o.result`;
  required_variables with their fallbacks (:60-79), config defaults (:92-98);
  update_terminal_velocity (:100-179; Sundby 1983) = ONE launch over the active elements (odr_egg_terminal_velocity,
  csrc/odr_egg.hip.h: the reference's float32 operation order);
  update() = terminal velocity -> vertical_mixing -> advect_ocean_current -> vertical_advection (:181-193): the
  Runge-Kutta stages of the current sample at the mixed depth.  No wind drift, no Stokes drift.

The reference calls update_terminal_velocity again at the top of every mixing sub-step (oceandrift.py:509).  Without
vertical_mixing:TSprofiles it reads the same environment every time, so one launch per step gives the same values.
vertical_mixing:TSprofiles = True (temperature and salinity columns interpolated to the element's depth in every sub-step)
is not built: set_config refuses it by name.

Four of the reference's required variables have no device id and nothing in the reference's model reads them:
surface_downward_x_stress, surface_downward_y_stress, turbulent_kinetic_energy, turbulent_generic_length_scale.  Their
environment:fallback:* / environment:constant:* keys exist and a reader that offers them is accepted, but they are neither
sampled nor exported: `o.required_variables` of an instance holds the fourteen sampled names, the class attribute all
eighteen.

rng='numpy' consumes np.random as the reference does: random(n) once per mixing sub-step.
"""
from . import _abi
from .oceandrift import OceanDrift

# required by the reference's class, read by nothing in it, and without a device variable id
UNSAMPLED_VARIABLES = ('surface_downward_x_stress', 'surface_downward_y_stress', 'turbulent_kinetic_energy',
                       'turbulent_generic_length_scale')


class PelagicEggDrift(OceanDrift):
    """opendrift/models/pelagicegg.py:45-193 (see the module docstring: four required variables are accepted, not sampled)."""
    aux_properties = list(_abi.EGG_PROPERTIES)     # slot order of odr_particles_set_property
    aux_defaults = {'diameter': 0.0014, 'neutral_buoyancy_salinity': 31.25, 'density': 1028., 'hatched': 0.}   # :30-42 (NEA cod)
    fuse_vertical_advection = False     # update(): the current advection lies between the mixing and the vertical advection
    required_variables = {   # pelagicegg.py:60-79
        'x_sea_water_velocity': {'fallback': 0},
        'y_sea_water_velocity': {'fallback': 0},
        'sea_surface_height': {'fallback': 0},
        'sea_surface_wave_significant_height': {'fallback': 0},
        'sea_ice_area_fraction': {'fallback': 0},
        'x_wind': {'fallback': 0},
        'y_wind': {'fallback': 0},
        'land_binary_mask': {'fallback': None},
        'sea_floor_depth_below_sea_level': {'fallback': 100},
        'ocean_vertical_diffusivity': {'fallback': 0.02, 'profiles': True},
        'ocean_mixed_layer_thickness': {'fallback': 50},
        'sea_water_temperature': {'fallback': 10, 'profiles': True},
        'sea_water_salinity': {'fallback': 34, 'profiles': True},
        'surface_downward_x_stress': {'fallback': 0},
        'surface_downward_y_stress': {'fallback': 0},
        'turbulent_kinetic_energy': {'fallback': 0},
        'turbulent_generic_length_scale': {'fallback': 0},
        'upward_sea_water_velocity': {'fallback': 0},
    }

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)       # (config keys for all eighteen variables)
        for v in UNSAMPLED_VARIABLES:
            self.required_variables.pop(v)
        self._set_config_default('general:coastline_action', 'previous')      # :92-98
        self._set_config_default('drift:vertical_mixing', True)
        self._set_config_default('drift:vertical_mixing_at_surface', True)
        self._set_config_default('drift:vertical_advection_at_surface', True)

    def add_reader(self, readers, variables=None, first=False):
        if not isinstance(readers, (list, tuple)):
            readers = [readers]
        for r in readers:
            if not (hasattr(r, 'get_variables') and hasattr(r, 'variables')):
                raise TypeError('Please provide Reader object')
            super().add_reader(r, [v for v in (variables or r.variables) if v not in UNSAMPLED_VARIABLES], first)

    def update_terminal_velocity(self, Tprofiles=None, Sprofiles=None, z_index=None):   # :100-179
        if Tprofiles is not None or Sprofiles is not None:
            raise NotImplementedError('temperature / salinity profiles in update_terminal_velocity (DESIGN.md section 7b)')
        if self.num_elements_active() > 0:
            self.P.egg_terminal_velocity(self.aux_properties.index('diameter'),
                                         self.aux_properties.index('neutral_buoyancy_salinity'))

    def update(self):   # :181-193
        self.update_terminal_velocity()
        self.vertical_mixing()
        self.advect_ocean_current()
        if self.get_config('drift:vertical_advection') is True:
            self.vertical_advection()
