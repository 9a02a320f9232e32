"""PlastDrift on the device path: marine litter that is moved by the current, the Stokes drift and the wind, and submerged by
the wind.

Mirrors opendrift/models/plastdrift.py:

  element type (PlastElement, :23-29): Lagrangian3DArray with terminal_velocity = 0.01 m/s (positive: rising);
  required_variables with their fallbacks (:44-57), the enum vertical_mixing:mixingmodel ('randomwalk' | 'analytical', default
  'analytical', :66-72) and the changed defaults (:74-78): drift:vertical_mixing, drift:vertical_advection (never called by
  update(), here neither), drift:use_tabularised_stokes_drift, general:coastline_action = 'previous',
  vertical_mixing:diffusivitymodel = 'windspeed_Sundby1983';
  update() (:80-92) = advect_ocean_current -> update_particle_depth -> stokes_drift -> advect_wind: the two movers see the new
  depth;
  update_particle_depth (:94-107): 'randomwalk' is OceanDrift.vertical_mixing; 'analytical' draws the depth of every active element
  anew, z = -np.random.exponential(scale = ocean_vertical_diffusivity / terminal_velocity) -- odr_plast_depth (csrc/odr_plast.hip.h,
  DESIGN.md section 7j).  A sinking element (negative scale) raises ValueError as NumPy does, and no depth has changed.

drift:use_tabularised_stokes_drift is on: without a wave reader the Stokes drift and the wave height come from the wind inside
get_environment (OceanDrift._parameterise_waves).  The coefficients are data of the reference and are not shipped: they are looked
for as stokes_tables.py says (PlastDrift(stokes_tables=...), ODR_STOKES_TABLES, an installed opendrift), and prepare_run() raises
without them.  update() is the model's own and the option needs a launch of its own: run() takes the call-by-call lane.

rng='numpy' consumes np.random as the reference does: standard_exponential(n) once per step ('analytical': np.random.exponential
(scale, n) is scale * standard_exponential(n) and leaves the same generator state).

Not built, refused by name: a sharded run (the option's two decisions are over the elements of all ranks).
"""
import numpy as np

from .config import CONFIG_LEVEL_ADVANCED
from .oceandrift import OceanDrift


class PlastDrift(OceanDrift):
    """opendrift/models/plastdrift.py:32-107 (see the module docstring)."""
    element_properties = dict(OceanDrift.element_properties, terminal_velocity=0.01)      # :23-29
    fuse_vertical_advection = False     # update() never calls vertical_advection(): the mixing launch must not take it along
    required_variables = {   # plastdrift.py:44-57
        'x_sea_water_velocity': {'fallback': 0},
        'y_sea_water_velocity': {'fallback': 0},
        'sea_surface_height': {'fallback': 0},
        'sea_surface_wave_stokes_drift_x_velocity': {'fallback': 0},
        'sea_surface_wave_stokes_drift_y_velocity': {'fallback': 0},
        'sea_surface_wave_significant_height': {'fallback': 0},
        'x_wind': {'fallback': 0},
        'y_wind': {'fallback': 0},
        'ocean_vertical_diffusivity': {'fallback': 0.02, 'profiles': True},
        'ocean_mixed_layer_thickness': {'fallback': 50},
        'sea_floor_depth_below_sea_level': {'fallback': 10000},
        'land_binary_mask': {'fallback': None},
    }

    def __init__(self, *args, **kwargs):
        from . import distributed as D
        if D.env_world()[2] > 1:      # (before anything of the sharded machinery starts)
            raise NotImplementedError('PlastDrift in a sharded run: whether Stokes drift and wave height are derived from the wind '
                                      'is decided over the elements of all ranks and would need a collective (DESIGN.md section 7j)')
        super().__init__(*args, **kwargs)
        self._add_config({'vertical_mixing:mixingmodel': {      # :66-72
            'type': 'enum', 'enum': ['randomwalk', 'analytical'], 'default': 'analytical', 'level': CONFIG_LEVEL_ADVANCED,
            'description': 'How turbulence spreads the elements over depth: a random walk, or a depth drawn anew every step'}})
        self._set_config_default('drift:vertical_mixing', True)      # :74-78
        self._set_config_default('drift:vertical_advection', True)
        self._set_config_default('drift:use_tabularised_stokes_drift', True)
        self._set_config_default('general:coastline_action', 'previous')
        self._set_config_default('vertical_mixing:diffusivitymodel', 'windspeed_Sundby1983')

    def update_particle_depth(self):   # :94-107
        if self.get_config('drift:vertical_mixing') is not True:
            return
        model = self.get_config('vertical_mixing:mixingmodel')
        if model == 'randomwalk':
            self.vertical_mixing()
        if model == 'analytical':
            n = self.num_elements_active()
            if n == 0:
                return
            if self.rng == 'numpy':
                self.P.plast_depth(draws=np.random.standard_exponential(n))
            else:
                self.P.plast_depth(step=self.steps_calculation)

    def update(self):   # :80-92
        self.advect_ocean_current()
        self.update_particle_depth()
        self.stokes_drift()
        self.advect_wind()
