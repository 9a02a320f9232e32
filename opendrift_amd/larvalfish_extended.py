"""LarvalFishExtended on the device path: eggs that hatch after a fixed time, and larvae or phytoplankton that keep a preferred
depth band or migrate between a day depth and a night depth, day and night decided per element by the solar elevation.

Mirrors opendrift/models/larvalfish_extended.py:

  element properties (LarvalFishExtendedElement, :28-41): stage_fraction, hatched -- float32, in the property slots of
  odr_particles_set_property (include/odrift.h ODR_LARVALX_*), carried through compaction and sort and recorded in `o.result`.
  `hatched` is uint8 in the reference; here it is a float32 slot holding 0 (egg) or 1 (larva), like LarvalFish's;
  required_variables with their fallbacks (:73-88), the eleven config keys (:97-167), the three defaults (:169-171);
  update_fish_larvae (:292-318) = ONE launch over the active elements (odr_larvalx_hatch): stage_fraction += float32 of
  (dt / 86400) / egg:hatch_time_days, formed here in float64;
  _apply_vertical_behavior (:206-290) = ONE launch (odr_larvalx_behave, csrc/odr_larvalx.hip.h): the band half-widths
  (_compute_band_half_width, :177-186) and what the solar elevation takes from the time alone (oceandrift.solar_time_scalars) are
  formed here once per step; day or night is decided per element on the device from its own longitude and latitude
  (csrc/odr_solar.hip.h);
  update() = update_fish_larvae (larva only) -> advect_ocean_current -> stokes_drift -> vertical_mixing ->
  _apply_vertical_behavior (:324-342).  No wind drift, no vertical advection, no terminal velocity.

The reference holds z in the float32 its element type declares until the vertical mixing has run and in float64 from then on; the
behaviour step rounds differently in the two (csrc/odr_larvalx.hip.h).  Here z is always float64: with drift:vertical_mixing off
the launch is told to reproduce the float32 roundings.  stage_fraction is held in the float32 the element type declares; the
reference turns a property left at its scalar default into a float64 array (elements/elements.py:219-222).

vertical_mixing:TSprofiles = True is not built: the inherited set_config refuses it by name.

rng='numpy' consumes np.random as the reference does: random(n) once per mixing sub-step.  A sharded run needs nothing new: both
kernels are per element and every rank reads the same clock.
"""
import numpy as np

from . import _abi
from .config import CONFIG_LEVEL_ADVANCED, CONFIG_LEVEL_BASIC, CONFIG_LEVEL_ESSENTIAL
from .oceandrift import OceanDrift, solar_time_scalars


class LarvalFishExtended(OceanDrift):
    """opendrift/models/larvalfish_extended.py:44-342 (see the module docstring)."""
    aux_properties = list(_abi.LARVALX_PROPERTIES)     # slot order of odr_particles_set_property
    aux_defaults = {'stage_fraction': 0., 'hatched': 0.}   # :34-41
    fuse_vertical_advection = False     # update(): the reference's has no vertical advection at all
    required_variables = {   # larvalfish_extended.py:73-88
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
        self._add_config({     # :97-167
            'biology:particle_type': {'type': 'enum', 'enum': ['larva', 'phytoplankton'], 'default': 'larva', 'level': CONFIG_LEVEL_ESSENTIAL,
                                      'description': 'Larvae have egg and hatching stages. Phytoplankton only use vertical behavior.'},
            'biology:vertical_behavior_mode': {'type': 'enum', 'enum': ['none', 'depth', 'dvm'], 'default': 'dvm', 'level': CONFIG_LEVEL_ESSENTIAL,
                                               'description': 'none: no active movement. depth: keep a preferred depth band. '
                                                              'dvm: diel vertical migration between a day and a night depth.'},
            'biology:w_active': {'type': 'float', 'default': 0.003, 'min': 0.0, 'max': 1.0, 'units': 'm/s', 'level': CONFIG_LEVEL_BASIC,
                                 'description': 'Maximum active vertical positioning speed.'},
            'biology:z_pref': {'type': 'float', 'default': -10.0, 'min': -10000, 'max': 0.0, 'units': 'm', 'level': CONFIG_LEVEL_BASIC,
                               'description': 'Preferred depth for depth mode (negative down from the surface).'},
            'biology:z_day': {'type': 'float', 'default': -25.0, 'min': -10000, 'max': 0.0, 'units': 'm', 'level': CONFIG_LEVEL_BASIC,
                              'description': 'Target depth during daytime for dvm mode.'},
            'biology:z_night': {'type': 'float', 'default': -5.0, 'min': -10000, 'max': 0.0, 'units': 'm', 'level': CONFIG_LEVEL_BASIC,
                                'description': 'Target depth during nighttime for dvm mode.'},
            'biology:dz_min': {'type': 'float', 'default': 1.0, 'min': 0.1, 'max': 100, 'units': 'm', 'level': CONFIG_LEVEL_ADVANCED,
                               'description': 'Minimum half-width of a depth band.'},
            'biology:dz_rel': {'type': 'float', 'default': 0.1, 'min': 0.0, 'max': 1.0, 'units': 'fraction', 'level': CONFIG_LEVEL_ADVANCED,
                               'description': 'Half-width of a depth band as a fraction of its depth.'},
            'biology:dz_max': {'type': 'float', 'default': 15.0, 'min': 0.1, 'max': 1000, 'units': 'm', 'level': CONFIG_LEVEL_ADVANCED,
                               'description': 'Maximum half-width of a depth band.'},
            'egg:hatching_method': {'type': 'enum', 'enum': ['fixed_time'], 'default': 'fixed_time', 'level': CONFIG_LEVEL_BASIC,
                                    'description': 'fixed_time: hatch after a fixed duration.'},
            'egg:hatch_time_days': {'type': 'float', 'default': 2.0, 'min': 0.004, 'max': 416, 'units': 'days', 'level': CONFIG_LEVEL_BASIC,
                                    'description': 'Time to hatching when hatching_method is fixed_time.'},
        })
        self._set_config_default('drift:vertical_mixing', True)      # :169-171
        self._set_config_default('drift:vertical_mixing_at_surface', True)
        self._set_config_default('drift:vertical_advection_at_surface', True)

    def _compute_band_half_width(self, z):   # :177-186
        dz = self.get_config('biology:dz_rel') * np.abs(z)
        dz = np.maximum(dz, self.get_config('biology:dz_min'))
        return float(np.minimum(dz, self.get_config('biology:dz_max')))

    def update_fish_larvae(self):   # :292-318 (the early return without larvae there is logging only)
        if self.num_elements_active() > 0:
            days_in_timestep = self.time_step.total_seconds() / 86400
            self.P.larvalx_hatch(days_in_timestep / self.get_config('egg:hatch_time_days'), self.aux_properties.index('stage_fraction'),
                                 self.aux_properties.index('hatched'))

    def _apply_vertical_behavior(self):   # :206-290
        behavior = self.get_config('biology:vertical_behavior_mode')
        if behavior == 'none' or self.num_elements_active() == 0:
            return
        dt, w_active = self.time_step.total_seconds(), self.get_config('biology:w_active')
        if w_active <= 0.0 or dt <= 0.0:
            return
        kw = dict(active_only_hatched=self.get_config('biology:particle_type') == 'larva',
                  z_is_float32=self.get_config('drift:vertical_mixing') is False, hatched_slot=self.aux_properties.index('hatched'))
        if behavior == 'depth':
            z_pref = self.get_config('biology:z_pref')
            self.P.larvalx_behave('depth', dt, w_active, (z_pref, self._compute_band_half_width(z_pref)), **kw)
        else:
            z_day, z_night = self.get_config('biology:z_day'), self.get_config('biology:z_night')
            self.P.larvalx_behave('dvm', dt, w_active, (z_night, self._compute_band_half_width(z_night)),
                                  (z_day, self._compute_band_half_width(z_day)), solar_time_scalars(self.time), **kw)

    def update(self):   # :324-342
        if self.get_config('biology:particle_type') == 'larva':
            self.update_fish_larvae()
        self.advect_ocean_current()
        self.stokes_drift()
        self.vertical_mixing()
        self._apply_vertical_behavior()
