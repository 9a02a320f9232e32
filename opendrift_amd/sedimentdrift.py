"""SedimentDrift on the device path: sinking particles that settle on the sea floor and are resuspended where the current is
fast enough.

Mirrors opendrift/models/sedimentdrift.py:

  element properties (SedimentElement, :28-36): terminal_velocity (default -0.001 m/s, seed:terminal_velocity) and `settled`,
  which the reference declares and never writes -- carried here as a float32 property (slot 0, default 0) and recorded in
  `o.result`; the state of an element is elements.moving (0: settled);
  required_variables with their fallbacks (:45-61), config (:69-86);
  update() (:88-106) = current -> vertical advection -> wind -> Stokes drift -> vertical mixing -> resuspension, on the
  call-by-call lane of run();
  bottom_interaction (:108-116): INSIDE the device's sea-floor check of the mixing sub-steps and of vertical_buoyancy
  (ODR_SEAFLOOR_SETTLE, include/odrift.h): an element below the sea floor is lifted onto it and gets moving = 0;
  resuspension (:118-126) = ONE launch over the active elements (odr_resuspend, csrc/odr_sediment.hip.h).

The reference's hook settles every moving element with z <= Zmin in a sub-step in which some element is below the floor; the
device settles the elements that were below.  The two differ only for a moving element that lies exactly on Zmin without
having been below (needs K == 0 and terminal_velocity == 0 together): DESIGN.md section 7c.

general:seafloor_action 'none' and 'previous' leave the element below the floor, where the reference's hook would settle it
without lifting it: not built, run() refuses both by name.  'deactivate' needs nothing: deactivate_elements has set
moving = 0 before the hook looks (basemodel/__init__.py:1790).

sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment has no device id.  The reference's
wave_period() prefers it to the peak period when it is not 0 (physics_methods.py:918-923): with the value 0 -- no reader, no
constant, the fallback of 0 -- it changes nothing and is dropped from the instance's sampled variables; a reader that offers it
or a non-zero constant / fallback raises NotImplementedError.

rng='numpy' consumes np.random as the reference does: random(n) once per mixing sub-step.  A sharded run needs nothing new:
settling and resuspension are per element, no global reduction.
"""
from .config import CONFIG_LEVEL_ESSENTIAL
from .oceandrift import OceanDrift

TM02 = 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'
REFUSED_SEAFLOOR_ACTIONS = ('none', 'previous')


class SedimentDrift(OceanDrift):
    """opendrift/models/sedimentdrift.py:39-126 (see the module docstring)."""
    aux_properties = ['settled']      # slot order of odr_particles_set_property; seeded from seed:settled (:30-32)
    fuse_vertical_advection = False     # update(): the vertical advection comes BEFORE the mixing
    element_properties = dict(OceanDrift.element_properties, terminal_velocity=-0.001)   # :33-35: 1 mm/s negative buoyancy
    required_variables = {   # sedimentdrift.py:45-61
        'x_sea_water_velocity': {'fallback': 0},
        'y_sea_water_velocity': {'fallback': 0},
        'sea_surface_height': {'fallback': 0},
        'upward_sea_water_velocity': {'fallback': 0},
        'x_wind': {'fallback': 0},
        'y_wind': {'fallback': 0},
        'sea_surface_wave_stokes_drift_x_velocity': {'fallback': 0},
        'sea_surface_wave_stokes_drift_y_velocity': {'fallback': 0},
        'sea_surface_wave_period_at_variance_spectral_density_maximum': {'fallback': 0},
        TM02: {'fallback': 0},
        'land_binary_mask': {'fallback': None},
        'ocean_vertical_diffusivity': {'fallback': 0.02, 'profiles': True},
        'ocean_mixed_layer_thickness': {'fallback': 50},
        'sea_floor_depth_below_sea_level': {'fallback': 10000},
    }

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)       # (config keys for all fourteen variables)
        self.required_variables.pop(TM02)
        self._add_config({
            'vertical_mixing:resuspension_threshold': {     # :69-79
                'type': 'float', 'default': 0.2, 'min': 0, 'max': 3, 'units': 'm/s', 'level': CONFIG_LEVEL_ESSENTIAL,
                'description': 'Sedimented particles will be resuspended if bottom current shear exceeds this value.'},
            'seed:settled': {'type': 'float', 'default': 0., 'min': 0, 'max': 1, 'level': CONFIG_LEVEL_ESSENTIAL, 'description': ''}})
        self._set_config_default('general:coastline_action', 'previous')      # :81-86
        self._set_config_default('drift:vertical_mixing', True)

    def set_config(self, key, value):
        if key in ('environment:constant:' + TM02, 'environment:fallback:' + TM02) and value:
            raise NotImplementedError('%s has no device variable: only the value 0 is supported (DESIGN.md section 7c)' % TM02)
        super().set_config(key, value)

    def add_reader(self, readers, variables=None, first=False):
        for r in readers if isinstance(readers, (list, tuple)) else [readers]:
            if hasattr(r, 'variables') and TM02 in (variables or r.variables):
                raise NotImplementedError('%s has no device variable: a reader that offers it is not supported '
                                          '(DESIGN.md section 7c)' % TM02)
        super().add_reader(readers, variables, first)

    def run(self, *args, **kwargs):
        action = self.get_config('general:seafloor_action', 'lift_to_seafloor')
        if action in REFUSED_SEAFLOOR_ACTIONS:      # (before anything is set up on the device)
            raise NotImplementedError("general:seafloor_action = '%s' is not implemented for SedimentDrift: the element would settle "
                                      "below the sea floor (DESIGN.md section 7c); use 'lift_to_seafloor' or 'deactivate'" % action)
        return super().run(*args, **kwargs)

    def _seafloor_action_in_update(self, action):
        # interact_with_seafloor() 'lift_to_seafloor' followed by bottom_interaction() (oceandrift.py:364-368, :556-561)
        return 'settle' if action == 'lift_to_seafloor' else action

    def bottom_interaction(self, Zmin=None):   # :108-116
        """Nothing to do here: the settling is part of the device's sea-floor check (_seafloor_action_in_update)."""

    def resuspension(self):   # :118-126
        if self.num_elements_active() > 0:
            self.P.resuspend(self.get_config('vertical_mixing:resuspension_threshold'), count=False)

    def update(self):   # :88-106
        self.advect_ocean_current()
        self.vertical_advection()
        self.advect_wind()
        self.stokes_drift()
        self.vertical_mixing()
        self.resuspension()
