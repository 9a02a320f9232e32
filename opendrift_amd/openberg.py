"""OpenBerg on the device path: iceberg drift from ocean and wind drag, wave radiation, Coriolis and sea ice.

Mirrors opendrift/models/openberg.py (Keghouche et al. 2010):

  element properties (IcebergObj, :45-100): sail, draft, length, width, iceb_x_velocity, iceb_y_velocity -- float32, in the
  property slots of odr_particles_set_property (include/odrift.h ODR_BERG_*), carried through compaction and sort and recorded
  in `o.result`.  The six coefficients (weight_coef, the four drag coefficients, wave_drag_coef) are scalars of the run: the
  reference holds them as float64 arrays of ONE float32 value each when they are seeded as scalars (elements/elements.py:219-222);
  required_variables with their fallbacks (:297-321), the eleven config keys (:357-424);
  roll_over (:587-614) = ONE launch over the active elements (odr_berg_roll_over);
  advect_iceberg (:427-552) = odr_berg_advect: a prepare launch (the factors of the forces, V0, grounding and degrounding), SciPy's
  RK45 over the velocity vector of the whole active set with one launch and one 8-byte read-back per attempt, and a finish
  launch (positions along the geodesic, the two velocity properties) -- csrc/odr_berg.hip.h, DESIGN.md section 7e;
  update() = roll_over -> melt -> advect_iceberg (:616-620).  Elements stay at z = 0.

Not built, refused by name: processes:melting (needs temperature and salinity columns),
drift:vertical_profile (needs current columns), drift:sea_surface_slope (its variables have no id), coefficients that differ between
elements, a reader for sea_surface_wave_from_direction or sea_ice_thickness (both are scalars of the call: set them with
environment:constant: or leave the fallback), and a sharded run (the error norm would need a collective per attempt).
"""
import numpy as np

from . import _abi
from .config import CONFIG_LEVEL_BASIC, CONFIG_LEVEL_ESSENTIAL
from .oceandrift import OceanDrift

COEFFICIENTS = {'weight_coef': 1.0, 'water_form_drag_coef': 0.25, 'water_skin_drag_coef': 0.0055, 'wind_form_drag_coef': 0.8,
                'wind_skin_drag_coef': 0.0022, 'wave_drag_coef': 0.3}      # IcebergObj (:76-93)
SCALAR_VARIABLES = ('sea_surface_wave_from_direction', 'sea_ice_thickness')      # no variable id: scalars of odr_berg_advect
UNSAMPLED_VARIABLES = SCALAR_VARIABLES + ('sea_surface_x_slope', 'sea_surface_y_slope', 'sea_water_temperature', 'sea_water_salinity')


class OpenBerg(OceanDrift):
    """opendrift/models/openberg.py:293-620 (see the module docstring)."""
    aux_properties = list(_abi.BERG_PROPERTIES)     # slot order of odr_particles_set_property
    aux_defaults = {'sail': 10., 'draft': 90., 'length': 100., 'width': 30., 'iceb_x_velocity': 0., 'iceb_y_velocity': 0.}   # :48-99
    required_variables = {   # openberg.py:297-321
        'x_sea_water_velocity': {'fallback': None, 'profiles': True},
        'y_sea_water_velocity': {'fallback': None, 'profiles': True},
        'sea_floor_depth_below_sea_level': {'fallback': 10000},
        'sea_surface_height': {'fallback': 0, 'important': False},
        'sea_surface_x_slope': {'fallback': 0, 'important': False},
        'sea_surface_y_slope': {'fallback': 0, 'important': False},
        'x_wind': {'fallback': None},
        'y_wind': {'fallback': None},
        'horizontal_diffusivity': {'fallback': 100, 'important': False},
        'sea_surface_wave_significant_height': {'fallback': 0},
        'sea_surface_wave_from_direction': {'fallback': 0},
        'sea_surface_wave_stokes_drift_x_velocity': {'fallback': 0, 'important': False},
        'sea_surface_wave_stokes_drift_y_velocity': {'fallback': 0, 'important': False},
        'sea_water_temperature': {'fallback': 2, 'profiles': True, 'important': False},
        'sea_water_salinity': {'fallback': 35, 'profiles': True, 'important': False},
        'sea_ice_area_fraction': {'fallback': 0, 'important': False},
        'sea_ice_thickness': {'fallback': 0, 'important': False},
        'sea_ice_x_velocity': {'fallback': 0, 'important': False},
        'sea_ice_y_velocity': {'fallback': 0, 'important': False},
        'land_binary_mask': {'fallback': None},
    }
    REFUSED = {'processes:melting': 'needs temperature and salinity columns', 'drift:vertical_profile': 'needs current columns',
               'drift:sea_surface_slope': 'sea_surface_x_slope / sea_surface_y_slope have no variable id'}

    def __init__(self, *args, **kwargs):
        from . import distributed as D
        if D.env_world()[2] > 1:      # (before anything of the sharded machinery starts)
            raise NotImplementedError('OpenBerg in a sharded run: the error norm of the solver would need a collective per attempt '
                                      '(DESIGN.md section 7e)')
        super().__init__(*args, **kwargs)
        # what the device samples: the variables the default configuration reads.  The others keep their environment:constant: /
        # environment:fallback: keys (made by OceanDrift.__init__ from the full table above)
        for v in UNSAMPLED_VARIABLES:
            self.required_variables.pop(v)
        for v in ('x_sea_water_velocity', 'y_sea_water_velocity'):
            self.required_variables[v].pop('profiles')
        b = lambda default, text: {'type': 'bool', 'default': default, 'description': text, 'level': CONFIG_LEVEL_BASIC}      # noqa: E731
        self._add_config({     # :357-424
            'drift:wave_rad': b(True, 'If True, wave radiation force is added'),
            'drift:stokes_drift': b(False, 'If True, stokes drift force is added'),
            'drift:coriolis': b(True, 'If True, coriolis force is added'),
            'drift:sea_surface_slope': b(False, 'If True, sea surface slope force is added'),
            'drift:vertical_profile': b(False, 'If True, depth integrated currents are applied'),
            'processes:grounding': b(True, 'If True, grounding is enabled'),
            'processes:roll_over': b(True, 'If True, roll over is enabled'),
            'processes:melting': b(False, 'If True, melting is enabled'),
            'melting:wave': b(True, 'If True, melting due to wave erosion is enabled'),
            'melting:lateral': b(True, 'If True, lateral melting is enabled'),
            'melting:basal': b(True, 'If True, basal melting is enabled')}, overwrite=True)      # (drift:stokes_drift is OceanDrift's too: off here)
        self._add_config({'seed:%s' % k: {'type': 'float', 'default': v, 'min': -1e12, 'max': 1e12, 'level': CONFIG_LEVEL_ESSENTIAL, 'description': ''}
                          for k, v in COEFFICIENTS.items()})
        self.coefficients = None      # fixed by the first seed_elements
        self.solver_attempts = []     # (attempts, rejected attempts) of every advect_iceberg
        self._lat_is_float32 = True   # set where run() starts

    def set_config(self, key, value):
        if key in self.REFUSED and value:
            raise NotImplementedError('%s = True is not implemented for OpenBerg: it %s (DESIGN.md section 7e)' % (key, self.REFUSED[key]))
        super().set_config(key, value)

    def add_reader(self, readers, variables=None, first=False):
        for r in readers if isinstance(readers, (list, tuple)) else [readers]:
            for v in SCALAR_VARIABLES:
                if v in (variables or getattr(r, 'variables', ())):
                    raise NotImplementedError('%s from a reader is not implemented for OpenBerg: it is a scalar of the run, set '
                                              'environment:constant:%s or leave the fallback (DESIGN.md section 7e)' % (v, v))
        super().add_reader(readers, variables=variables, first=first)

    def seed_elements(self, lon, lat, time=None, **kwargs):
        """sail, draft, length and width as scalars or per-element arrays (defaults from seed:<name>); the six coefficients as
        scalars, the same in every call."""
        coef = {}
        for k in COEFFICIENTS:
            v = kwargs.pop(k, None)
            v = self.get_config('seed:%s' % k) if v is None else v
            if np.size(v) != 1 and len(np.unique(np.asarray(v, np.float32))) != 1:
                raise NotImplementedError('%s with values that differ between elements is not implemented for OpenBerg: the '
                                          'coefficients are scalars of the run (DESIGN.md section 7e)' % k)
            coef[k] = float(np.float32(np.ravel(v)[0]))      # (IcebergObj declares them float32)
        if self.coefficients is not None and coef != self.coefficients:
            k = [k for k in coef if coef[k] != self.coefficients[k]][0]
            raise NotImplementedError('%s differs from an earlier seed_elements call: the coefficients are scalars of the run '
                                      '(DESIGN.md section 7e)' % k)
        super().seed_elements(lon, lat, time, **kwargs)
        self.coefficients = coef

    def run(self, *args, **kwargs):
        # a run that starts from seeded elements starts from float32 latitudes again (as f32_first of OceanDrift.run)
        self._lat_is_float32 = self.steps_calculation == 0
        return super().run(*args, **kwargs)

    def _scalar_variable(self, v):
        c = self.get_config('environment:constant:%s' % v)
        return float(self.get_config('environment:fallback:%s' % v) if c is None else c)

    def roll_over(self):   # :587-614
        if self.get_config('processes:roll_over') is False or self.num_elements_active() == 0:
            return
        slot = self.aux_properties.index
        self.P.berg_roll_over(slot('sail'), slot('draft'), slot('length'), slot('width'))

    def melt(self):   # :555-584: processes:melting = True is refused by set_config
        return

    def advect_iceberg(self):   # :427-552
        if self.num_elements_active() == 0:
            return
        slot = self.aux_properties.index
        # until the first update_positions of a run the reference's elements.lat is a float32 array (elements.py:71-88) and its
        # Coriolis parameter a float32 value
        self.solver_attempts.append(self.P.berg_advect(
            self.time_step.total_seconds(), wave_from_direction=self._scalar_variable('sea_surface_wave_from_direction'),
            sea_ice_thickness=self._scalar_variable('sea_ice_thickness'), wave_rad=self.get_config('drift:wave_rad'),
            stokes_drift=self.get_config('drift:stokes_drift'), coriolis=self.get_config('drift:coriolis'),
            grounding=self.get_config('processes:grounding'), lat_is_float32=self._lat_is_float32,
            sail_slot=slot('sail'), draft_slot=slot('draft'), length_slot=slot('length'), width_slot=slot('width'),
            x_velocity_slot=slot('iceb_x_velocity'), y_velocity_slot=slot('iceb_y_velocity'), **self.coefficients))
        self._lat_is_float32 = False

    def update(self):   # :616-620
        self.roll_over()
        self.melt()
        self.advect_iceberg()
