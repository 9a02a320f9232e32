"""ShipDrift on the device path: drift of ships from wind force, wave-drift force, wave damping and form drag.

Mirrors opendrift/models/shipdrift.py (Soergaard & Vada 1998, "Observations and modelling of drifting ships", DnV 96-2011):

  element properties (ShipObject, :32-77): length, height, draft, beam, wind_drag_coeff, water_drag_coeff, orientation --
  float32, in the property slots of odr_particles_set_property (include/odrift.h ODR_SHIP_*), carried through compaction and
  sort and recorded in `o.result`; slot 7 holds the index of the element's class (below).  jibeProbability (0.04 1/h) is
  declared by the reference and never read: it is kept as the constant JIBE_PROBABILITY;
  required_variables with their fallbacks (:89-103), seed:orientation and the default drift:max_speed = 2 (:149-155);
  seed_elements (:157-214): dimensions per element or as scalars, the two range warnings, the wind and water drag coefficients
  from the piecewise formulas (float64, stored float32), orientation left / right / alternating;
  update() (:216-343) = ONE launch, odr_ship_drift (csrc/odr_ship.hip.h): move with the current, wind
  force, wave spectrum and the force / damping integrals, period factors, four damping iterations, move with the drift
  velocity, stranding with the reason 'ship stranded'.  update is the model's own, so run() takes the call-by-call lane.

The wave-force table wforce.dat is data of the reference (shipdrift.py:110-136 reads it from the directory of its own module)
and is not shipped here.  It is looked for, in this order: ShipDrift(wforce=path), the environment variable ODR_WFORCE,
`models/wforce.dat` of an installed `opendrift` package (found without importing it); without one the constructor raises.  The
reference interpolates the table with two scipy.interpolate.LinearNDInterpolator objects (:137-145) -- a Qhull triangulation of
a regular grid, which cannot be derived, only asked.  A ship's clipped ratios (beam / length, draft / length) never change and
the 49 frequencies below 7 are constants of the model, so the interpolators are asked ONCE per class -- a unique pair of the
clipped float32 ratios -- when elements are seeded, and the device reads table[n_classes][49][2].  scipy is imported when the
first table is built; without it that raises ImportError by name.

Two decisions of update() belong to the whole call and are made on the host from the movers' reduction (_wave_modes): where
wave height and period come from (the sampled variable if some element has one > 0, else the wind: physics_methods.py:893-943),
and whether the wave direction is the wind's or the Stokes drift's (:304-313).

The Tm02 wave period has no device id of its own; this model does not require the peak period and carries Tm02 in its slot
on its own device context (Context.slot_aliases, set by ShipDrift.ctx); a reader's peak period is not sampled.  An element whose
period is exactly 0 while others have one (a reader that does not cover it) gets no waves; the reference's replacement by the
mean of the others (physics_methods.py:936-939) is not built.

Not built, refused by name: a sharded run (the two decisions would need a collective), wave or Stokes
variables from ensemble readers.
"""
import logging
import os

import numpy as np

from . import _abi
from .config import CONFIG_LEVEL_ESSENTIAL
from .oceandrift import OceanDrift, OpenDriftSimulation

logger = logging.getLogger(__name__)

TM02 = 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment'
TP = 'sea_surface_wave_period_at_variance_spectral_density_maximum'
HS = 'sea_surface_wave_significant_height'
SX, SY = 'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity'
WAVE_VARIABLES = (HS, TM02, SX, SY)
JIBE_PROBABILITY = 0.04      # ShipObject.jibeProbability [1/h] (:74-76): never read by the reference
DIMENSIONS = {'length': 80., 'height': 8., 'draft': 4., 'beam': 10.}      # ShipObject defaults (:40-67)
NSPEC, OMMIN2, OMMIN3, OMMAX = 100, 2.25, 7.0, 12.0      # update() (:249-253)
DOM = (OMMAX - OMMIN2) / (NSPEC - 1)
OMEGAS = [OMMIN2 + i * DOM for i in range(NSPEC) if OMMIN2 + i * DOM < OMMIN3]      # the frequencies the interpolators are asked at
assert len(OMEGAS) == _abi.SHIP_TABLE_ROWS


def read_wforce(path):
    """Parse a wforce.dat as the reference does (shipdrift.py:110-136).  Kept as it is there: the fill loop runs `ndraft` rows
    of `nbeam` values into F[o, i, :], although the axes are declared (nomega, nbeam, ndraft) -- the table is square."""
    with open(path, 'r') as w:
        w.readline()
        nbeam = int(w.readline().split()[0])
        BL = np.array(w.readline().split()[0:nbeam], dtype=float)
        ndraft = int(w.readline().split()[0])
        DL = np.array(w.readline().split()[0:ndraft], dtype=float)
        nomega = int(w.readline().split()[0])
        omega = np.zeros(nomega)
        F, D = np.zeros((nomega, nbeam, ndraft)), np.zeros((nomega, nbeam, ndraft))
        for o in range(nomega):
            omega[o] = float(w.readline().split()[0])
            for i in range(ndraft):
                F[o, i, :] = w.readline().split()[0:nbeam]
            for i in range(ndraft):
                D[o, i, :] = w.readline().split()[0:nbeam]
    return dict(nbeam=nbeam, BL=BL, ndraft=ndraft, DL=DL, nomega=nomega, omega=omega, F=F, D=D)


def find_wforce(path=None):
    """Path of the wave-force table or None: `path`, $ODR_WFORCE, an installed opendrift's models/wforce.dat."""
    if path is not None:
        return path
    if os.environ.get('ODR_WFORCE'):
        return os.environ['ODR_WFORCE']
    try:
        import importlib.util
        spec = importlib.util.find_spec('opendrift')
    except (ImportError, ValueError):
        spec = None
    for loc in (spec.submodule_search_locations or []) if spec is not None else []:
        cand = os.path.join(loc, 'models', 'wforce.dat')
        if os.path.exists(cand):
            return cand
    return None


def wforce_interpolators(w):
    """The reference's two interpolators (:137-145): same point order (meshgrid(indexing='ij') ravelled), same values."""
    try:
        from scipy.interpolate import LinearNDInterpolator
    except ImportError as e:
        raise ImportError('ShipDrift needs scipy (scipy.interpolate.LinearNDInterpolator) to interpolate the wave-force table '
                          'as the reference does: %s' % e)
    wi_omega, wi_BL, wi_DL = np.meshgrid(w['omega'], w['BL'], w['DL'], indexing='ij')
    points = (wi_omega.ravel(), wi_BL.ravel(), wi_DL.ravel())
    return LinearNDInterpolator(points, w['F'].ravel()), LinearNDInterpolator(points, w['D'].ravel())


def clipped_ratios(length, draft, beam):
    """bl, dl of update() (:220-227) from the float32 element properties: float32, both clips."""
    length, draft, beam = (np.asarray(a, dtype=np.float32) for a in (length, draft, beam))
    dl = draft / length
    bl = beam / length
    bl = np.clip(bl, 0.12, 0.18)
    dl = np.clip(dl, 0.025, 0.07)
    bl = np.clip(bl, 0.121, 0.179)
    dl = np.clip(dl, 0.0251, 0.069)
    return bl, dl


def class_table(interpolators, bl, dl):
    """[len(bl)][49][2] float64: what update() gets from the two interpolators (:276-277) for the float32 ratios bl, dl at each
    of the 49 frequencies, asked as the reference asks (a Python float and two float32 arrays)."""
    bl, dl = np.atleast_1d(np.asarray(bl, np.float32)), np.atleast_1d(np.asarray(dl, np.float32))
    out = np.empty((len(bl), len(OMEGAS), 2))
    for k, omi in enumerate(OMEGAS):
        out[:, k, 0] = interpolators[0](omi, bl, dl)
        out[:, k, 1] = interpolators[1](omi, bl, dl)
    if not np.isfinite(out).all():
        raise ValueError('the wave-force interpolators returned a value that is not finite')
    return out


# water drag coefficient over beta = 2 draft / length (:195-202): straight lines (from beta, Cd there, to beta, Cd there, the
# width as the reference writes it), 1.27 above the last
CD_SEGMENTS = ((0.05, 1.50, 0.06, 1.44, 0.01), (0.06, 1.44, 0.08, 1.38, 0.02), (0.08, 1.38, 0.10, 1.32, 0.02), (0.10, 1.32, 0.12, 1.27, 0.02))


def drag_coefficients(height, draft, length):
    """Cf, Cd of seed_elements (:185-202) from float64 dimensions, each branch in the reference's operation order (the values
    are stored float32 and compared with the reference's bit for bit); dl is clipped only where the reference clips it (:171-177)."""
    dl = draft / length
    if dl.min() < 0.025 or dl.max() > 0.07:
        dl = np.clip(dl, 0.025, 0.07)
    exposed = height - draft
    # wind drag coefficient: two straight lines that meet the constant 1.4 at 37.2 m of exposed height
    Cf = np.where(exposed > 37.2, 1.4, np.where(exposed > 15, 1.045 + 0.016 * (exposed - 15.), 0.700 + 0.023 * exposed))
    beta = 2.0 * dl
    Cd = np.full(len(beta), CD_SEGMENTS[-1][3])
    for x0, y0, x1, y1, width in reversed(CD_SEGMENTS):      # the lower segments overwrite
        Cd = np.where(beta <= x1, y0 + (y1 - y0) / width * (beta - x0), Cd)
    return Cf, Cd


class ShipDrift(OceanDrift):
    """opendrift/models/shipdrift.py:80-343 (see the module docstring)."""
    aux_properties = list(_abi.SHIP_PROPERTIES)     # slot order of odr_particles_set_property
    required_variables = {   # shipdrift.py:89-103
        'x_wind': {'fallback': None},
        'y_wind': {'fallback': None},
        'land_binary_mask': {'fallback': None},
        'x_sea_water_velocity': {'fallback': None},
        'y_sea_water_velocity': {'fallback': None},
        'horizontal_diffusivity': {'fallback': 100, 'important': False},
        SX: {'fallback': 0},
        SY: {'fallback': 0},
        HS: {'fallback': 0},
        TM02: {'fallback': 0},
    }
    winwav_angle = 20      # angular offset in degrees (:105)
    _PROVISIONAL = dict(OpenDriftSimulation._PROVISIONAL, **{'ship stranded': 106})

    def __init__(self, *args, wforce=None, **kwargs):
        from . import distributed as D
        if D.env_world()[2] > 1:      # (before anything of the sharded machinery starts)
            raise NotImplementedError('ShipDrift in a sharded run: where the waves come from and which direction they take are '
                                      'decided for all elements at once and would need a collective (DESIGN.md section 7f)')
        if wforce is not None and not os.path.exists(wforce):
            raise FileNotFoundError(wforce)
        path = find_wforce(wforce)
        if path is None:
            raise FileNotFoundError('ShipDrift needs the reference\'s wave-force table wforce.dat, which is not shipped: pass its '
                                    'path as ShipDrift(wforce=...), set ODR_WFORCE or install opendrift')
        self.wforce = read_wforce(path)
        self._wforce_argument = wforce
        super().__init__(*args, **kwargs)
        self._add_config({'seed:orientation': {      # :149-153
            'type': 'enum', 'enum': ['left', 'right', 'random'], 'default': 'random', 'level': CONFIG_LEVEL_ESSENTIAL,
            'description': 'If ships are oriented to the left or right of the downwind direction, or whether this is unknown. '
                           'Left/right means that wind will hit ship from backboard/steerboard'}})
        limits = {'length': (1, 500), 'height': (1, 100), 'draft': (1, 30), 'beam': (1, 70)}      # :40-67
        self._add_config({'seed:%s' % k: {'type': 'float', 'default': v, 'min': limits[k][0], 'max': limits[k][1], 'units': 'm',
                                          'level': CONFIG_LEVEL_ESSENTIAL, 'description': ''} for k, v in DIMENSIONS.items()})
        self._set_config_default('drift:max_speed', 2)
        self._interpolators = None
        self.ship_classes = []              # (bl, dl) as float32 pairs, in the order of their class index
        self.ship_class_table = None        # [n_classes][49][2]
        self._device_table = None

    def _clone_arguments(self):
        return dict(super()._clone_arguments(), wforce=self._wforce_argument)

    def add_reader(self, readers, variables=None, first=False):
        for r in readers if isinstance(readers, (list, tuple)) else [readers]:
            vs = list(variables or getattr(r, 'variables', ()))
            for v in WAVE_VARIABLES:
                if v in vs and isinstance(getattr(r, 'arrays', {}).get(v), (list, tuple)):
                    raise NotImplementedError('%s from an ensemble reader is not implemented for ShipDrift: the provenance of the '
                                              'waves is decided for all elements at once (DESIGN.md section 7f)' % v)
            if TP in vs:      # not a variable of this model; its device slot carries Tm02
                vs.remove(TP)
                if not vs:    # (an empty list would make the base class take all of the reader's variables)
                    continue
            super().add_reader(r, variables=vs, first=first)

    @property
    def ctx(self):
        """The device context, with the Tm02 wave period riding the peak period's slot ON THIS CONTEXT (Context.slot_aliases):
        this model requires Tm02 and never samples the peak period.  No other model's context resolves the name."""
        c = OpenDriftSimulation.ctx.fget(self)
        c.slot_aliases[TM02] = _abi.VARIABLES[TP]
        return c

    def _class_indices(self, bl, dl):
        """The class index of every (bl, dl); new classes are appended and their tables asked from the interpolators."""
        keys = list(zip(bl.tolist(), dl.tolist()))
        new = sorted(set(keys) - set(self.ship_classes))
        if new:
            if self._interpolators is None:
                self._interpolators = wforce_interpolators(self.wforce)
            t = class_table(self._interpolators, np.array([k[0] for k in new], np.float32), np.array([k[1] for k in new], np.float32))
            self.ship_class_table = t if self.ship_class_table is None else np.concatenate([self.ship_class_table, t])
            self.ship_classes += new
            self._drop_device_table()       # uploaded again by the next update()
        index = {k: i for i, k in enumerate(self.ship_classes)}
        return np.array([index[k] for k in keys], dtype=np.float32)

    def _drop_device_table(self):
        if self._device_table is not None:
            self._device_table.close()
            self._device_table = None

    def seed_elements(self, lon, lat, time=None, **kwargs):
        """length, height, draft, beam as scalars or per-element arrays (defaults from seed:<name>); orientation as an array of
        0 / 1, else by seed:orientation."""
        given = {k: kwargs.pop(k, None) for k in DIMENSIONS}
        orientation = kwargs.pop('orientation', None)
        num = self._seed_number(lon, time, kwargs.get('number'), kwargs.get('number_per_point'))
        dim = {}
        for k, v in given.items():
            v = self.get_config('seed:%s' % k) if v is None else v
            if np.size(v) not in (1, num):
                raise ValueError('%s has length %s, but %s elements were seeded' % (k, np.size(v), num))
            dim[k] = np.atleast_1d(np.asarray(v, dtype=np.float64)) * np.ones(num)
        # Check that beam and height vs length are within expected range (:170-183)
        dl, bl = dim['draft'] / dim['length'], dim['beam'] / dim['length']
        if dl.min() < 0.025 or dl.max() > 0.07:
            logger.warning('Ratio of draft to length should be in range 0.025 to 0.07, given range is %s-%s. Using border value.'
                           % (dl.min(), dl.max()))
        if bl.min() < 0.12 or bl.max() > 0.18:
            logger.warning('Ratio of beam to length should be in range 0.12 to 0.18, given range is %s-%s. Using border value.'
                           % (bl.min(), bl.max()))
        Cf, Cd = drag_coefficients(dim['height'], dim['draft'], dim['length'])
        if orientation is None:      # :204-211
            oc = self.get_config('seed:orientation')
            orientation = np.zeros(num) if oc == 'left' else (np.ones(num) if oc == 'right' else np.r_[:num] % 2)
        elif np.size(orientation) not in (1, num) or not np.isin(orientation, (0, 1)).all():
            raise ValueError('orientation must be 0 or 1 for each of the %s elements seeded' % num)
        props = {k: dim[k].astype(np.float32) for k in DIMENSIONS}
        props.update(wind_drag_coeff=Cf.astype(np.float32), water_drag_coeff=Cd.astype(np.float32),
                     orientation=np.asarray(orientation, dtype=np.float32) * np.ones(num, np.float32))
        props['ship_class'] = self._class_indices(*clipped_ratios(props['length'], props['draft'], props['beam']))
        super().seed_elements(lon, lat, time, **props, **kwargs)

    def _wave_modes(self):
        """(hs_mode, tp_mode, wave_dir_from_stokes) of this step's odr_ship_drift.  Wave height and period: the sampled variable
        where some element has a value > 0, else from the wind (significant_wave_height / wave_period,
        physics_methods.py:893-943; calculate_missing_environment_variables has stored the period to the float32 environment,
        :876-883: tp_mode 3).  Wave direction: the reference takes the wind's when the maxima of BOTH Stokes components are
        exactly 0 (:304-305); the movers' reduction holds the maximum of their float32 SUM, which is 0 under that condition for
        every field but one whose components cancel exactly or are all <= 0 with both maxima 0."""
        iz = self._identically_zero
        if all(iz(v) for v in WAVE_VARIABLES):
            return 1, 3, False
        r = self._reduce_scalars()
        return (0 if r['hs_max'] > 0 else 1), (0 if r['tp_max'] > 0 else 3), bool(r['stokes_sum_max'] != 0)

    def update(self):   # :216-343
        if self.num_elements_active() == 0:
            return
        if self._device_table is None:
            self._device_table = self.P.ship_table(self.ship_class_table)
        hs_mode, tp_mode, from_stokes = self._wave_modes()
        slot = self.aux_properties.index
        # (the class indices were made with the table: no read-back to check them)
        self.P.ship_drift(self.time_step.total_seconds(), self._device_table, hs_mode=hs_mode, tp_mode=tp_mode,
                          wave_dir_from_stokes=from_stokes, stranded_code=self._status_code('ship stranded'),
                          length_slot=slot('length'), height_slot=slot('height'), draft_slot=slot('draft'), beam_slot=slot('beam'),
                          wind_drag_slot=slot('wind_drag_coeff'), water_drag_slot=slot('water_drag_coeff'),
                          orientation_slot=slot('orientation'), class_slot=slot('ship_class'), check_classes=False)
