"""The coefficients behind drift:use_tabularised_stokes_drift.

The reference fits polynomials to two tables of its own (surface Stokes drift per wind speed and significant wave height per wind
speed, for fetches of 5, 25 and 50 km: physics_methods.py:488-568) with np.polyfit and evaluates them with np.polyval.  Tables
and fit are data of the reference and are not shipped here: the fitted coefficients are looked for, in this order,

  1. the `stokes_tables=` argument of the model's constructor or of set_stokes_tables(): a dict, or the path of a file;
  2. the environment variable ODR_STOKES_TABLES: the path of a file;
  3. an installed `opendrift`: its two functions are called once with a zero wind and the coefficients they fitted are read back
     from its module.

A file is JSON, {"<fetch>": {"stokes": [...], "hs": [...]}, ...}, or an .npz with the arrays stokes_<fetch> and hs_<fetch>;
coefficients lead with the highest power, as np.polyfit returns them.  tests/golden/stokes_tables.json is such a file, written by
tools/gen_golden_plastdrift.py from the reference's own functions.
"""
import json
import os

import numpy as np

FETCHES = ('5000', '25000', '50000')
MAX_STOKES_COEFFICIENTS = 7        # a launch argument of odr_stokes_from_wind
ENV = 'ODR_STOKES_TABLES'
MISSING = ('drift:use_tabularised_stokes_drift needs the polynomial coefficients the reference fits to its Stokes drift and wave '
           'height tables, which are not shipped: pass stokes_tables= (a dict or the path of a JSON / npz file) to the constructor '
           'or to set_stokes_tables(), set %s to such a path, or install opendrift' % ENV)


def _checked(tables, where):
    out = {}
    for fetch, t in tables.items():
        try:
            stokes, hs = np.array(t['stokes'], dtype=np.float64), np.array(t['hs'], dtype=np.float64)
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError('%s: fetch %r needs the lists "stokes" and "hs" (%s)' % (where, fetch, e))
        if stokes.ndim != 1 or not 1 <= len(stokes) <= MAX_STOKES_COEFFICIENTS or hs.shape != (2,) or \
                not (np.isfinite(stokes).all() and np.isfinite(hs).all()):
            raise ValueError('%s: fetch %r needs 1 .. %d finite coefficients of the drift factor and 2 of the wave height'
                             % (where, fetch, MAX_STOKES_COEFFICIENTS))
        out[str(fetch)] = {'stokes': stokes, 'hs': hs}
    if not out:
        raise ValueError('%s holds no fetch' % where)
    return out


def load(source):
    """The tables of a dict or of a JSON / npz file, checked: {fetch: {'stokes': float64[1..7], 'hs': float64[2]}}."""
    if isinstance(source, dict):
        return _checked(source, 'stokes_tables')
    path = os.fspath(source)
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    if path.endswith('.npz'):
        with np.load(path) as f:
            fetches = sorted(k[len('stokes_'):] for k in f.files if k.startswith('stokes_'))
            return _checked({k: {'stokes': f['stokes_' + k], 'hs': f['hs_' + k]} for k in fetches}, path)
    with open(path) as fh:
        return _checked(json.load(fh), path)


def from_installed_reference():
    """The coefficients an installed opendrift fits, or None without one."""
    try:
        from opendrift.models import physics_methods as pm
    except ImportError:
        return None
    zero = (np.zeros(1, np.float32), np.zeros(1, np.float32))
    pm.wave_stokes_drift_parameterised(zero, FETCHES[0])         # (the first call fits every fetch)
    pm.wave_significant_height_parameterised(zero, FETCHES[0])
    stokes, hs = getattr(pm, '__stokes_coefficients__'), getattr(pm, '__stokes_hs_coefficients__')
    return _checked({f: {'stokes': stokes[f], 'hs': hs[f]} for f in FETCHES}, 'the installed opendrift')


def find(argument=None):
    """(tables, where they came from) by the order of the module docstring, or (None, None)."""
    if argument is not None:
        return load(argument), 'argument'
    if os.environ.get(ENV):
        return load(os.environ[ENV]), ENV
    t = from_installed_reference()
    return (t, 'opendrift') if t is not None else (None, None)
