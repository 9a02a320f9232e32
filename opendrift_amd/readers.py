"""Reader plugin surface -- host side.

Same contract as the reference's readers (opendrift/readers/basereader/): a reader sets
`proj4`, `xmin/xmax/ymin/ymax`, `variables`, `start_time/end_time/time_step` (or `times`),
optionally `z`, and implements

    get_variables(requested_variables, time=None, x=None, y=None, z=None) -> dict

returning, for a StructuredReader, one block {'x','y','z','time', var: [ny,nx] | [nz,ny,nx]}
(basereader/structured.py:125-147), or, for a ContinuousReader, arrays at the exact positions
(basereader/continuous.py:20-29).  `get_variables` stays on the host, so existing reader code
works unmodified; the interception point is the ReaderBlock: when a new time level is needed
its block is uploaded once (interpolation/structured.py:15-94 becomes odr_block_upload) and
every ReaderBlock.interpolate becomes a device gather.  Analytic readers that the device
evaluates in closed form (constant, double gyre, oscillating) are recognised by `device_kind`.
"""
from datetime import datetime, timedelta
from numbers import Number

import threading

import numpy as np

from . import _abi, projection


def _epoch(t):
    return (t - datetime(1970, 1, 1)).total_seconds()


class ReaderOperators:
    """readers/operators/ops.py: the arithmetic of readers (Combine, :9-96) and the variable filters (Filter, :100-117).  What the
    reference rejects is rejected here in the same way: `r1 - r2`, `r1 + 2 * r2`, `2 * (3 * r1)` and `(2 * r1) + 1` are TypeErrors,
    because a reader combined with a number (NumCombinedReader) is no reader and has no operators."""

    def __add__(self, other):
        if isinstance(other, Number):
            return NumCombinedReader.add(other, self)
        if isinstance(other, BaseReader):
            return CombinedReader(self, other)
        return NotImplemented

    def __radd__(self, other):
        return self.__add__(other)

    def __mul__(self, other):
        if isinstance(other, Number):
            return NumCombinedReader.mul(other, self)
        return NotImplemented

    def __rmul__(self, other):
        return self.__mul__(other)

    def __truediv__(self, other):
        if isinstance(other, Number):
            return NumCombinedReader.div(other, self)
        return NotImplemented

    def __sub__(self, other):
        return self + (-1 * other)

    def combine_gaussian(self, measurement_reader, std):
        """ops.py:52-96: this reader pulled towards a point measurement (a TimeseriesReader with `lon` / `lat`) with the weight
        exp(-(d / std)^2 / 2) of the WGS84 distance d; std [m].  The reference's form with a LIST of measurement readers is
        refused (NotImplementedError)."""
        return CombinedReader(self, measurement_reader, kind='gaussian', std=std)

    def filter_vars(self, vars):
        """Only keep the specified variables."""
        return FilteredReader(self, vars)

    def exclude_vars(self, vars):
        """Remove the specified variables."""
        return FilteredReader(self, [v for v in self.variables if v not in set(vars)])


class BaseReader(ReaderOperators):
    """Attributes of basereader/__init__.py:107-118 + variables.ReaderDomain (variables.py:20-46)."""
    name = 'reader'
    proj4 = '+proj=latlong'
    xmin = xmax = ymin = ymax = None
    zmin, zmax = -np.inf, np.inf
    start_time = end_time = time_step = times = None
    always_valid = False
    z = None
    variables = []
    device_kind = None   # 'constant' | 'double_gyre' | 'oscillating' | 'landmask' | None (gridded)

    def __init__(self):
        self.proj = projection.Proj(self.proj4)
        self.is_lazy = False
        self.number_of_fails = 0
        if self.start_time is not None and self.time_step is not None and self.times is None:
            n = int(round((self.end_time - self.start_time).total_seconds() / self.time_step.total_seconds())) + 1
            self.times = [self.start_time + k * self.time_step for k in range(n)]

    # ---- variables.py:111-143
    def lonlat2xy(self, lon, lat):
        return self.proj(lon, lat)

    def xy2lonlat(self, x, y):
        return self.proj(x, y, inverse=True)

    def covers_time(self, time):   # variables.py:392-400
        if self.always_valid or self.start_time is None:
            return True
        return self.start_time <= time <= self.end_time

    def nearest_time(self, time):  # variables.py:402-443 -> indices of the bracketing levels
        if self.times is None or len(self.times) == 1:
            return 0, 0
        import bisect
        ib = max(0, bisect.bisect_right(self.times, time) - 1)
        ia = ib if self.times[ib] == time else min(ib + 1, len(self.times) - 1)
        return ib, ia

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        raise NotImplementedError


class ContinuousReader(BaseReader):
    def get_variables_interpolated(self, variables, profiles=None, profiles_depth=None, time=None, lon=None, lat=None, z=None,
                                   rotate_to_proj=None):
        """ContinuousReader._get_variables_interpolated_ (continuous.py:31-46) on the host: ({variable: values exactly at the
        positions, NaN where the reader does not cover position or time}, None) -- what the host evaluation of a reader
        expression asks of its leaves."""
        lon, lat = np.atleast_1d(np.asarray(lon, dtype=np.float64)), np.atleast_1d(np.asarray(lat, dtype=np.float64))
        n = len(lon)
        z = np.zeros(n) if z is None else np.atleast_1d(np.asarray(z, dtype=np.float64)) * np.ones(n)
        env = {v: np.full(n, np.nan) for v in variables}
        if time is not None and not self.covers_time(time):
            return env, None
        x, y = self.lonlat2xy(lon, lat)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        ok = np.ones(n, bool)
        if self.xmin is not None:
            ok &= (x >= self.xmin) & (x <= self.xmax) & (y >= self.ymin) & (y <= self.ymax)
        ok &= (z >= self.zmin) & (z <= self.zmax)
        if ok.any():
            res = self.get_variables(list(variables), time, x[ok], y[ok], z[ok])
            for v in variables:
                a = np.ma.filled(np.ma.asarray(res[v]), np.nan) * np.ones(int(ok.sum()))
                if a.dtype == np.float32:      # the operand keeps its dtype (a float32 array stays one under n * x)
                    env[v] = env[v].astype(np.float32)
                env[v][ok] = a
        return env, None


def convolution_weights(convolve):
    """The kernel __convolve_block__ hands to scipy.ndimage.convolve (structured.py:173-178): ones((N, N)) / ones((N, N)).sum() for
    an int N, else the argument itself as a float64 array."""
    if isinstance(convolve, (int, np.integer)):
        kernel = np.ones((convolve, convolve))
        return kernel / kernel.sum()
    return np.asarray(convolve, dtype=np.float64)


def _convolve_nearest(a, kernel):
    """scipy.ndimage.convolve(a, kernel[..., None] if a is 3-D else kernel, mode='nearest') restated -- the kernel over the first
    two axes of `a`: a correlation with the kernel flipped along both axes, centred at size // 2 (one less along an axis of even
    size), indices clamped to the edge; one float64 accumulator per cell, the terms float64(value) * weight added in C order of
    the flipped kernel, weights with |w| <= DBL_EPSILON left out; rounded once to the array's dtype."""
    flipped = kernel[::-1, ::-1]
    n0, n1 = a.shape[:2]
    c = [s // 2 - (1 if s % 2 == 0 else 0) for s in kernel.shape]
    pad = [(c[0], kernel.shape[0] - 1 - c[0]), (c[1], kernel.shape[1] - 1 - c[1])] + [(0, 0)] * (a.ndim - 2)
    p = np.pad(a, pad, mode='edge').astype(np.float64)
    acc = np.zeros(a.shape, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(kernel.shape[0]):
            for j in range(kernel.shape[1]):
                w = float(flipped[i, j])
                if abs(w) > np.finfo(np.float64).eps:
                    acc = acc + p[i:i + n0, j:j + n1] * w
        return acc.astype(a.dtype)


def convolve_block(env, convolve):
    """StructuredReader.__convolve_block__ (structured.py:167-192) without SciPy: every variable of the block but 'x', 'y', 'z' and
    'time' -- land_binary_mask and sea_floor_depth_below_sea_level included -- convolved in place with the kernel of
    set_convolution_kernel; a 2-D variable over (y, x), a 3-D variable [nz, ny, nx] with kernel[:, :, None], i.e. over (z, y): x is
    not smoothed there (the reference's behaviour).  Returns env.  The arithmetic is the device pass's (csrc/odr_convolve.hip.h):
    equal to scipy.ndimage.convolve bit for bit.  The one deviation: the entries of a masked array count as NaN, as in every
    upload here; the reference convolves whatever data lie under the mask."""
    if convolve is None:
        return env
    kernel = convolution_weights(convolve)
    if kernel.ndim != 2:
        raise ValueError('a convolution kernel is an int or a 2-D array of weights, got shape %s' % (kernel.shape,))
    for v in env:
        if v in ('x', 'y', 'z', 'time') or isinstance(env[v], str):
            continue
        if isinstance(env[v], (list, tuple)):
            if v == 's_level_variables':
                continue
            raise NotImplementedError('ensemble members (%s) are not convolved: the reference fails on the list' % v)
        a = env[v]
        a = np.ma.filled(a, np.nan) if isinstance(a, np.ma.MaskedArray) else np.asarray(a)
        if a.ndim in (2, 3):
            env[v] = _convolve_nearest(a, kernel)
    return env


class StructuredReader(BaseReader):
    """basereader/structured.py.  A reader that sets no projection (`proj4` None or 'fakeproj') but has 2D `lon` /
    `lat` node arrays is 'unprojected' (structured.py:44-113): x/y are pixel indices, xy2lonlat is bilinear in the
    node arrays (:421-436) and lonlat2xy is the Delaunay lookup (:438-472) -- which runs on the device
    (odr_source_grid_curvilinear); on the host it is available once the reader is bound to a device context."""
    projected = True
    convolve = None      # set_convolution_kernel

    def set_convolution_kernel(self, convolve):
        """structured.py:163-165: a convolution kernel, or the size N of a box mean, that every block of this reader is convolved
        with before it is prepared (__convolve_block__, :167-192: scipy.ndimage.convolve(..., mode='nearest') of every variable;
        a 3-D variable with kernel[:, :, None], i.e. over z and y) -- on the device, as the first pass of the level's preparation
        (odr_source_set_convolution; convolve_block is the same arithmetic on the host).  An int N means np.ones((N, N)) / N**2;
        anything else is taken as a 2-D array of weights as given, not normalised; None switches it off.  Levels that are
        resident on the device when the kernel changes stay as they are.  ValueError for a kernel that is not 2-D or has an
        edge longer than _abi.CONVOLVE_MAX_EDGE."""
        if convolve is not None:
            k = convolution_weights(convolve)
            if k.ndim != 2 or k.size == 0:
                raise ValueError('reader %s: a convolution kernel is an int or a 2-D array of weights, got shape %s' % (self.name, k.shape))
            if max(k.shape) > _abi.CONVOLVE_MAX_EDGE:
                raise ValueError('reader %s: convolution kernel of %d x %d weights, at most %d x %d fit the device pass'
                                 % ((self.name,) + k.shape + (_abi.CONVOLVE_MAX_EDGE,) * 2))
        self.convolve = convolve

    def __init__(self):
        if self.proj4 is None or self.proj4 == 'fakeproj':
            self.projected = False
            self.lon = np.ascontiguousarray(self.lon, dtype=np.float64)
            self.lat = np.ascontiguousarray(self.lat, dtype=np.float64)
            self.proj4 = 'None'
            self.xmin = self.ymin = 0.
            self.delta_x = self.delta_y = 1.
            self.xmax = self.lon.shape[1] - 1
            self.ymax = self.lon.shape[0] - 1
            self.numx, self.numy = self.xmax, self.ymax
            self.x = np.arange(0, self.xmax + 1)
            self.y = np.arange(0, self.ymax + 1)
            self._device_lookup = None
            proj4, self.proj4 = self.proj4, '+proj=latlong'
            super().__init__()
            self.proj4, self.proj = proj4, None
        else:
            super().__init__()

    def xy2lonlat(self, x, y):
        if self.projected:
            return super().xy2lonlat(x, y)
        x, y = np.array(x, dtype=np.float64, ndmin=1), np.array(y, dtype=np.float64, ndmin=1)
        bad = (x < self.xmin) | (x > self.xmax) | (y < self.ymin) | ~np.isfinite(x) | ~np.isfinite(y)
        xc, yc = np.where(bad, 0.0, x), np.clip(np.where(bad, 0.0, y), 0, self.ymax)   # mode='nearest' beyond ymax
        i0 = np.minimum(xc.astype(np.int64), self.lon.shape[1] - 2)
        j0 = np.minimum(yc.astype(np.int64), self.lon.shape[0] - 2)
        tx, ty = xc - i0, yc - j0

        def bil(a):
            return ((1 - ty) * ((1 - tx) * a[j0, i0] + tx * a[j0, i0 + 1]) +
                    ty * ((1 - tx) * a[j0 + 1, i0] + tx * a[j0 + 1, i0 + 1]))
        lon, lat = bil(self.lon), bil(self.lat)
        lon[bad] = np.nan
        lat[bad] = np.nan
        return lon, lat

    def lonlat2xy(self, lon, lat):
        if self.projected:
            return super().lonlat2xy(lon, lat)
        if self._device_lookup is None:
            raise RuntimeError('reader %s has no projection: lonlat2xy is the device lookup, available once the '
                               'reader is part of a simulation (add_reader + first step)' % self.name)
        return self._device_lookup(lon, lat)


class ConstantReader(ContinuousReader):
    """reader_constant.Reader (readers/reader_constant.py): the same value everywhere."""
    device_kind = 'constant'

    def __init__(self, parameter_value_map=None, **kwargs):
        m = dict(parameter_value_map or kwargs)
        self._element_ID = None
        if 'element_ID' in m:
            # values per element (reader_constant.py:42-58,70-80): the listed IDs get their values, every other element
            # NaN -> next reader / fallback.  Evaluated on the host at every sample (no closed form for the device).
            self.device_kind = None
            self._element_ID = True              # set to the IDs of the call by the model (environment.py:621-623)
            self._ids = np.atleast_1d(np.asarray(m.pop('element_ID'))).astype(np.int64)
            self._parameter_value_map = {k: np.atleast_1d(np.asarray(v, dtype=np.float64)) for k, v in m.items()}
        else:
            self._parameter_value_map = {k: float(np.atleast_1d(v)[0]) for k, v in m.items()}
        self.variables = list(self._parameter_value_map)
        self.proj4 = '+proj=latlong'
        self.xmin, self.xmax, self.ymin, self.ymax = -180, 180, -90, 90
        self.name = 'constant_reader'
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        out = {'time': time, 'x': x, 'y': y, 'z': z}
        for v in requested_variables:
            value = self._parameter_value_map[v]
            if self._element_ID is None:
                out[v] = value * np.ones(np.shape(x))
                continue
            ids = np.atleast_1d(self._element_ID)              # the IDs of this call's elements
            a = np.full(np.shape(x), np.nan)
            pos = {int(i): k for k, i in enumerate(self._ids)}
            hit = np.array([int(i) in pos for i in ids], dtype=bool)
            if hit.any():
                a[hit] = value[0] if len(value) == 1 else value[[pos[int(i)] for i in ids[hit]]]
            out[v] = a
        return out


class LandmaskRasterReader(ContinuousReader):
    """reader_global_landmask.Reader (readers/reader_global_landmask.py:201-255) over a lon/lat raster handed in by the
    caller: land_binary_mask exactly at the element positions.  The reference's class wraps the GSHHG dataset through
    roaring_landmask, which is not part of this repository; its contains_many(x, y) is what `cells` replaces:
    cells[iy, ix] != 0 is land, cell (ix, iy) covers lon0 + [ix, ix+1) dlon x lat0 + [iy, iy+1) dlat, ocean outside.
    It is also the landmask `coastline_crossing` searches when general:coastline_approximation_precision is set."""
    device_kind = 'landmask'
    name = 'global_landmask'
    variables = ['land_binary_mask']

    def __init__(self, lon0, lat0, dlon, dlat, cells):
        self.lon0, self.lat0, self.dlon, self.dlat = float(lon0), float(lat0), float(dlon), float(dlat)
        self.cells = np.ascontiguousarray(np.asarray(cells) != 0, dtype=np.uint8)
        self.proj4 = '+proj=latlong'
        self.xmin, self.xmax, self.ymin, self.ymax = -180, 180, -90, 90
        self.always_valid = True
        super().__init__()

    def contains_many(self, x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        ix = np.floor((x - self.lon0) / self.dlon).astype(np.int64)
        iy = np.floor((y - self.lat0) / self.dlat).astype(np.int64)
        ny, nx = self.cells.shape
        ok = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
        out = np.zeros(x.shape, bool)
        out[ok] = self.cells[iy[ok], ix[ok]] != 0
        return out

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        x = np.mod(np.asarray(x, dtype=np.float64) + 180, 360) - 180      # modulate_longitude
        return {'time': time, 'x': x, 'y': y, 'z': z, 'land_binary_mask': self.contains_many(x, y)}


class FailingReader(ContinuousReader):
    """reader_failing.Reader (readers/reader_failing.py:20-43): raises in every call, for testing the quarantine of
    readers after readers:max_number_of_fails failures."""

    def __init__(self):
        self.variables = ['x_wind', 'y_wind']
        self.proj4 = '+proj=latlong'
        self.xmin, self.xmax, self.ymin, self.ymax = -180, 180, -90, 90
        self.name = 'failing_reader'
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        raise ValueError('Failing reader, for testing only.')


class DoubleGyreReader(ContinuousReader):
    """reader_double_gyre.Reader (readers/reader_double_gyre.py:24-79)."""
    device_kind = 'double_gyre'

    def __init__(self, initial_time=datetime(2000, 1, 1), epsilon=0.1, omega=0.628, A=0.25,
                 proj4='+proj=stere +lat_0=0 +lon_0=0 +lat_ts=0 +units=m +a=6.371e+06 +e=0 +no_defs'):
        self.name = 'double_gyre'
        self.proj4 = proj4
        self.xmin, self.xmax, self.ymin, self.ymax = 0., 2., 0., 1.
        self.A, self.epsilon, self.omega, self.initial_time = A, epsilon, omega, initial_time
        self.variables = ['x_sea_water_velocity', 'y_sea_water_velocity']
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        t = (time - self.initial_time).total_seconds()
        a = self.epsilon * np.sin(self.omega * t)
        b = 1 - 2 * self.epsilon * np.sin(self.omega * t)
        f = a * x * x + b * x
        dfdx = 2 * a * x + b
        return {'x_sea_water_velocity': -np.pi * self.A * np.sin(np.pi * f) * np.cos(np.pi * y),
                'y_sea_water_velocity': np.pi * self.A * np.cos(np.pi * f) * np.sin(np.pi * y) * dfdx,
                'land_binary_mask': np.zeros(np.shape(x)), 'time': time, 'x': x, 'y': y}


class OscillatingReader(ContinuousReader):
    """reader_oscillating.Reader (readers/reader_oscillating.py:23-59)."""
    device_kind = 'oscillating'

    def __init__(self, variable, amplitude, period=timedelta(hours=24), phase=0, zero_time=datetime(2017, 1, 1)):
        self.variables = [variable]
        self.amplitude, self.period_seconds, self.zero_time = amplitude, period.total_seconds(), zero_time
        self.proj4 = '+proj=latlong +datum=WGS84'
        self.xmin, self.xmax, self.ymin, self.ymax = -180, 180, -90, 90
        self.name = 'oscillating_reader'
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        phase = ((time - self.zero_time).total_seconds() / self.period_seconds) * np.pi
        return {'time': time, 'x': x, 'y': y, 'z': z,
                self.variables[0]: self.amplitude * np.sin(phase) * np.ones(np.shape(x))}


# the x / y components the reference rotates from the reader's axes to east / north (basereader/consts.py:27-36)
VECTOR_PAIRS_XY = [('x_wind', 'y_wind'), ('sea_ice_x_velocity', 'sea_ice_y_velocity'),
                   ('x_sea_water_velocity', 'y_sea_water_velocity'),
                   ('sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity')]


def wgs84_forward_azimuth(lon1, lat1, lon2, lat2):
    """Azimuth (degrees clockwise from north) at point 1 of the WGS84 geodesic to point 2 -- what pyproj.Geod(ellps='WGS84')
    .inv(...)[0] gives the reference in rotate_vectors (variables.py:94-97) -- by Vincenty's inverse iteration (short lines
    between neighbouring grid nodes: converges in a few rounds)."""
    a, f = 6378137.0, 1 / 298.257223563
    b = (1 - f) * a
    L = np.radians(np.asarray(lon2, dtype=np.float64) - np.asarray(lon1, dtype=np.float64))
    L = (L + np.pi) % (2 * np.pi) - np.pi
    U1 = np.arctan((1 - f) * np.tan(np.radians(np.asarray(lat1, dtype=np.float64))))
    U2 = np.arctan((1 - f) * np.tan(np.radians(np.asarray(lat2, dtype=np.float64))))
    sU1, cU1, sU2, cU2 = np.sin(U1), np.cos(U1), np.sin(U2), np.cos(U2)
    lam = L.copy()
    for _ in range(30):
        sl, cl = np.sin(lam), np.cos(lam)
        ss = np.hypot(cU2 * sl, cU1 * sU2 - sU1 * cU2 * cl)
        cs = sU1 * sU2 + cU1 * cU2 * cl
        sig = np.arctan2(ss, cs)
        with np.errstate(invalid='ignore', divide='ignore'):
            sa = np.where(ss > 0, cU1 * cU2 * sl / ss, 0.0)
            c2a = 1 - sa * sa
            c2m = np.where(c2a > 0, cs - 2 * sU1 * sU2 / c2a, 0.0)
        Cc = f / 16 * c2a * (4 + f * (4 - 3 * c2a))
        new = L + (1 - Cc) * f * sa * (sig + Cc * ss * (c2m + Cc * cs * (-1 + 2 * c2m * c2m)))
        done = np.max(np.abs(new - lam)) < 1e-14
        lam = new
        if done:
            break
    return np.degrees(np.arctan2(cU2 * np.sin(lam), cU1 * sU2 - sU1 * cU2 * np.cos(lam)))


def wgs84_distance(lon1, lat1, lon2, lat2):
    """Length [m] of the WGS84 geodesic between two points -- pyproj.Geod(ellps='WGS84').inv(...)[2] -- by Vincenty's inverse
    iteration: within a millimetre of it except between nearly antipodal points, where the iteration does not converge (the
    device's inverse, csrc/odr_geodinv.hip.h, has no such limit)."""
    a, f = 6378137.0, 1 / 298.257223563
    b = (1 - f) * a
    L = np.radians(np.asarray(lon2, dtype=np.float64) - np.asarray(lon1, dtype=np.float64))
    L = (L + np.pi) % (2 * np.pi) - np.pi
    U1 = np.arctan((1 - f) * np.tan(np.radians(np.asarray(lat1, dtype=np.float64))))
    U2 = np.arctan((1 - f) * np.tan(np.radians(np.asarray(lat2, dtype=np.float64))))
    sU1, cU1, sU2, cU2 = np.sin(U1), np.cos(U1), np.sin(U2), np.cos(U2)
    lam = L * np.ones(np.broadcast(sU1, sU2).shape)
    for _ in range(100):
        sl, cl = np.sin(lam), np.cos(lam)
        ss = np.hypot(cU2 * sl, cU1 * sU2 - sU1 * cU2 * cl)
        cs = sU1 * sU2 + cU1 * cU2 * cl
        sig = np.arctan2(ss, cs)
        with np.errstate(invalid='ignore', divide='ignore'):
            sa = np.where(ss > 0, cU1 * cU2 * sl / ss, 0.0)
            c2a = 1 - sa * sa
            c2m = np.where(c2a > 0, cs - 2 * sU1 * sU2 / c2a, 0.0)
        Cc = f / 16 * c2a * (4 + f * (4 - 3 * c2a))
        new = L + (1 - Cc) * f * sa * (sig + Cc * ss * (c2m + Cc * cs * (-1 + 2 * c2m * c2m)))
        done = np.all(np.abs(new - lam) < 1e-15) if np.size(new) else True
        lam = new
        if done:
            break
    u2 = c2a * (a * a - b * b) / (b * b)
    A = 1 + u2 / 16384 * (4096 + u2 * (-768 + u2 * (320 - 175 * u2)))
    B = u2 / 1024 * (256 + u2 * (-128 + u2 * (74 - 47 * u2)))
    dsig = B * ss * (c2m + B / 4 * (cs * (-1 + 2 * c2m * c2m) - B / 6 * c2m * (-3 + 4 * ss * ss) * (-3 + 4 * c2m * c2m)))
    return b * A * (sig - dsig)


def node_y_azimuth(lon2d, lat2d):
    """Azimuth of the mesh's +y direction at every node: from the node to its neighbour one row up (the last row: the
    arrival azimuth of the line from the row below), on WGS84."""
    lon2d, lat2d = np.asarray(lon2d, dtype=np.float64), np.asarray(lat2d, dtype=np.float64)
    az = np.empty(lon2d.shape)
    az[:-1] = wgs84_forward_azimuth(lon2d[:-1], lat2d[:-1], lon2d[1:], lat2d[1:])
    az[-1] = (wgs84_forward_azimuth(lon2d[-1], lat2d[-1], lon2d[-2], lat2d[-2]) + 180.0 + 180.0) % 360.0 - 180.0
    return az


class GridReader(StructuredReader):
    """In-memory StructuredReader with time levels and optional z levels (the shape of
    reader_constant_2d.py:20-49 / reader_netCDF_CF_generic / reader_ROMS_native output blocks).
    arrays: {variable: [nt, ny, nx] or [nt, nz, ny, nx], or a list of such arrays = ensemble members}.

    A projection the device has no closed form for (rotated pole `ob_tran`, utm, laea, ... -- the reference hands any proj4
    to pyproj, variables.py:111-143): give the 2-D node coordinates `lon`, `lat` that such files carry.  The reader is then
    served like one WITHOUT projection (structured.py:44-113): positions through the node-array lookup on the device
    (odr_source_grid_curvilinear), and the vector pairs of every block rotated to east / north at the nodes by the azimuth
    of the mesh's y axis (rotate_vectors, variables.py:59-108, does it after the interpolation, at the element: the
    difference is second order in the turn of the axes across one cell -- DESIGN.md 9)."""
    # A reference file reader hands out the z levels ASKED FOR (one more on either side + verticalbuffer,
    # reader_netCDF_CF_generic.py:414-423, basereader/__init__.py:52); the device block of this reader always holds every level,
    # and OceanDrift applies that cut to the diffusivity columns where it matters (drift:truncate_ocean_model_below_m).  A reader
    # standing for one that ignores the depth range asked of it sets always_delivers_all_levels = True.
    verticalbuffer = 1
    always_delivers_all_levels = False

    def __new__(cls, x, y, times, arrays, z=None, proj4='+proj=latlong', name='grid_reader', lon=None, lat=None):
        if cls is GridReader and proj4 is not None:
            try:
                projection.parse_proj4(proj4)
            except NotImplementedError:
                if lon is None or lat is None:
                    raise NotImplementedError(
                        'projection "%s" has no closed form on the device (latlong, stere, merc, lcc have): pass the 2-D node '
                        'coordinates lon=, lat= of the grid and the reader is served through the node lookup' % proj4)
                r = object.__new__(NodeLookupGridReader)     # not a GridReader instance: Python does not call __init__ on it
                r.__init__(x, y, times, arrays, z=z, proj4=proj4, name=name, lon=lon, lat=lat)
                return r
        return object.__new__(cls)

    def __init__(self, x, y, times, arrays, z=None, proj4='+proj=latlong', name='grid_reader', lon=None, lat=None):
        self.proj4, self.name = proj4, name
        self.x, self.y, self.z = np.asarray(x), np.asarray(y), (None if z is None else np.asarray(z, dtype=np.float64))
        self.xmin, self.xmax = float(self.x.min()), float(self.x.max())
        self.ymin, self.ymax = float(self.y.min()), float(self.y.max())
        self.times = list(times)
        self.start_time, self.end_time = self.times[0], self.times[-1]
        self.time_step = (self.times[1] - self.times[0]) if len(self.times) > 1 else None
        self.arrays = arrays
        # 2-D variables that are the same array at every time level (sea floor depth, land mask): declared once here, so that
        # the device reads them at one of the two bracketing levels (odr_block_set_content_ids) without comparing levels
        def same(a, b):
            return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)
        self.static_variables = [v for v, a in arrays.items() if isinstance(a, np.ndarray) and a.ndim == 3 and a.shape[0] > 1 and
                                 all(same(a[0], a[k]) for k in range(1, a.shape[0]))]
        self.variables = list(arrays)
        super().__init__()

    buffer = 2      # pixels around the requested positions (StructuredReader.set_buffer_size, structured.py:125-147)

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        """The block covering the requested positions x, y plus `buffer` pixels (as reader_netCDF_CF_generic /
        reader_ROMS_native cut it, reader_netCDF_CF_generic.py:404-470); without positions the whole domain."""
        it = self.times.index(time)
        jy, ix = slice(None), slice(None)
        if x is not None and y is not None and np.size(x) > 0 and self.x.ndim == 1 and len(self.x) > 1:
            def window(c, q):
                asc = c[-1] > c[0]
                ca = c if asc else c[::-1]
                lo = int(np.clip(np.searchsorted(ca, np.nanmin(q), side='right') - 1 - self.buffer, 0, len(c) - 1))
                hi = int(np.clip(np.searchsorted(ca, np.nanmax(q), side='left') + self.buffer, 0, len(c) - 1))
                return slice(lo, hi + 1) if asc else slice(len(c) - 1 - hi, len(c) - lo)
            ix, jy = window(np.asarray(self.x, dtype=np.float64), np.asarray(x, dtype=np.float64)), \
                window(np.asarray(self.y, dtype=np.float64), np.asarray(y, dtype=np.float64))
        out = {'x': self.x[ix], 'y': self.y[jy], 'time': time, 'z': self.z if self.z is not None else 0}
        for v in requested_variables:
            a = self.arrays[v]
            if isinstance(a, (list, tuple)):      # ensemble data: a list of member arrays (structured.py:125-147)
                out[v] = [m[it][..., jy, ix] for m in a]
            else:
                out[v] = a[it][..., jy, ix]
        return out


class CurvilinearGridReader(StructuredReader):
    """In-memory StructuredReader on a curvilinear mesh given by 2D lon/lat node arrays and NO projection -- the
    situation of reader_ROMS_native / reader_netCDF_CF_generic files that only carry lon(y,x), lat(y,x)
    (structured.py:44-113).  arrays: {variable: [nt, ny, nx] or [nt, nz, ny, nx]}; vector components are taken as
    east/north (the reference's rotation for such readers is by the azimuth of due north, i.e. none)."""

    def __init__(self, lon, lat, times, arrays, z=None, name='curvilinear_grid_reader'):
        self.proj4, self.name = None, name
        self.lon, self.lat = lon, lat
        self.z = None if z is None else np.asarray(z, dtype=np.float64)
        self.times = list(times)
        self.start_time, self.end_time = self.times[0], self.times[-1]
        self.time_step = (self.times[1] - self.times[0]) if len(self.times) > 1 else None
        self.arrays = arrays
        self.variables = list(arrays)
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        it = self.times.index(time)
        out = {'x': self.x, 'y': self.y, 'time': time, 'z': self.z if self.z is not None else 0}
        for v in requested_variables:
            out[v] = self.arrays[v][it]
        return out


class NodeLookupGridReader(CurvilinearGridReader):
    """What GridReader(...) returns for a proj4 string the device cannot evaluate: the same arrays behind 2-D node
    coordinates, vector pairs rotated to east / north per block (see GridReader)."""

    def __init__(self, x, y, times, arrays, z=None, proj4=None, name='grid_reader', lon=None, lat=None):
        lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
        if lon.shape != (len(y), len(x)) or lat.shape != lon.shape:
            raise ValueError('lon / lat must be [len(y), len(x)] node arrays')
        self.native_proj4 = proj4
        self.native_x, self.native_y = np.asarray(x), np.asarray(y)
        super().__init__(lon, lat, times, arrays, z=z, name=name)
        rot = -np.radians(node_y_azimuth(lon, lat))          # rot_angle_rad = -rot_angle_vectors_rad (variables.py:103)
        self._cos, self._sin = np.cos(rot), np.sin(rot)
        self._pairs = [(a, b) for a, b in VECTOR_PAIRS_XY if a in self.arrays and b in self.arrays]

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        out = super().get_variables(requested_variables, time, x, y, z)
        for a, b in self._pairs:
            if a in out and b in out:
                def rotate(u, v):
                    # masked cells (land, missing data of a netCDF block) become NaN as in the plain upload path
                    # (np.ma.filled); np.asarray() would hand the fill value 9.96921e36 on as a velocity
                    u = np.ma.filled(np.ma.asarray(u).astype(np.float32), np.nan)
                    v = np.ma.filled(np.ma.asarray(v).astype(np.float32), np.nan)
                    return ((u * self._cos - v * self._sin).astype(np.float32),      # variables.py:104-107
                            (u * self._sin + v * self._cos).astype(np.float32))
                if isinstance(out[a], (list, tuple)):      # ensemble members
                    rot = [rotate(u, v) for u, v in zip(out[a], out[b])]
                    out[a], out[b] = [r[0] for r in rot], [r[1] for r in rot]
                else:
                    out[a], out[b] = rotate(out[a], out[b])
            elif a in out or b in out:
                raise ValueError('reader %s: %s and %s are rotated together -- request both' % (self.name, a, b))
        return out


ROMS_ZLEVELS = np.array([0, -.5, -1, -3, -5, -10, -25, -50, -75, -100, -150, -200, -250, -300, -400, -500, -600, -700,
                         -800, -900, -1000, -1500, -2000, -2500, -3000, -3500, -4000, -4500, -5000, -5500, -6000, -6500,
                         -7000, -7500, -8000], dtype=np.float64)   # reader_ROMS_native.py:134-138


class SigmaGridReader(StructuredReader):
    """In-memory reader with the vertical structure of reader_ROMS_native: 3-D variables live on N terrain-following
    s-levels (arrays3d: {variable: [nt, N, ny, nx]}), 2-D ones on the grid (arrays2d: {variable: [nt, ny, nx]}); `h`
    bottom depth, `hc`, `Cs_r`, `Vtransform` as in a ROMS file.  Blocks handed to the model are on the reader's fixed
    z levels (`zlevels`, default: the reference's list down to the deepest node), regridded per time level as
    reader_ROMS_native.get_variables does (:617-684) -- on the device (`s_levels = True` tells the binding that
    get_variables returns s-level arrays plus the target levels)."""
    s_levels = True

    def __init__(self, x, y, times, arrays3d, arrays2d, h, hc, Cs_r, Vtransform=2, zlevels=None, proj4='+proj=latlong',
                 name='sigma_grid_reader'):
        self.proj4, self.name = proj4, name
        self.x, self.y = np.asarray(x), np.asarray(y)
        self.h = np.ascontiguousarray(h, dtype=np.float64)
        self.hc, self.Cs_r, self.Vtransform = float(hc), np.asarray(Cs_r, dtype=np.float64), int(Vtransform)
        if zlevels is None:
            deeper = np.nonzero(ROMS_ZLEVELS < -float(self.h.max()))[0]
            zlevels = ROMS_ZLEVELS[:deeper[0] + 1] if len(deeper) else ROMS_ZLEVELS
        self.z = np.asarray(zlevels, dtype=np.float64)
        self.xmin, self.xmax = float(self.x.min()), float(self.x.max())
        self.ymin, self.ymax = float(self.y.min()), float(self.y.max())
        self.times = list(times)
        self.start_time, self.end_time = self.times[0], self.times[-1]
        self.time_step = (self.times[1] - self.times[0]) if len(self.times) > 1 else None
        self.arrays3d, self.arrays2d = dict(arrays3d), dict(arrays2d)
        self.variables = list(self.arrays3d) + list(self.arrays2d)
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        it = self.times.index(time)
        out = {'x': self.x, 'y': self.y, 'time': time, 'z': self.z,
               's_level_variables': [v for v in requested_variables if v in self.arrays3d]}
        for v in requested_variables:
            out[v] = self.arrays3d[v][it] if v in self.arrays3d else self.arrays2d[v][it]
        return out


class UnstructuredReader(BaseReader):
    """In-memory reader on a triangular mesh, the reference's UnstructuredReader family (basereader/unstructured.py,
    reader_netCDF_CF_unstructured.py; FVCOM-style output): node variables at the nearest node, face variables at the nearest
    face centre, 3-D ones at the nearest sigma layer or level of that column, all at the nearest time level.  Nothing is
    interpolated.

    x, y [N] / xc, yc [E]: node / face-centre coordinates in the mesh's CRS (`proj4`).  node_arrays / face_arrays: {variable:
    [nt, N] | [nt, L, N] | [N]} (over E for faces); a [nt, L, .] array is on the layers when L == len(siglay), on the levels when
    L == len(siglev) -- decided by the count, as the reference decides by shp[1].  siglay [L, N], siglev [L + 1, N], h [N] and
    their *_center / h_center twins over the faces are kept as float32, which is what model files hold: float64 input is ROUNDED
    to float32 here, so that sigma * h is the float32 product the reference forms.

    On the device (`device_kind = 'umesh'`) the whole get_variables -- projection, search, sigma rule, gather, rotation of vector
    pairs, merge by priority -- is one launch per call (odr_umesh_sample).  `get_variables` below answers on the
    host with scipy's cKDTree, as the reference does; it needs no device.

    Two deviations from the reference, on purpose: a 2-D variable is the value at the nearest node / face at the
    nearest time (the reference's 2-D branch returns a slab of the array without picking per element or per time), and any
    array with a level axis is 3-D (the reference asks for a dimension literally named 'siglev' on nodes)."""
    device_kind = 'umesh'

    def __init__(self, x, y, xc, yc, times, node_arrays, face_arrays, siglay=None, siglev=None, siglay_center=None, siglev_center=None,
                 h=None, h_center=None, proj4='+proj=latlong', name='unstructured_reader'):
        self.proj4, self.name = proj4, name
        pd = projection.parse_proj4(proj4)        # NotImplementedError: not on the device path
        if pd.get('kind') == 'ob_tran':
            raise NotImplementedError('a mesh on a rotated pole (+proj=ob_tran) is not on the device path')
        self.x, self.y = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y))
        self.xc, self.yc = (np.ascontiguousarray(a if a is not None else [], dtype=np.float64).ravel() for a in (xc, yc))
        if len(self.x) != len(self.y) or len(self.xc) != len(self.yc) or len(self.x) == 0:
            raise ValueError('%d x and %d y node coordinates, %d xc and %d yc face centres' % (len(self.x), len(self.y), len(self.xc), len(self.yc)))
        if not (np.isfinite(self.x).all() and np.isfinite(self.y).all() and np.isfinite(self.xc).all() and np.isfinite(self.yc).all()):
            raise ValueError('a mesh coordinate is not finite')
        N, E = len(self.x), len(self.xc)
        self.xmin, self.xmax, self.ymin, self.ymax = float(self.x.min()), float(self.x.max()), float(self.y.min()), float(self.y.max())
        self.times = None if times is None else list(times)
        if self.times:
            if any(b <= a for a, b in zip(self.times, self.times[1:])):
                raise ValueError('times must increase')
            self.start_time, self.end_time = self.times[0], self.times[-1]

        def f32(a, npts, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape[-1] != npts:
                raise ValueError('%s has %d points, the mesh %d' % (what, a.shape[-1], npts))
            return a
        self.siglay, self.siglev, self.h = f32(siglay, N, 'siglay'), f32(siglev, N, 'siglev'), f32(h, N, 'h')
        self.siglay_center, self.siglev_center, self.h_center = f32(siglay_center, E, 'siglay_center'), \
            f32(siglev_center, E, 'siglev_center'), f32(h_center, E, 'h_center')
        lays = [a.shape[0] for a in (self.siglay, self.siglay_center) if a is not None]
        levs = [a.shape[0] - 1 for a in (self.siglev, self.siglev_center) if a is not None]
        if len(set(lays + levs)) > 1:
            raise ValueError('the sigma arrays disagree on the number of layers: %s layers, %s levels' % (lays, [k + 1 for k in levs]))
        self.n_siglay = (lays + levs + [0])[0]
        self.node_arrays, self.face_arrays = {}, {}
        nt = len(self.times) if self.times else 1
        for arrays, mine, npts, sig, depth, where in ((node_arrays or {}, self.node_arrays, N, (self.siglay, self.siglev), self.h, 'node'),
                                                      (face_arrays or {}, self.face_arrays, E, (self.siglay_center, self.siglev_center),
                                                       self.h_center, 'face')):
            for v, a in arrays.items():
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.ndim not in (1, 2, 3) or a.shape[-1] != npts or (a.ndim > 1 and a.shape[0] != nt):
                    raise ValueError('%s variable %s of shape %s: expected [%d], [%d, %d] or [%d, levels, %d]' % (where, v, a.shape, npts, nt, npts, nt, npts))
                if a.ndim == 3:
                    L = a.shape[1]
                    s = sig[0] if L == self.n_siglay else sig[1] if L == self.n_siglay + 1 else None
                    if not self.n_siglay or s is None or depth is None:
                        raise ValueError('%s variable %s has %d levels: the reader needs the matching sigma array (%d layers) and the depth '
                                         '%s' % (where, v, L, self.n_siglay, 'h' if where == 'node' else 'h_center'))
                mine[v] = a
        both = set(self.node_arrays) & set(self.face_arrays)
        if both:
            raise ValueError('%s given on nodes and on faces' % sorted(both))
        self.variables = list(self.node_arrays) + list(self.face_arrays)
        self._trees = {}
        super().__init__()

    # ---- time: the `times` branch of variables.py:417-430
    def nearest_time(self, time):
        """(nearest_time, time_before, time_after, indx_nearest, indx_before, indx_after); midway between two levels: the later."""
        if not self.times:
            return None, None, None, 0, 0, 0
        if len(self.times) == 1:
            return self.times[0], self.times[0], None, 0, 0, 0
        import bisect
        ib = max(0, bisect.bisect_left(self.times, time) - 1)
        if ib + 1 < len(self.times) and self.times[ib + 1] == time:
            ib += 1
        ia = min(ib + 1, len(self.times) - 1)
        k = ib if (time - self.times[ib]) < (self.times[ia] - time) else ia
        return self.times[k], self.times[ib], self.times[ia], k, ib, ia

    def placement(self, variable):
        """(array, on_faces, number of levels or 0) of a variable; ValueError when the reader has neither."""
        if variable in self.node_arrays:
            a, on_faces = self.node_arrays[variable], False
        elif variable in self.face_arrays:
            a, on_faces = self.face_arrays[variable], True
        else:
            raise ValueError('Variable not available: %s\nAvailable parameters are: %s' % (variable, self.variables))
        return a, on_faces, (a.shape[1] if a.ndim == 3 else 0)

    def level(self, variable, k):
        """The array of time level k: [points] or [levels, points]."""
        a = self.placement(variable)[0]
        return a if a.ndim == 1 else a[k]

    def _tree(self, on_faces):
        if on_faces not in self._trees:
            from scipy.spatial import cKDTree
            self._trees[on_faces] = cKDTree(np.c_[self.xc, self.yc] if on_faces else np.c_[self.x, self.y])
        return self._trees[on_faces]

    def nearest_node(self, x, y):
        return self._tree(False).query(np.c_[x, y], k=1)[1]

    def nearest_face(self, x, y):
        return self._tree(True).query(np.c_[x, y], k=1)[1]

    def sigma_index(self, variable, idx, z):
        """argmin(|sigma[:, idx] * h[idx] - z|), the first minimum (__nearest_node_sigma__ / __nearest_face_sigma__)."""
        _, on_faces, L = self.placement(variable)
        lay = L == self.n_siglay
        sigma = (self.siglay_center if lay else self.siglev_center) if on_faces else (self.siglay if lay else self.siglev)
        depths = sigma[:, idx] * (self.h_center if on_faces else self.h)[idx]
        return np.argmin(np.abs(depths - np.atleast_2d(np.asarray(z, dtype=np.float64))), axis=0)

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        """{variable: float32 values at the nearest node / face, sigma layer / level and time level} for positions x, y in the
        mesh's coordinates and depths z -- for every position, covered or not (the caller masks, as the reference's does)."""
        if isinstance(requested_variables, str):
            requested_variables = [requested_variables]
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
        z = np.zeros(len(x)) if z is None else np.broadcast_to(np.asarray(z, dtype=np.float64), x.shape)
        if time is None:
            time = self.start_time
        if self.times and not self.covers_time(time):
            raise ValueError('Requested time (%s) is outside the time coverage (%s - %s) of %s' % (time, self.start_time, self.end_time, self.name))
        k = self.nearest_time(time)[3]
        out, found = {}, {}
        for v in requested_variables:
            a, on_faces, L = self.placement(v)
            if on_faces not in found:
                found[on_faces] = self.nearest_face(x, y) if on_faces else self.nearest_node(x, y)
            idx = found[on_faces]
            lev = self.level(v, k)
            out[v] = lev[self.sigma_index(v, idx, z), idx] if L else lev[idx]
        return out

    def rotation_angle(self, x, y):
        """rot_angle_rad of rotate_vectors (variables.py:59-109) at mesh positions: minus the WGS84 azimuth of the 10 m line along +y."""
        lo1, la1 = self.xy2lonlat(x, y)
        lo2, la2 = self.xy2lonlat(x, np.asarray(y) + 10.0)
        return -np.radians(wgs84_forward_azimuth(lo1, la1, lo2, la2))

    def modulate_longitude(self, lon):      # variables.py:259-280, for a geographic mesh
        lon = np.asarray(lon, dtype=np.float64)
        return np.mod(lon + 180, 360) - 180 if self.xmin < 0 else np.mod(lon, 360)

    def get_variables_interpolated(self, variables, time, lon, lat, z, rotate=True):
        """What the device launch gives an element with an empty slot, on the host: NaN outside the box of the nodes or outside
        the time coverage, vector pairs rotated to east / north unless the mesh is geographic."""
        lon, lat = np.atleast_1d(np.asarray(lon, dtype=np.float64)), np.atleast_1d(np.asarray(lat, dtype=np.float64))
        n = len(lon)
        out = {v: np.full(n, np.nan, np.float32) for v in variables}
        for v in variables:
            self.placement(v)
        if self.times and not self.covers_time(time):
            return out
        geographic = projection.parse_proj4(self.proj4).get('kind', 'latlong') == 'latlong'
        x, y = (self.modulate_longitude(lon), lat) if geographic else self.lonlat2xy(lon, lat)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(x + y) & (x >= self.xmin) & (x <= self.xmax) & (y >= self.ymin) & (y <= self.ymax)
        if not ok.any():
            return out
        zz = np.broadcast_to(np.asarray(z, dtype=np.float64), (n,))[ok]
        res = self.get_variables(list(variables), time, x[ok], y[ok], zz)
        if rotate and not geographic:
            for vx, vy in VECTOR_PAIRS_XY:
                if vx in res and vy in res:
                    rot = self.rotation_angle(x[ok], y[ok])
                    u, w = res[vx], res[vy]
                    res[vx], res[vy] = u * np.cos(rot) - w * np.sin(rot), u * np.sin(rot) + w * np.cos(rot)
        for v in variables:
            out[v][ok] = res[v]
        return out


class SchismReader(BaseReader):
    """In-memory reader on a triangular mesh that INTERPOLATES, the reference's reader for SCHISM output
    (readers/reader_schism_native.py): every time level is a cloud of points -- the nodes for a 2-D variable, node x vertical level
    at the level's own `zcor` for a 3-D one -- a value is the inverse-distance mean over the three nearest points of that cloud
    (ReaderBlockUnstruct.interpolate, :982-1056), and the values of the two time levels that bracket the time are blended
    linearly (:614-642).

    x, y [N]: node coordinates in the mesh's CRS (`proj4`; None: geographic, as the reference assumes).  node_arrays: {variable:
    [nt, N] | [N] (static) | [nt, N, L] (3-D, SCHISM's own axis order)}; zcor [nt, N, L]: the vertical coordinate, negative down,
    NaN or masked for the levels below the sea bed of a node, +-inf becomes 15.0 (:942-943).  All are kept as float32, which is
    what model files hold; NaN or masked data is no data, and a NaN neighbour makes the mean NaN (a dry node in the reference).

    use_3d follows :129-143 and :246-248: None means 3-D when a 3-D array and zcor are given; 3-D without zcor raises the
    reference's ValueError; a geographic mesh switches it off (metres and degrees do not mix in one distance), and 3-D arrays are
    then refused: the caller gives depth-averaged ones.

    Coverage is strict inclusion in the convex hull of the nodes (basereader/unstructured.py:76-144), tested with ShapeReader's
    crossing rule; the reference tests with shapely, so a point exactly ON the hull's edge may fall on the other side here.

    On the device (`device_kind = 'schism'`) a whole get_environment call -- projection, hull test, the exact three-nearest search
    in 2-D and per time level in 3-D, weights, time blend, rotation of vector pairs, merge by priority -- is one launch
    (odr_schism_sample).  `get_variables_interpolated` answers on the host with scipy's cKDTree and NumPy, written
    from the reference's expressions; it needs no device.

    Refused by name: land_binary_mask (the reference's branch for it calls a class that does not exist, :996; ShapeReader serves
    the land mask), +proj=ob_tran, set_convolution_kernel (the reference's __convolve_block__ convolves node lists as if they
    were images), ensemble lists, more than 128 vertical levels.  The valid range of a standard name (:632-642) is not applied:
    no reader of this package applies one."""
    device_kind = 'schism'
    STATIC_VARIABLES = ('sea_floor_depth_below_sea_level', 'land_binary_mask')      # :478

    def __init__(self, x, y, times, node_arrays, zcor=None, proj4=None, use_3d=None, name='schism_reader'):
        self.proj4 = '+proj=latlong' if proj4 is None else proj4
        self.name = name
        pd = projection.parse_proj4(self.proj4)        # NotImplementedError: not on the device path
        if pd.get('kind') == 'ob_tran':
            raise NotImplementedError('a mesh on a rotated pole (+proj=ob_tran) is not on the device path')
        self.x, self.y = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y))
        N = len(self.x)
        if len(self.y) != N:
            raise ValueError('%d x and %d y node coordinates' % (N, len(self.y)))
        if N < 3:
            raise ValueError('a mesh of %d nodes: a value is the mean over the three nearest' % N)
        if not (np.isfinite(self.x).all() and np.isfinite(self.y).all()):
            raise ValueError('a mesh coordinate is not finite')
        self.xmin, self.xmax, self.ymin, self.ymax = float(self.x.min()), float(self.x.max()), float(self.y.min()), float(self.y.max())
        self.times = list(times) if times is not None else []
        if not self.times:
            raise ValueError('times must hold at least one time level')
        if any(b <= a for a, b in zip(self.times, self.times[1:])):
            raise ValueError('times must increase')
        self.start_time, self.end_time = self.times[0], self.times[-1]
        self.time_step = (self.times[1] - self.times[0]) if len(self.times) > 1 else None
        nt = len(self.times)
        self.node_arrays = {}
        for v, a in (node_arrays or {}).items():
            if v == 'land_binary_mask':
                raise NotImplementedError('land_binary_mask on a SCHISM mesh: the reference interpolates it with a class that does not '
                                          'exist (Nearest2DInterpolator); ShapeReader serves the land mask')
            if isinstance(a, (list, tuple)):
                raise NotImplementedError('ensemble members (%s) on a SCHISM mesh are not built' % v)
            a = np.ascontiguousarray(np.ma.filled(np.ma.asarray(a, dtype=np.float32), np.nan), dtype=np.float32)
            if not (a.shape == (N,) or (a.ndim in (2, 3) and a.shape[:2] == (nt, N))):
                raise ValueError('variable %s of shape %s: expected [%d], [%d, %d] or [%d, %d, levels]' % (v, a.shape, N, nt, N, nt, N))
            self.node_arrays[v] = a
        levels = sorted({a.shape[2] for a in self.node_arrays.values() if a.ndim == 3})
        if len(levels) > 1:
            raise ValueError('the 3-D variables disagree on the number of vertical levels: %s' % levels)
        self.n_levels = levels[0] if levels else 0
        if self.n_levels > _abi.SCHISM_MAX_VERTICAL:
            raise NotImplementedError('%d vertical levels: the device columns hold at most %d (UMESH_MAXSIGMA)' % (self.n_levels, _abi.SCHISM_MAX_VERTICAL))
        three_d = [v for v, a in self.node_arrays.items() if a.ndim == 3]
        self.use_3d = use_3d
        if self.use_3d is None:      # :129-134
            self.use_3d = bool(three_d) and zcor is not None
        if self.use_3d and three_d and zcor is None:      # :136-143
            raise ValueError('variable zcor must be present to be able to use 3D currents')
        self.geographic = pd.get('kind', 'latlong') == 'latlong' or not (self.x > 360.).any()      # :246; a latlong proj4 decides too
        if self.geographic and self.use_3d:      # :246-248
            self.use_3d = False
        if three_d and not self.use_3d:
            raise NotImplementedError('3-D variables %s on a reader that does not use 3-D data (%s): give depth-averaged [nt, N] arrays'
                                      % (sorted(three_d), 'a geographic mesh: metres and degrees do not make one distance'
                                         if self.geographic else 'use_3d is off, or zcor is missing'))
        self.zcor = None
        if self.use_3d and three_d:
            z = np.array(np.ma.filled(np.ma.asarray(zcor, dtype=np.float32), np.nan), dtype=np.float32, order='C')
            if z.shape != (nt, N, self.n_levels):
                raise ValueError('zcor of shape %s: expected [%d, %d, %d]' % (z.shape, nt, N, self.n_levels))
            z[np.isinf(z)] = np.float32(15.0)      # :942-943
            short = [k for k in range(nt) if np.isfinite(z[k]).sum() < 3]
            if short:
                raise ValueError('time level %d of zcor holds fewer than three finite entries: a value is the mean over the three '
                                 'nearest points' % short[0])
            self.zcor = z
        self.variables = list(self.node_arrays)
        from scipy.spatial import ConvexHull      # Qhull, as the reference (_build_boundary_polygon_)
        ring = ConvexHull(np.c_[self.x, self.y]).vertices
        self.hull_x, self.hull_y = np.ascontiguousarray(self.x[ring]), np.ascontiguousarray(self.y[ring])
        self._hull = ShapeReader([np.c_[self.hull_x, self.hull_y]], proj4_str=self.proj4)      # its crossing rule, its box
        self._tree2, self._trees3 = None, {}
        super().__init__()

    nearest_time = UnstructuredReader.nearest_time
    rotation_angle = UnstructuredReader.rotation_angle
    modulate_longitude = UnstructuredReader.modulate_longitude

    def set_convolution_kernel(self, convolve):
        raise NotImplementedError('set_convolution_kernel on a SCHISM mesh: the reference\'s __convolve_block__ convolves node lists as '
                                  'if they were images')

    def levels_of(self, variable):
        """Vertical levels of a variable's array (0: a 2-D variable); ValueError when the reader does not have it."""
        if variable not in self.node_arrays:
            raise ValueError('Variable not available: %s\nAvailable parameters are: %s' % (variable, self.variables))
        a = self.node_arrays[variable]
        return a.shape[2] if a.ndim == 3 else 0

    def level(self, variable, k):
        """The array of time level k: [N] or [N, L]."""
        self.levels_of(variable)
        a = self.node_arrays[variable]
        return a if a.ndim == 1 else a[k]

    def covers_positions(self, x, y):
        """Strictly inside the convex hull of the nodes, by ShapeReader's rule; x + y not finite is outside."""
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
        xmin, xmax, ymin, ymax = self._hull.box
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(x + y) & (x >= xmin) & (x <= xmax) & (y >= ymin) & (y <= ymax)
        if ok.any():
            ok[ok] = self._hull.contains(x[ok], y[ok])
        return ok

    def cloud(self, k):
        """(x_3d, y_3d, z_3d) of time level k: node x level flattened with the masked entries removed (convert_3d_to_array)."""
        keep = ~np.isnan(self.zcor[k])
        return np.repeat(self.x, self.n_levels).reshape(keep.shape)[keep], np.repeat(self.y, self.n_levels).reshape(keep.shape)[keep], \
            self.zcor[k][keep]

    def nearest3(self, x, y, z=None, k=0):
        """(dist [n, 3], idx [n, 3]) of scipy's cKDTree.query(..., 3) over the nodes (z None) or over the cloud of time level k."""
        from scipy.spatial import cKDTree
        if z is None:
            if self._tree2 is None:
                self._tree2 = cKDTree(np.vstack((self.x, self.y)).T)
            return self._tree2.query(np.vstack((x, y)).T, 3)
        if k not in self._trees3:
            if len(self._trees3) >= 4:
                self._trees3.clear()
            self._trees3[k] = cKDTree(np.vstack(self.cloud(k)).T)
        return self._trees3[k].query(np.vstack((x, y, z)).T, 3)

    def interpolate_level(self, variables, k, x, y, z):
        """ReaderBlockUnstruct.interpolate for time level k: {variable: float64 values} at positions in mesh coordinates.  A
        position or depth that is not finite has no neighbours: NaN."""
        x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
        out, found = {}, {}
        for v in variables:
            L = self.levels_of(v)
            fin = np.isfinite(x + y + z) if L else np.isfinite(x + y)
            if bool(L) not in found:
                found[bool(L)] = self.nearest3(x[fin], y[fin], z[fin] if L else None, k)
            dist, i = found[bool(L)]
            dist = dist.copy()
            dist[dist < 1.e-10] = 1.e-10
            fac = 1. / dist
            data = self.level(v, k)
            if L:
                data = data[~np.isnan(self.zcor[k])]
            out[v] = np.full(len(x), np.nan)
            out[v][fin] = (fac * data.take(i)).sum(-1) / fac.sum(-1)
        return out

    def get_variables_interpolated(self, variables, time, lon, lat, z, rotate=True):
        """What the device launch gives an element with an empty slot, on the host: {variable: float32}; NaN outside the hull or
        outside the time coverage; vector pairs rotated to east / north unless the mesh is geographic."""
        lon, lat = np.atleast_1d(np.asarray(lon, dtype=np.float64)), np.atleast_1d(np.asarray(lat, dtype=np.float64))
        n = len(lon)
        variables = list(variables)
        out = {v: np.full(n, np.nan, np.float32) for v in variables}
        for v in variables:
            self.levels_of(v)
        if not self.covers_time(time):
            return out
        latlong = projection.parse_proj4(self.proj4).get('kind', 'latlong') == 'latlong'
        x, y = (self.modulate_longitude(lon), lat) if latlong else self.lonlat2xy(lon, lat)
        return self.get_variables(variables, time, x, y, z, rotate=rotate)

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None, rotate=True):
        """The same at positions x, y in the mesh's own coordinates (what a host-evaluated reader is asked)."""
        variables = [requested_variables] if isinstance(requested_variables, str) else list(requested_variables)
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
        n = len(x)
        out = {v: np.full(n, np.nan, np.float32) for v in variables}
        for v in variables:
            self.levels_of(v)
        time = self.start_time if time is None else time
        if not self.covers_time(time):
            return out
        z = 0.0 if z is None else z
        latlong = projection.parse_proj4(self.proj4).get('kind', 'latlong') == 'latlong'
        ok = self.covers_positions(x, y)
        if not ok.any():
            return out
        zz = np.broadcast_to(np.asarray(z, dtype=np.float64), (n,))[ok]
        kb, ka, w = self.time_weight(time, variables)
        env = self.interpolate_level(variables, kb, x[ok], y[ok], zz)
        if ka is not None:
            after = self.interpolate_level(variables, ka, x[ok], y[ok], zz)
            # (a masked array from here on: __check_variable_array__ stores it as float32)
            env = {v: (env[v] * (1 - w) + after[v] * w).astype(np.float32) for v in variables}
        if rotate and not latlong:
            for vx, vy in VECTOR_PAIRS_XY:
                if vx in env and vy in env:
                    rot = self.rotation_angle(x[ok], y[ok])
                    u, w_ = env[vx], env[vy]
                    env[vx], env[vy] = u * np.cos(rot) - w_ * np.sin(rot), u * np.sin(rot) + w_ * np.cos(rot)
        for v in variables:
            out[v][ok] = env[v]
        return out

    def time_weight(self, time, variables):
        """(index before, index after or None, weight_after) of _get_variables_interpolated_ :472-481, :618-620: no blend at a
        level exactly, with one level only, or when every requested variable is static."""
        _, t_before, t_after, _, kb, ka = self.nearest_time(time)
        if t_after is None or time == t_before or all(v in self.STATIC_VARIABLES for v in variables):
            return kb, None, 0.0
        return kb, ka, (time - t_before).total_seconds() / (t_after - t_before).total_seconds()


def _polygon_rings(geom):
    """[[exterior, hole, ...], ...] of one entry of ShapeReader's `polygons`: an (n, 2) array, a pair (exterior, [holes]), or
    anything with the __geo_interface__ / GeoJSON shape of a Polygon or MultiPolygon (a Feature is unwrapped)."""
    g = getattr(geom, '__geo_interface__', geom)
    if isinstance(g, dict):
        if g.get('type') == 'Feature':
            return _polygon_rings(g['geometry'])
        if g.get('type') == 'Polygon':
            return [[r for r in g['coordinates']]]
        if g.get('type') == 'MultiPolygon':
            return [[r for r in poly] for poly in g['coordinates']]
        raise ValueError('a geometry of type %r: ShapeReader takes Polygon and MultiPolygon' % (g.get('type'),))
    if isinstance(g, (tuple, list)) and len(g) == 2 and np.ndim(g[0]) == 2 and not np.isscalar(g[1]) and \
            (len(g[1]) == 0 or np.ndim(g[1][0]) == 2):
        return [[g[0]] + list(g[1])]
    return [[g]]


def _ring_edges(ring):
    """(x1, y1, x2, y2) of the edges of one ring: closed if it is open, edges of zero length dropped."""
    a = np.asarray(ring, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError('a ring must be an (n, 2) array of vertices, got shape %s' % (a.shape,))
    a = a[:, :2]
    if not np.isfinite(a).all():
        raise ValueError('a ring has a coordinate that is not finite')
    if len(np.unique(a, axis=0)) < 3:
        raise ValueError('a ring of fewer than three distinct vertices')
    b = np.roll(a, -1, axis=0)
    keep = (a[:, 0] != b[:, 0]) | (a[:, 1] != b[:, 1])
    return a[keep, 0], a[keep, 1], b[keep, 0], b[keep, 1]


class ShapeReader(ContinuousReader):
    """reader_shape.Reader (readers/reader_shape.py): land_binary_mask from coastline polygons, given as arrays.  A point is on
    land when any polygon contains it; a polygon contains a point inside its exterior ring and inside none of its holes;
    polygons may overlap, an island in a lake is a polygon of its own.  invert=True: 1 - contains (:106-110).

    polygons: a sequence of (n, 2) arrays (one ring), pairs (exterior, [hole, ...]) and objects or dicts with the
    __geo_interface__ / GeoJSON shape of a Polygon or MultiPolygon (shapely geometries), mixed.  Rings may be closed or open, in
    either orientation.  Coordinates are in the CRS `proj4_str`.

    On the device (`device_kind = 'shape'`) the whole lookup of a get_environment call -- projection, coverage box, an exact
    crossing-number test behind a uniform grid, invert, merge by priority -- is one launch (odr_shape_sample).
    `get_variables` answers on the host with the same rule over all edges.  A point exactly on a ring is outside for shapely;
    here it falls on whichever side the half-open crossing rule puts it.  `from_shpfiles` is not built."""
    device_kind = 'shape'
    name = 'shape'
    variables = ['land_binary_mask']
    always_valid = True

    def __init__(self, polygons, proj4_str='+proj=lonlat +ellps=WGS84', invert=False, land_buffer_distance=None):
        self._land_kdtree = None
        self._land_kdtree_buffer_distance = land_buffer_distance
        self.invert = bool(invert)
        self.proj4 = proj4_str
        pd = projection.parse_proj4(proj4_str)        # NotImplementedError: not on the device path
        if pd.get('kind') == 'ob_tran':
            raise NotImplementedError('polygons on a rotated pole (+proj=ob_tran) are not on the device path')
        self.polys = [rings for g in list(polygons) for rings in _polygon_rings(g)]
        if len(self.polys) == 0:
            raise AssertionError('no geometries loaded')      # (the reference's assert, reader_shape.py:97)
        parts, ids = [], []
        for k, rings in enumerate(self.polys):
            for ring in rings:
                e = _ring_edges(ring)
                parts.append(e)
                ids.append(np.full(len(e[0]), k, np.int32))
        self.x1, self.y1, self.x2, self.y2 = (np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(4))
        self.poly = np.ascontiguousarray(np.concatenate(ids))
        self.n_polygons = len(self.polys)
        super().__init__()
        xmin, xmax, ymin, ymax = float(self.x1.min()), float(self.x1.max()), float(self.y1.min()), float(self.y1.max())
        self.box = (xmin, xmax, ymin, ymax)      # of the rings, in their own coordinates: the coverage the device tests
        if pd.get('kind', 'latlong') == 'latlong':      # reader_shape.py:102-104: the bounds through lonlat2xy (the identity here)
            (self.xmin, self.ymin), (self.xmax, self.ymax) = (float(v) for v in self.lonlat2xy(xmin, ymin)), \
                (float(v) for v in self.lonlat2xy(xmax, ymax))
        else:      # (the reference hands projected bounds to lonlat2xy, which gives no box at all: the rings' own box here)
            self.xmin, self.xmax, self.ymin, self.ymax = self.box

    def modulate_longitude(self, lon):      # variables.py:259-280, for geographic polygons
        lon = np.asarray(lon, dtype=np.float64)
        return np.mod(lon + 180, 360) - 180 if self.box[0] < 0 else np.mod(lon, 360)

    def contains(self, x, y, chunk=1 << 14):
        """The definition, over all edges (csrc/odr_shape.hip.h): per polygon the parity of its edges with (y1 > py) != (y2 > py)
        and x1 + (py - y1) * (x2 - x1) / (y2 - y1) < px; the OR over the polygons.  bool per point."""
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel(), np.atleast_1d(np.asarray(y, dtype=np.float64)).ravel()
        out = np.zeros(len(x), bool)
        first = np.r_[0, np.flatnonzero(np.diff(self.poly)) + 1]      # the edges are grouped by polygon
        step = max(1, chunk * 64 // max(len(self.x1), 1))
        with np.errstate(divide='ignore', invalid='ignore'):
            for o in range(0, len(x), step):
                px, py = x[o:o + step, None], y[o:o + step, None]
                cross = ((self.y1 > py) != (self.y2 > py)) & (self.x1 + (py - self.y1) * (self.x2 - self.x1) / (self.y2 - self.y1) < px)
                out[o:o + step] = (np.add.reduceat(cross, first, axis=1) & 1).any(axis=1)
        return out

    def _on_land(self, x, y):
        c = self.contains(x, y)
        return 1 - c if self.invert else c

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        """{'land_binary_mask': 1 / 0 per position (x, y) in the reader's coordinates} -- for every position, covered or not (the
        caller masks, as the reference's does)."""
        if isinstance(requested_variables, str):
            requested_variables = [requested_variables]
        for v in requested_variables:
            if v not in self.variables:
                raise ValueError('Variable not available: %s\nAvailable parameters are: %s' % (v, self.variables))
        shape = np.shape(x)
        return {'x': x, 'y': y, 'land_binary_mask': np.reshape(self._on_land(x, y), shape)}

    def mask(self, lon, lat):
        """What the device launch gives an element with an empty slot, on the host: float32 1 / 0, NaN outside the box."""
        lon, lat = np.atleast_1d(np.asarray(lon, dtype=np.float64)), np.atleast_1d(np.asarray(lat, dtype=np.float64))
        geographic = projection.parse_proj4(self.proj4).get('kind', 'latlong') == 'latlong'
        x, y = (self.modulate_longitude(lon), lat) if geographic else self.lonlat2xy(lon, lat)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(x + y) & (x >= self.box[0]) & (x <= self.box[1]) & (y >= self.box[2]) & (y <= self.box[3])
        out = np.full(len(lon), np.nan, np.float32)
        if ok.any():
            out[ok] = self._on_land(x[ok], y[ok])
        return out

    def boundary_vertices(self):
        """(x, y) of the vertices of all rings (reader_shape.py `unwrap` of the polygons' boundaries)."""
        return self.x1, self.y1

    def get_nearest_outside(self, x, y, buffer_distance=None, nearest=None):
        """reader_shape.py:132-159 for buffer_distance None or 0: (x, y, distance) of the boundary vertex nearest to each point.
        nearest: a function (vx, vy, qx, qy) -> indices (the model passes the device's exact k-d tree); default scipy's cKDTree."""
        if buffer_distance not in (None, 0):
            raise NotImplementedError('get_nearest_outside with a buffer distance of %r: polygon offsetting is not built' % (buffer_distance,))
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
        vx, vy = self.boundary_vertices()
        if nearest is None:
            if self._land_kdtree is None:
                from scipy.spatial import cKDTree
                self._land_kdtree = cKDTree(np.c_[vx, vy])
            ind = self._land_kdtree.query(np.c_[x, y])[1]
        else:
            ind = np.asarray(nearest(vx, vy, x, y), dtype=np.int64)
        return vx[ind], vy[ind], np.sqrt((vx[ind] - x) ** 2 + (vy[ind] - y) ** 2)


class TimeseriesReader(ContinuousReader):
    """reader_timeseries.Reader (readers/reader_timeseries.py): {'time': [datetimes], variable: [values], 'lon': , 'lat': } -- the value
    of the nearest time level, the same everywhere.  `lon` / `lat` are kept as attributes (the centre of the measurement for
    combine_gaussian), not as variables.  Added to a model on its own it is evaluated on the host like any user-defined
    ContinuousReader; as a leaf of a reader expression it is one scalar per variable and call (a uniform leaf of the device
    program)."""

    def __init__(self, parameter_value_map):
        m = dict(parameter_value_map)
        self.times = m.pop('time')
        if not hasattr(self.times, '__len__'):
            raise ValueError('time must be an array of datetime objects')
        self.times = list(self.times)
        for key in ('lon', 'lat'):
            if key in m:
                setattr(self, key, m.pop(key))
        for key in m:
            m[key] = np.atleast_1d(m[key]).astype(np.float64)
            if len(m[key]) != len(self.times):
                raise ValueError('All variables must have same length as time array')
        self._parameter_value_map = m
        self.variables = list(m)
        self.proj4 = '+proj=latlong'
        self.xmin, self.xmax, self.ymin, self.ymax = -180, 180, -90, 90
        self.start_time, self.end_time = self.times[0], self.times[-1]
        self.time_step = (self.times[1] - self.times[0]) if len(self.times) > 1 else None
        self.name = 'reader_timeseries'
        times = self.times
        super().__init__()
        self.times = times

    def nearest_index(self, time):
        """indx_nearest of variables.py:402-443 from the bracketing levels of BaseReader.nearest_time; midway: the later."""
        ib, ia = self.nearest_time(time)
        return ib if (time - self.times[ib]) < (self.times[ia] - time) else ia

    def value(self, variable, time):
        return float(self._parameter_value_map[variable][self.nearest_index(time)])

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        out = {'time': time, 'x': x, 'y': y, 'z': z}
        for v in requested_variables:
            out[v] = self.value(v, time) * np.ones(np.shape(x))
        return out


def _none_or(a, b, cmp):      # readerops.py:7-13
    return b if a is None else a if b is None else cmp(a, b)


class CombinedReader(BaseReader):
    """readerops.Combined (readers/operators/readerops.py): `a + b`, or a.combine_gaussian(b, std).  It is a reader, so it nests:
    (r1 + r2) + r1.  variables: those both operands have (in a's order); start_time the later, end_time the earlier of the two;
    covers_time the AND.  The result is missing wherever an operand is, and there are no vertical profiles (the reference's
    get_variables_interpolated does not forward `profiles`).  It does not forward `rotate_to_proj` either: the operands' vector
    pairs are NOT rotated to east / north, the components of a projected grid are added along the grid's own axes
    (readerops.py:84-101; tools/gen_golden_reader_ops.py records it) -- and so they are here.

    In a model (`device_kind = 'combined'`) every call of get_environment is one launch over the flattened expression
    (odr_combined_sample); get_variables_interpolated is the NumPy evaluation for expressions whose leaves are all
    ContinuousReaders."""
    device_kind = 'combined'

    def __init__(self, a, b, kind='add', std=None):
        self.a, self.b, self.kind, self.std = a, b, kind, std
        others = list(b) if isinstance(b, (list, tuple)) else [b]
        if kind == 'gaussian' and isinstance(b, (list, tuple)):
            raise NotImplementedError('combine_gaussian with a list of measurement readers: the reference\'s list form could not be '
                                      'run for a known answer (tools/gen_golden_reader_ops.py); blend towards one measurement reader')
        if kind == 'gaussian':
            for r in others:
                if not (isinstance(r, TimeseriesReader) and hasattr(r, 'lon') and hasattr(r, 'lat')):
                    raise TypeError('combine_gaussian: the measurement reader must be a TimeseriesReader with lon and lat')
            stds = np.atleast_1d(np.asarray(std, dtype=np.float64))
            if len(stds) not in (1, len(others)) or not (np.isfinite(stds).all() and (stds > 0).all()):
                raise ValueError('combine_gaussian: std must be a positive number, or one per measurement reader')
            self.stds = [float(stds[k if len(stds) > 1 else 0]) for k in range(len(others))]
        elif kind != 'add' or isinstance(b, (list, tuple)):
            raise TypeError('readers are combined with + or combine_gaussian')
        self.variables = [v for v in a.variables if all(v in r.variables for r in others)]
        self.start_time, self.end_time = a.start_time, a.end_time
        for r in others:
            self.start_time = _none_or(self.start_time, r.start_time, max)
            self.end_time = _none_or(self.end_time, r.end_time, min)
        self.name = 'Combined(%s | %s)' % (a.name, b.name)
        self.xmin, self.xmax, self.ymin, self.ymax = -180, 180, -90, 90
        self.proj4 = '+proj=latlong'
        super().__init__()

    def _others(self):
        return list(self.b) if isinstance(self.b, (list, tuple)) else [self.b]

    def covers_time(self, time):
        return all(r.covers_time(time) for r in [self.a] + self._others())

    def get_variables_interpolated(self, variables, profiles=None, profiles_depth=None, time=None, lon=None, lat=None, z=None,
                                   rotate_to_proj=None):
        assert set(variables).issubset(self.variables), '%s is not subset of %s' % (variables, self.variables)
        env_a, _ = _interpolated(self.a, variables, time, lon, lat, z)
        env_b = [_interpolated(r, variables, time, lon, lat, z)[0] for r in self._others()]
        env = {}
        for v in variables:
            if self.kind == 'add':
                env[v] = env_a[v] + env_b[0][v]
            else:
                f = np.stack([gaussian_factor(lon, lat, r.lon, r.lat, s) for r, s in zip(self._others(), self.stds)])
                env[v] = env_a[v] * (1 - np.sum(f, axis=0)) + np.sum(np.stack([e[v] for e in env_b]) * f, axis=0)
        return env, None


def gaussian_factor(lon, lat, lon_center, lat_center, std):
    """exp(-(d / std)^2 / 2), d the WGS84 distance to the centre (ops.py:59-94; wgs84_distance)."""
    lon, lat = np.broadcast_arrays(np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64))
    d = wgs84_distance(lon, lat, float(lon_center), float(lat_center))
    return np.exp(-np.power(d / float(std), 2.) / 2)


def _interpolated(reader, variables, time, lon, lat, z):
    if not hasattr(reader, 'get_variables_interpolated') or isinstance(reader, StructuredReader):
        raise NotImplementedError('reader %s is evaluated on the device only: the host evaluation of a reader expression takes '
                                  'ContinuousReaders as leaves' % reader.name)
    return reader.get_variables_interpolated(variables, time=time, lon=lon, lat=lat, z=z)


class NumCombinedReader:
    """numops.Combined (readers/operators/numops.py): a reader combined with a number -- n + r, n * r, r / n (r - n is r + (-n)).
    It is NOT a reader and has no operators of its own, so it is always the root of an expression; everything else is forwarded
    to its reader.  On the device the result is float64 whatever the operand's class: the reference's operand is a masked array,
    whose arithmetic makes a 0-d float64 array of the number (tools/gen_golden_reader_ops.py)."""
    device_kind = 'combined'

    def __init__(self, n, r, op, descop='|'):
        assert isinstance(n, Number)
        assert isinstance(r, BaseReader)
        self.n, self.r, self.op = n, r, op
        self.name = 'NumCombined(%s %s %s)' % (r.name, descop, n)

    @staticmethod
    def add(n, r):
        return NumCombinedReader(n, r, 'add', '+')

    @staticmethod
    def mul(n, r):
        return NumCombinedReader(n, r, 'mul', '*')

    @staticmethod
    def div(n, r):
        return NumCombinedReader(n, r, 'div', '/')

    def __getattr__(self, attr):
        if attr in ('n', 'r', 'op'):      # (not set yet: no forwarding loop)
            raise AttributeError(attr)
        return getattr(self.r, attr)

    def apply(self, x):
        return self.n + x if self.op == 'add' else self.n * x if self.op == 'mul' else x / self.n

    def get_variables_interpolated(self, variables, *args, **kwargs):
        assert set(variables).issubset(self.r.variables), '%s is not a subset of variables in %s' % (variables, self.r.name)
        env, _ = self.r.get_variables_interpolated(variables, *args, **kwargs)
        return {v: self.apply(env[v]) for v in variables}, None


class FilteredReader(ReaderOperators):
    """filter.FilterVariables (readers/operators/filter.py): a reader of which only some variables are forwarded."""
    device_kind = 'combined'

    def __init__(self, r, vars):
        vars = list(vars)
        assert set(vars).issubset(r.variables), '%s is not a subset of variables in %s' % (vars, r.name)
        self.r, self.v = r, vars
        self.name = 'Filter(%s | %s)' % (r.name, vars)

    @property
    def variables(self):
        return self.v

    def __getattr__(self, attr):
        if attr in ('r', 'v'):
            raise AttributeError(attr)
        return getattr(self.r, attr)


def expression_postfix(reader):
    """The expression in postfix, as the device program has it: [(kind, payload, (d0, d1, d2))] with kind one of _abi.COMBINE_* and
    payload the leaf reader of a SOURCE / UNIFORM / GAUSS_TERM entry."""
    if isinstance(reader, NumCombinedReader):
        kind = {'add': _abi.COMBINE_NUM_ADD, 'mul': _abi.COMBINE_NUM_MUL, 'div': _abi.COMBINE_NUM_DIV}[reader.op]
        return expression_postfix(reader.r) + [(kind, None, (float(reader.n), 0.0, 0.0))]
    if isinstance(reader, FilteredReader):
        return expression_postfix(reader.r)
    if isinstance(reader, CombinedReader):
        if reader.kind == 'add':
            return expression_postfix(reader.a) + expression_postfix(reader.b) + [(_abi.COMBINE_ADD, None, (0.0, 0.0, 0.0))]
        return expression_postfix(reader.a) + [(_abi.COMBINE_GAUSS_TERM, r, (float(r.lon), float(r.lat), s))
                                               for r, s in zip(reader._others(), reader.stds)] + \
            [(_abi.COMBINE_GAUSS_END, None, (0.0, 0.0, 0.0))]
    if isinstance(reader, TimeseriesReader):
        return [(_abi.COMBINE_UNIFORM, reader, (0.0, 0.0, 0.0))]
    return [(_abi.COMBINE_SOURCE, reader, (0.0, 0.0, 0.0))]


def expression_depth(postfix):
    """The most values the program holds at once."""
    depth = deepest = 0
    for kind, _, _ in postfix:
        depth += 1 if kind in (_abi.COMBINE_SOURCE, _abi.COMBINE_UNIFORM) else -1 if kind == _abi.COMBINE_ADD else 0
        deepest = max(deepest, depth)
    return deepest


def check_device_expression(reader):
    """NotImplementedError, with the reason, for an expression the device program does not take."""
    name = reader.name
    post = expression_postfix(reader)
    for kind, r, _ in post:
        if kind != _abi.COMBINE_SOURCE:
            continue
        dk = getattr(r, 'device_kind', None)
        if dk in ('umesh', 'shape'):
            raise NotImplementedError('reader expression %s: operators on a mesh or shape reader (%s) are not built' % (name, r.name))
        if dk == 'schism':
            raise NotImplementedError('reader expression %s: operators on a SchismReader (%s) are not built' % (name, r.name))
        if dk is None and isinstance(r, ContinuousReader):
            raise NotImplementedError('reader expression %s: leaf %s is a ContinuousReader evaluated on the host; the device '
                                      'program takes gridded, constant, analytic, landmask and timeseries readers' % (name, r.name))
        if dk is None and not isinstance(r, StructuredReader):
            raise NotImplementedError('reader expression %s: leaf %s is no reader the device can sample' % (name, r.name))
        if any(isinstance(a, (list, tuple)) for a in getattr(r, 'arrays', {}).values()):
            raise NotImplementedError('reader expression %s: leaf %s hands out ensemble members' % (name, r.name))
    if expression_depth(post) > _abi.COMBINE_STACK:
        raise NotImplementedError('reader expression %s is deeper than the device program supports: it would hold %d values at once, '
                                  'at most %d fit (an accumulator and two saved temporaries)' % (name, expression_depth(post), _abi.COMBINE_STACK))
    if len(post) > _abi.COMBINE_MAX_OPS:
        raise NotImplementedError('reader expression %s has %d operations, at most %d fit' % (name, len(post), _abi.COMBINE_MAX_OPS))
    uniform = {id(r) for kind, r, _ in post if kind in (_abi.COMBINE_UNIFORM, _abi.COMBINE_GAUSS_TERM)}
    if len(uniform) > _abi.COMBINE_MAX_UNIFORM:
        raise NotImplementedError('reader expression %s has %d timeseries readers, at most %d fit' % (name, len(uniform), _abi.COMBINE_MAX_UNIFORM))
    return post


def _dev(a):
    """a block array as Context.upload_block_device wants it: the device pointer of a CUDA tensor, else the host array"""
    return int(a.data_ptr()) if hasattr(a, 'is_cuda') and a.is_cuda else a


class ReaderLevelsError(RuntimeError):
    """The time levels one step needs do not fit the device slots: a configuration error of the run, NOT a reader
    failure (the model's reader-failure handling must not swallow it and fall back to constants silently)."""


_READER_IO_LOCK = threading.Lock()   # one get_variables at a time, whichever thread: netCDF / HDF5 builds are rarely thread-safe


class _ShapeOnly:
    """A variable of a reader level on a rank that does not hold the arrays (they arrive by odr_block_broadcast)."""

    def __init__(self, shape):
        self.shape = tuple(int(n) for n in shape)


class ReadAhead:
    """Rank 0 of a sharded run owns the host Reader: every time level the other ranks receive passes through ITS
    get_variables.  Called inline it stops rank 0's step loop for the duration of the file read, and -- one collective per
    step -- every other rank with it.  This runs the read of the level that comes NEXT on a worker thread as soon as a
    level has been handed out; when the level is due (one period later: _prefetch_dist starts its broadcast) the block is
    there.  The reference reads inline in its single process (basereader/structured.py:121-170); the block is the same
    object either way.  A read-ahead for another level or window than the one asked for is waited for and dropped."""

    def __init__(self, reader, variables):
        self.reader, self.variables = reader, list(variables)
        self._pool, self._fut, self._key = None, None, None
        self.hits = self.misses = 0
        self.worker_s = 0.0          # time the worker spent inside get_variables (off the step loop)

    @staticmethod
    def _key_of(k, x, y):
        return (int(k), None if x is None else (np.asarray(x).tobytes(), np.asarray(y).tobytes()))

    def _get(self, k, x, y, timed=False):
        import time as _time
        r = self.reader
        t = r.times[k] if r.times is not None else None
        t0 = _time.perf_counter()
        with _READER_IO_LOCK:
            block = r.get_variables(self.variables, t, x, y, np.array([0.0]))
        if timed:
            self.worker_s += _time.perf_counter() - t0
        return block

    def start(self, k, x, y):
        """Begin reading level k on the worker (returns at once)."""
        if self._fut is not None:
            return
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='odr-reader')
        self._key = self._key_of(k, x, y)
        self._fut = self._pool.submit(self._get, k, x, y, True)

    def read(self, k, x, y):
        """The block of level k: the worker's if it was read ahead (its exception is raised here, where an inline read
        would have raised it), an inline read otherwise."""
        fut, key = self._fut, self._key
        self._fut = self._key = None
        if fut is not None:
            if key == self._key_of(k, x, y):
                self.hits += 1
                return fut.result()
            try:
                fut.result()
            except Exception:      # noqa: BLE001 -- of a level nobody asked for
                pass
        self.misses += 1
        return self._get(k, x, y)

    def close(self):
        """Waits for a read in flight (its exception, of a level nobody will ask for, is logged, not raised) and ends the worker."""
        fut, self._fut, self._key = self._fut, None, None
        if fut is not None:
            try:
                fut.result()
            except Exception as e:      # noqa: BLE001
                import logging
                logging.getLogger(__name__).debug('read-ahead of a level that is no longer wanted failed: %r', e)
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None


class DeviceReaderBinding:
    """Device image of one reader: constant/analytic source, or a grid source whose time levels
    (ReaderBlocks) are uploaded on demand.  Stands where StructuredReader keeps
    var_block_before/after (structured.py:121-123)."""
    NSLOTS = 6        # = MAXLEVELS of the device source: t0, t0 + dt/2 and t0 + dt may each sit between two different levels
    PREFETCH = True   # stage the next time level on the upload stream while the current one is in use

    def __init__(self, ctx, reader, variables=None, shared=None):
        """shared: {id(reader): binding} of the bindings the model made for readers added on their own -- a reader expression
        samples a leaf that is among them through that binding (one source id, one set of resident levels)."""
        self.ctx, self.reader = ctx, reader
        self.variables = [v for v in (variables or reader.variables)]
        self.slots = {}      # time index -> slot
        self.staged = {}     # time index -> slot uploaded asynchronously, not yet committed
        self.prefetch = self.PREFETCH
        self._pinned = False
        from .distributed import env_world
        self.rank, _, self.world = env_world()
        self.stall_s = 0.0             # host time spent waiting for a level that was due (run().timing reports the sum)
        self._dist_pre = {}            # sharded run: time index -> (tensors, works) of a level whose broadcast is under way
        self._ahead, self._ahead_last = None, None   # sharded run, rank 0: the next level read on a worker thread (ReadAhead)
        self.mesh = None               # device.UMesh of an UnstructuredReader
        self.shape = None              # device.Shape of a ShapeReader
        self.leaves = None             # a reader expression: [(leaf reader, its binding, made here and not shared)]
        kind = getattr(reader, 'device_kind', None)
        # a ContinuousReader the device has no closed form for (a user's analytic or point-wise reader,
        # basereader/continuous.py:20-46): evaluated on the host at the element positions, values uploaded
        self.host_eval = kind is None and isinstance(reader, ContinuousReader)
        if kind == 'constant':
            self.sid = ctx.add_constant({v: reader._parameter_value_map[v] for v in self.variables})
        elif kind == 'double_gyre':
            self.sid = ctx.add_double_gyre(A=reader.A, epsilon=reader.epsilon, omega=reader.omega,
                                           t0=_epoch(reader.initial_time))
            self.variables = ['x_sea_water_velocity', 'y_sea_water_velocity', 'land_binary_mask']
        elif kind == 'landmask':
            self.sid = ctx.add_landmask(reader.lon0, reader.lat0, reader.dlon, reader.dlat, reader.cells)
        elif kind == 'oscillating':
            self.sid = ctx.add_oscillating(reader.variables[0], reader.amplitude, reader.period_seconds,
                                           _epoch(reader.zero_time))
        elif kind == 'umesh':
            # an unstructured mesh is no source of the device's priority-list walk (sid stays None: _bind_variables and
            # set_extent leave it alone); the model samples it in a launch of its own behind that walk (sample_mesh)
            self.sid = None
            self.mesh = ctx.umesh(reader.x, reader.y, reader.xc, reader.yc, proj=projection.parse_proj4(reader.proj4),
                                  **{k: getattr(reader, k) for k in ('siglay', 'siglev', 'siglay_center', 'siglev_center', 'h', 'h_center')})
            self.mesh_slots = {}     # time index -> slot of the mesh (at most three resident)
        elif kind == 'schism':
            # as an unstructured mesh: no source of the priority-list walk, sampled in a launch of its own behind it (sample_mesh)
            self.sid = None
            self.mesh = ctx.schism(reader.x, reader.y, reader.hull_x, reader.hull_y, n_levels=reader.n_levels if reader.zcor is not None else 0,
                                   proj=projection.parse_proj4(reader.proj4))
            self.mesh_slots = {}     # time index -> slot of the mesh (at most four resident)
        elif kind == 'shape':
            # coastline polygons: as a mesh, sampled in a launch of its own behind the priority-list walk (sample_shape)
            self.sid = None
            self.shape = ctx.shape(reader.x1, reader.y1, reader.x2, reader.y2, reader.poly, reader.n_polygons,
                                   proj=projection.parse_proj4(reader.proj4), invert=reader.invert)
        elif kind == 'combined':
            # a reader expression (CombinedReader, NumCombinedReader, FilteredReader): no source of its own; every leaf the device
            # samples has a binding -- the model's, when the same reader object was also added on its own and delivers the
            # expression's variables, else one made here -- and the whole expression is one launch behind the priority-list
            # walk (sample_combined).  Timeseries leaves are resolved on the host, per call.
            self.sid = None
            self.host_eval = False
            self.postfix = check_device_expression(reader)
            self.leaves, self.program, self._program_key = [], None, None
            for op, leaf, _ in self.postfix:
                if op != _abi.COMBINE_SOURCE or any(leaf is r for r, _, _ in self.leaves):
                    continue
                b = (shared or {}).get(id(leaf))
                if b is not None and set(self.variables) <= set(b.variables):
                    self.leaves.append((leaf, b, False))
                else:
                    self.leaves.append((leaf, DeviceReaderBinding(ctx, leaf, variables=[v for v in leaf.variables if v in self.variables]), True))
            self.uniform = []            # the timeseries readers, in the order of their uniform-leaf index
            for op, leaf, _ in self.postfix:
                if op in (_abi.COMBINE_UNIFORM, _abi.COMBINE_GAUSS_TERM) and not any(leaf is r for r in self.uniform):
                    self.uniform.append(leaf)
        else:
            self.sid = None  # created with the first block (the grid comes with it)
        if kind and kind not in ('umesh', 'schism', 'shape', 'combined') and reader.start_time is not None:
            ctx.set_time_coverage(self.sid, _epoch(reader.start_time), _epoch(reader.end_time), reader.always_valid)

    def _static_ids(self):
        """{variable: content id} of the 2-D variables the reader declares time-invariant (`static_variables`): the same id
        for every level of this binding (a re-cut window is a new device source: its levels are all uploaded again)."""
        sv = [v for v in getattr(self.reader, 'static_variables', ()) if v in self.variables]
        if not sv:
            return None
        base = (id(self) & 0xffffff) * 4096
        return {v: base + 1 + self.variables.index(v) for v in sv}

    def is_grid(self):
        return getattr(self.reader, 'device_kind', None) is None and not self.host_eval

    def evaluate_on_host(self, variables, time, lon, lat, z, element_ID=None):
        """ContinuousReader._get_variables_interpolated_ (continuous.py:31-46): the reader's values exactly at the element
        positions; NaN where it does not cover (position or time).  A reader that maps values to element IDs
        (`_element_ID`, environment.py:621-623) is told the IDs of the positions it receives."""
        r = self.reader
        n = len(lon)
        out = {v: np.full(n, np.nan, np.float32) for v in variables}
        if not r.covers_time(time):
            return out
        x, y = r.lonlat2xy(lon, lat)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        ok = np.ones(n, bool)
        if r.xmin is not None:
            ok &= (x >= r.xmin) & (x <= r.xmax) & (y >= r.ymin) & (y <= r.ymax)
        ok &= (z >= r.zmin) & (z <= r.zmax)
        if ok.any():
            if getattr(r, '_element_ID', None) is not None and element_ID is not None:
                r._element_ID = np.asarray(element_ID)[ok]
            res = r.get_variables(list(variables), time, x[ok], y[ok], z[ok])
            for v in variables:
                out[v][ok] = np.asarray(np.ma.filled(res[v], np.nan), dtype=np.float32) * np.ones(int(ok.sum()), np.float32)
        return out

    def set_extent(self, lonlat_box):
        """Reader.prepare(extent, ...) (basereader/__init__.py, called from Environment.finalize :139-211): the lon / lat
        box the simulation can reach.  Blocks are then requested for that box only (+ the reader's buffer) instead of
        the reader's whole domain -- what makes a basin-scale model with many levels fit: every resident time level is
        cut to the same window.  Readers whose window would be most of their domain, readers without projection
        (whole-mesh lookup) and s-level readers keep whole-domain blocks."""
        r = self.reader
        self.extent = None
        self.extent_lonlat = None
        if not self.is_grid() or not getattr(r, 'projected', True) or getattr(r, 's_levels', False) or lonlat_box is None:
            return
        if not (hasattr(r, 'x') and np.ndim(r.x) == 1 and len(r.x) > 8 and len(r.y) > 8):
            return
        lo0, la0, lo1, la1 = [float(v) for v in lonlat_box]
        self.extent_lonlat = (lo0, la0, lo1, la1)
        x, y = self._box_outline_xy(lo0, la0, lo1, la1)
        if not (np.isfinite(x).all() and np.isfinite(y).all()):
            return
        xs, ys = np.asarray(r.x, dtype=np.float64), np.asarray(r.y, dtype=np.float64)
        fx = (min(x.max(), xs.max()) - max(x.min(), xs.min())) / (xs.max() - xs.min())
        fy = (min(y.max(), ys.max()) - max(y.min(), ys.min())) / (ys.max() - ys.min())
        if fx <= 0 or fy <= 0 or fx * fy > 0.6:
            return        # no overlap (nothing to cut) or most of the domain anyway
        self.extent = (np.array([x.min(), x.max()]), np.array([y.min(), y.max()]))

    def _box_outline_xy(self, lo0, la0, lo1, la1):
        """The outline of a lon / lat box in the reader's coordinates, 33 points per edge: on a polar-stereographic or
        Lambert grid the edges of such a box bulge in x / y, its corners alone underestimate the footprint."""
        t = np.linspace(0, 1, 33)
        lon = np.concatenate([lo0 + (lo1 - lo0) * t, lo0 + (lo1 - lo0) * t, np.full(33, lo0), np.full(33, lo1)])
        lat = np.concatenate([np.full(33, la0), np.full(33, la1), la0 + (la1 - la0) * t, la0 + (la1 - la0) * t])
        x, y = self.reader.lonlat2xy(lon, lat)
        return np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def outside_window(self, lon_min, lon_max, lat_min, lat_max, guard_lon, guard_lat):
        """Do the elements (their lon / lat box) come within `guard` of the window the blocks were cut to?  (The reference's
        Reader.prepare() does not shrink a reader's coverage: its blocks follow the elements.  Here every resident level is
        cut to ONE window for the run -- set_extent() -- so elements that outrun drift:max_speed would fall off it and
        silently take the fallback values; the model checks with this and re-cuts the window, recut().)"""
        if getattr(self, 'extent', None) is None or self.extent_lonlat is None:
            return False
        lo0, la0, lo1, la1 = self.extent_lonlat
        r = self.reader
        # the window may be bounded by the reader's own domain: nothing to gain beyond it
        xs, ys = np.asarray(r.x, dtype=np.float64), np.asarray(r.y, dtype=np.float64)
        x, y = self._box_outline_xy(lon_min - guard_lon, lat_min - guard_lat, lon_max + guard_lon, lat_max + guard_lat)
        ex, ey = self.extent
        return bool((x.min() < max(ex[0], xs.min())) or (x.max() > min(ex[1], xs.max())) or
                    (y.min() < max(ey[0], ys.min())) or (y.max() > min(ey[1], ys.max())))

    def recut(self, lonlat_box):
        """A new window for the blocks: every resident level is dropped and the device source of the reader is rebuilt with
        the next upload (the model rebinds its variables: the reader's source id changes)."""
        for pool in (self.slots, self.staged):
            for k in list(pool):
                self.ctx.drop_block(self.sid, pool.pop(k))
        self._drain_prefetched()
        self.close_read_ahead()       # (a level of the old window may be on its way)
        self._dist_shapes = None
        if self.sid is not None:
            self.ctx.release_source(self.sid)      # its id serves the re-cut source: the context holds 16 sources, not 16 per run
        self.sid = None
        self.set_extent(lonlat_box)

    def close_read_ahead(self):
        """End of the run, a re-cut window, a discarded reader: the worker's read in flight is waited for (the caller may close
        the reader's file afterwards) and the pool is shut down; a later read starts a new one."""
        for _, b, own in (self.leaves or ()):
            if own:
                b.close_read_ahead()
        a, self._ahead = self._ahead, None
        if a is not None:
            self._ahead_stats = tuple(x + y for x, y in zip(getattr(self, '_ahead_stats', (0, 0, 0.0)), (a.hits, a.misses, a.worker_s)))
            a.close()

    def _drain_prefetched(self, keep=()):
        """Sharded run: levels whose broadcast was started ahead and that are not (no longer) wanted are waited for and let
        go -- their tensors and work handles must not stay pinned, and an entry left behind would block every later prefetch."""
        from . import distributed as D
        for k in [k for k in self._dist_pre if k not in keep]:
            tens, works = self._dist_pre.pop(k)
            try:
                D.finish_broadcast(works)
            except Exception:
                pass

    def ensure_levels(self, t0, t1, extent=None, broadcast=None, times=None):
        """Make the time levels the step from t0 to t1 samples resident (datetime arguments).  `times`: the instants the
        step samples THIS reader at (default: t0, the middle and t1 -- a Runge-Kutta-4 step of a reader that holds the
        current; the model passes [t0] for Euler and for readers the stages do not sample)."""
        r = self.reader
        if self.leaves is not None:      # the leaves made here; a shared leaf is the model's to keep resident
            for _, b, own in self.leaves:
                if own:
                    b.ensure_levels(t0, t1, extent=extent, broadcast=broadcast, times=times)
            return
        if self.mesh is not None:
            return self._ensure_mesh_levels(times if times is not None else (t0, t0 + (t1 - t0) / 2, t1))
        if extent is None:
            extent = getattr(self, 'extent', None)
        if not self.is_grid():
            return
        if t1 != t0:
            self._direction = 1 if t1 > t0 else -1      # of the run (ReadAhead reads the next level in that direction)
        if r.times is None:
            need = [0]
        else:
            # The step samples the reader at t0 (main loop), t0 + dt/2 and t0 + dt (Runge-Kutta stages,
            # physics_methods.py:638-670): the two levels bracketing EACH of these times must be resident -- not the
            # whole range in between (a model time step may span many reader levels), and never a truncated range
            # (a dropped 'before' level would make the device extrapolate in time).
            if times is None:
                times = (t0, t0 + (t1 - t0) / 2, t1)
            times = [t for t in times if r.covers_time(t)]
            if not times:
                return
            need = sorted({k for t in times for k in r.nearest_time(t)})
            if len(need) > self.NSLOTS:     # cannot happen with NSLOTS = 6 (three instants, two levels each)
                raise ReaderLevelsError('reader %s: one model time step needs %d time levels resident, at most %d fit'
                                        % (r.name, len(need), self.NSLOTS))
        # sharded prefetch: an entry the run has passed (the model step skipped that level, or the direction changed) is let go
        if self._dist_pre:
            self._drain_prefetched(keep=[k for k in self._dist_pre if (k >= min(need) if t1 >= t0 else k <= max(need))])
        # make room: first the resident levels the step does not need, then prefetched levels it does not need
        missing = [k for k in need if k not in self.slots and k not in self.staged]
        for pool in (self.slots, self.staged):
            for k in list(pool):
                if len(self.slots) + len(self.staged) + len(missing) <= self.NSLOTS:
                    break
                if k not in need:
                    self.ctx.drop_block(self.sid, pool.pop(k))
        for k in need:
            if k in self.slots:
                continue
            if k in self.staged:     # prefetched on the upload stream while the previous steps ran
                self.slots[k] = self.staged.pop(k)
                import time as _time
                t_wait = _time.perf_counter()
                self.ctx.commit_block(self.sid, self.slots[k])      # (waits for the upload stream if the level is not ready yet)
                self.stall_s += _time.perf_counter() - t_wait
                continue
            self._upload(k, extent, broadcast, asynchronous=False)
        # prefetch the time level the run will need next (readers whose arrays live in host memory)
        rccl = False
        if self.world > 1:
            from . import distributed as D
            rccl = D.backend() == 'rccl'
        if self.prefetch and self.world > 1 and not rccl and r.times is not None and broadcast is None and self.sid is not None and \
                getattr(self, '_dist_shapes', None) is not None:
            kn = (max(need) + 1) if t1 >= t0 else (min(need) - 1)
            if 0 <= kn < len(r.times) and kn not in self.slots and kn not in self._dist_pre and len(self._dist_pre) == 0:
                try:
                    self._prefetch_dist(kn, extent)
                except Exception:        # a failing read shows up -- on every rank alike -- when the level is due
                    self._dist_pre.pop(kn, None)
        elif self.prefetch and r.times is not None and broadcast is None and not getattr(r, 's_levels', False):
            kn = (max(need) + 1) if t1 >= t0 else (min(need) - 1)
            if 0 <= kn < len(r.times) and kn not in self.slots and kn not in self.staged:
                if len(self.slots) + len(self.staged) >= self.NSLOTS:     # room for the prefetch: the stalest level goes
                    stale = [k for k in self.slots if k not in need]
                    if stale:
                        k_old = min(stale) if t1 >= t0 else max(stale)
                        self.ctx.drop_block(self.sid, self.slots.pop(k_old))
                if len(self.slots) + len(self.staged) < self.NSLOTS:
                    self._upload(kn, extent, None, asynchronous=True)

    def _ensure_mesh_levels(self, times):
        """The time levels NEAREST to the given instants become resident on the mesh: at most three distinct ones, uploaded
        synchronously, every variable of the binding."""
        r = self.reader
        if r.device_kind == 'schism':
            return self._ensure_schism_levels(times)
        need = sorted({r.nearest_time(t)[3] for t in times if r.covers_time(t)})
        for k in [k for k in self.mesh_slots if k not in need]:
            self.mesh_slots.pop(k)
        free = [s for s in range(_abi.UMESH_LEVELS) if s not in self.mesh_slots.values()]
        for k in need:
            if k in self.mesh_slots:
                continue
            if not free:
                raise ReaderLevelsError('reader %s: one model time step needs %d time levels resident, at most %d fit'
                                        % (r.name, len(need), _abi.UMESH_LEVELS))
            slot = free.pop(0)
            t = _epoch(r.times[k]) if r.times else 0.0
            for v in self.variables:
                self.mesh.set_level(slot, t, v, r.level(v, k), r.placement(v)[1])
            self.mesh_slots[k] = slot

    def _ensure_schism_levels(self, times):
        """The time levels that BRACKET the given instants become resident on the SCHISM mesh: zcor and every variable of the
        binding, uploaded synchronously.  Four slots serve a step of up to one level spacing; a longer one is refused."""
        r = self.reader
        need = sorted({k for t in times if r.covers_time(t) for k in r.nearest_time(t)[4:6]})
        if len(need) > _abi.SCHISM_LEVELS:
            raise ReaderLevelsError('reader %s: one model time step needs %d time levels resident, at most %d fit: the step is '
                                    'longer than the spacing of the reader\'s time levels' % (r.name, len(need), _abi.SCHISM_LEVELS))
        for k in [k for k in self.mesh_slots if k not in need]:
            self.mesh_slots.pop(k)
        free = [s for s in range(_abi.SCHISM_LEVELS) if s not in self.mesh_slots.values()]
        for k in need:
            if k in self.mesh_slots:
                continue
            slot = free.pop(0)
            t = _epoch(r.times[k])
            if r.zcor is not None:
                self.mesh.set_zcor(slot, t, r.zcor[k])
            for v in self.variables:
                self.mesh.set_level(slot, t, v, r.level(v, k))
            self.mesh_slots[k] = slot

    def _sample_schism(self, P, variables, first, time):
        r = self.reader
        kb, ka, w = r.time_weight(time, variables)
        if kb not in self.mesh_slots or (ka is not None and ka not in self.mesh_slots):
            self._ensure_schism_levels([time])
        pairs = [p for p in VECTOR_PAIRS_XY if p[0] in variables and p[1] in variables]
        ordered = [v for p in pairs for v in p] + [v for v in variables if not any(v in p for p in pairs)]
        flag = dict(zip(variables, first))
        for o in range(0, len(ordered), _abi.UMESH_MAX_VARIABLES):
            vs = ordered[o:o + _abi.UMESH_MAX_VARIABLES]
            P.schism_sample(self.mesh, self.mesh_slots[kb], None if ka is None else self.mesh_slots[ka], w, vs, [flag[v] for v in vs])

    def sample_mesh(self, P, variables, first, time):
        """The mesh's values for the particle set P at `time`, merged into its environment slots by priority (first[k]: the mesh
        heads the list of variable k) -- on the device, in launches of at most eight variables.  The slot is chosen here by the
        reference's nearest-time rule; outside the reader's time coverage nothing is sampled (environment.py:640-668)."""
        r = self.reader
        if not r.covers_time(time):
            return
        if r.device_kind == 'schism':      # two bracketing levels and their weight: one launch (odr_schism_sample)
            return self._sample_schism(P, variables, first, time)
        k = r.nearest_time(time)[3]
        if k not in self.mesh_slots:
            self._ensure_mesh_levels([time])
        # a vector pair stays in one launch: its components are rotated together
        pairs = [p for p in VECTOR_PAIRS_XY if p[0] in variables and p[1] in variables]
        ordered = [v for p in pairs for v in p] + [v for v in variables if not any(v in p for p in pairs)]
        flag = dict(zip(variables, first))
        for o in range(0, len(ordered), _abi.UMESH_MAX_VARIABLES):
            vs = ordered[o:o + _abi.UMESH_MAX_VARIABLES]
            P.umesh_sample(self.mesh, self.mesh_slots[k], vs, [flag[v] for v in vs])

    def sample_shape(self, P, first):
        """The polygons' land_binary_mask for the particle set P, merged into its environment slot by priority (first: the reader
        heads the variable's list) -- on the device, one launch (odr_shape_sample).  The reader is valid at every time."""
        P.shape_sample(self.shape, first)

    def sample_combined(self, P, variables, first, time):
        """The expression's values for the particle set P at `time`, merged into its environment slots by priority (first[k]: the
        expression heads the list of variable k) -- on the device, one launch per eight variables (odr_combined_sample).  Outside
        the expression's time coverage nothing is sampled.  The levels of every gridded leaf that bracket `time` are made
        resident here, at the time of the call; the program is rebuilt when a leaf's source id changed (its first block, a re-cut
        window)."""
        r = self.reader
        if not r.covers_time(time):
            return
        for _, b, _ in self.leaves:
            if b.is_grid():
                b.ensure_levels(time, time, times=[time])
        sids = tuple(b.sid for _, b, _ in self.leaves)
        if any(sid is None for sid in sids):
            raise RuntimeError('reader expression %s: a leaf has no device source at %s' % (r.name, time))
        if self.program is None or self._program_key != sids:
            if self.program is not None:
                self.program.close()
            sid_of = {id(leaf): b.sid for leaf, b, _ in self.leaves}
            uni_of = {id(leaf): k for k, leaf in enumerate(self.uniform)}
            self.program = self.ctx.combined([(op, sid_of[id(leaf)] if op == _abi.COMBINE_SOURCE else uni_of.get(id(leaf), 0), d)
                                              for op, leaf, d in self.postfix])
            self._program_key = sids
        # (no vector pair has to stay together: the reference's Combined does not rotate its operands, see CombinedReader)
        ordered, flag, t = list(variables), dict(zip(variables, first)), _epoch(time)
        for o in range(0, len(ordered), _abi.COMBINE_MAX_VARIABLES):
            vs = ordered[o:o + _abi.COMBINE_MAX_VARIABLES]
            uniform = [[leaf.value(v, time) for leaf in self.uniform] for v in vs] if self.uniform else None
            P.combined_sample(self.program, vs, [flag[v] for v in vs], t, uniform)

    def _read_and_broadcast(self, k, x, y, async_op):
        """Sharded run: rank 0 reads time level k, every rank receives it.  A reader failure on rank 0 reaches every rank as
        RemoteReaderError (the header of broadcast_reader_block): no rank is left waiting in a collective, and all of them
        count the failure alike."""
        from . import distributed as D
        r = self.reader
        time = r.times[k] if r.times is not None else None
        block, err, cids = None, None, None
        if self.rank == 0:
            try:
                if self._ahead is None:
                    self._ahead = ReadAhead(r, self.variables)
                block = self._ahead.read(k, x, y)
                cids = self._static_ids()
                # the level after this one IN THE RUN'S DIRECTION, on the worker thread, while the steps of this period run
                # (the first read of a backward run used to assume forward time: one level read and dropped, two stalls)
                step = getattr(self, '_direction', 0) or (1 if self._ahead_last is None or k >= self._ahead_last else -1)
                kn = k + step
                self._ahead_last = k
                if self.prefetch and r.times is not None and 0 <= kn < len(r.times):   # (nothing past the last level)
                    self._ahead.start(kn, x, y)
            except Exception as e:      # noqa: BLE001 -- every reader exception is a reader failure (environment.py:640-668)
                err = e
        shapes = getattr(self, '_dist_shapes', None)
        meta, tens, works = D.broadcast_reader_block(block, self.variables, src=0, error=err, shapes=shapes, async_op=async_op,
                                                     content_ids=cids)
        if shapes is None:
            self._dist_shapes = {v: tuple(t.shape) for v, t in tens.items() if v != '__cid__'}
        return meta, tens, works

    def _read_level_rccl(self, k, x, y):
        """Sharded run over the C-ABI collectives (distributed.backend() == 'rccl'): rank 0 reads time level k; every rank
        learns its HEADER -- failure, array shapes, ensemble members, content ids and (first level) the coordinate metadata --
        in one small broadcast; the arrays themselves travel inside odr_block_broadcast.  Returns (block dict whose variables
        are host arrays on rank 0 and shape placeholders elsewhere, arrays-or-None, shapes)."""
        from . import distributed as D
        r = self.reader
        block, err, hdr, arrays = None, None, None, None
        if self.rank == 0:
            try:
                if self._ahead is None:
                    self._ahead = ReadAhead(r, self.variables)
                block = self._ahead.read(k, x, y)
                step = getattr(self, '_direction', 0) or (1 if self._ahead_last is None or k >= self._ahead_last else -1)
                kn = k + step
                self._ahead_last = k
                if self.prefetch and r.times is not None and 0 <= kn < len(r.times):
                    self._ahead.start(kn, x, y)

                def one(a):
                    return np.ascontiguousarray(np.ma.filled(a, np.nan) if isinstance(a, np.ma.MaskedArray) else a, dtype=np.float32)
                arrays, members = {}, {}
                for v in self.variables:
                    if isinstance(block[v], (list, tuple)):     # ensemble members stacked along the layer axis
                        m = np.stack([one(a) for a in block[v]])
                        arrays[v], members[v] = np.ascontiguousarray(m.reshape((-1,) + m.shape[-2:])), len(block[v])
                    else:
                        arrays[v] = block[v]      # (copied once, into page-locked staging memory: _upload)
                hdr = dict(shapes={v: tuple(np.shape(a)) for v, a in arrays.items()}, members=members, cids=self._static_ids())
                if getattr(self, '_dist_meta', None) is None:
                    hdr['meta'] = {kk: (np.asarray(block[kk]) if kk in ('x', 'y', 'z') and block.get(kk) is not None else block.get(kk))
                                   for kk in ('x', 'y', 'z', 's_level_variables') if kk in block}
            except Exception as e:      # noqa: BLE001 -- every reader exception is a reader failure (environment.py:640-668)
                err = e
                hdr = dict(error=repr(e))
        hdr = D.broadcast_object(hdr, src=0)
        if 'error' in hdr:
            if err is not None:
                raise err
            raise D.RemoteReaderError('the reader failed on rank 0: ' + hdr['error'])
        if 'meta' in hdr:
            self._dist_meta = hdr['meta']
        self._dist_members = hdr['members']
        self._level_cids = hdr['cids']
        out = dict(self._dist_meta)
        for v, shp in hdr['shapes'].items():
            out[v] = arrays[v] if arrays is not None else _ShapeOnly(shp)
        return out, arrays, hdr['shapes']

    def _prefetch_dist(self, kn, extent):
        """Start the broadcast of the level the run needs next while the current one is in use (every rank makes this call
        at the same step: the collectives stay in the same order everywhere)."""
        x = y = None
        if extent is not None:
            x, y = np.array(extent[0]), np.array(extent[1])
        meta, tens, works = self._read_and_broadcast(kn, x, y, async_op=True)
        self._dist_pre[kn] = (tens, works)

    def _bind_convolution(self, block):
        """reader.convolve (set_convolution_kernel) -> the device source, before a level is uploaded: the upload's preparation
        convolves it (odr_source_set_convolution) whichever way it arrives -- synchronous, asynchronous, from device memory
        (s-levels regridded to z first, as the reference convolves what get_variables returns) or by odr_block_broadcast in a
        sharded run, where every rank holds the reader object and so the kernel."""
        conv = getattr(self.reader, 'convolve', None)
        if conv is not None and any(isinstance(block.get(v), (list, tuple)) or v in getattr(self, '_dist_members', {}) for v in self.variables):
            raise NotImplementedError('reader %s convolves its blocks and hands out ensemble members: the reference fails on the '
                                      'list of members (structured.py:184)' % self.reader.name)
        # (a host call without device work, made per level: the kernel may change between levels, and a re-cut window is a new source)
        if conv is not None or getattr(self, '_convolved', False):
            one_layer = [v for v in self.variables if len(getattr(block.get(v), 'shape', ())) == 3 and block[v].shape[0] == 1]
            self.ctx.set_convolution(self.sid, None if conv is None else convolution_weights(conv), three_d=one_layer)
        self._convolved = conv is not None

    def _page_locked(self, v, arr):
        if isinstance(arr, (list, tuple)):       # ensemble members: stacked by the context
            return arr
        a = np.asarray(arr) if not isinstance(arr, np.ma.MaskedArray) else arr
        if isinstance(a, np.ndarray) and not isinstance(a, np.ma.MaskedArray) and a.dtype == np.float32 and \
                a.flags['C_CONTIGUOUS'] and any(lo <= a.ctypes.data and a.ctypes.data + a.nbytes <= hi
                                                for lo, hi in getattr(self, '_pinned_ranges', [])):
            return a
        stage = self.__dict__.setdefault('_stage', {})
        st = stage.get((self._ring, v))
        if st is None or st.shape != a.shape:
            st = np.empty(a.shape, np.float32)
            try:
                self.ctx.pin(st)
            except Exception:
                pass
            stage[(self._ring, v)] = st
        np.copyto(st, np.ma.filled(a, np.nan) if isinstance(a, np.ma.MaskedArray) else a, casting='unsafe')
        return st

    def _upload(self, k, extent, broadcast, asynchronous):
        """One reader time level -> one device block (synchronously, or staged on the upload stream)."""
        r = self.reader
        time = r.times[k] if r.times is not None else None
        x = y = None
        rccl_arrays = rccl_shapes = None
        if extent is not None:
            x, y = np.array(extent[0]), np.array(extent[1])
        if self.world > 1:
            # sharded run (one process per GPU): the rank that owns the host Reader reads the level, every rank receives
            # it -- over RCCL / xGMI straight into device memory (opendrift_amd/distributed.py).  A level whose broadcast
            # was started one period ahead (_prefetch_dist) only has to be waited for.
            from . import distributed as D
            import time as _time
            t_wait = _time.perf_counter()
            rccl_arrays = rccl_shapes = None
            if D.backend() == 'rccl':
                if getattr(r, 's_levels', False):
                    raise NotImplementedError('a sigma-level reader in a sharded run needs ODR_DIST_BACKEND=nccl (the regridding '
                                              'reads the level on every rank)')
                block, rccl_arrays, rccl_shapes = self._read_level_rccl(k, x, y)
                block['time'] = time
                self.stall_s += _time.perf_counter() - t_wait
            else:
                if k in self._dist_pre:
                    tens, works = self._dist_pre.pop(k)
                    D.finish_broadcast(works)
                    meta = None
                else:
                    meta, tens, _ = self._read_and_broadcast(k, x, y, async_op=False)
                self.stall_s += _time.perf_counter() - t_wait
                if meta is not None:
                    self._dist_members = meta.pop('__members__', {})   # ensemble variables arrive as [members x nz, ny, nx] stacks
                    self._dist_meta = meta
                block = dict(self._dist_meta)
                block['time'] = time
                cid_t = tens.pop('__cid__', None)
                self._level_cids = None if cid_t is None else dict(zip(self.variables, [int(i) for i in cid_t.cpu().tolist()]))
                for v, t in tens.items():
                    block[v] = t if t.is_cuda else t.numpy()
                self._tensors = tens      # keep the device tensors alive until the block is built
                asynchronous = False
        else:
            block = r.get_variables(self.variables, time, x, y, np.array([0.0]))
        if broadcast is not None:
            block = broadcast(block)
        bx, by = np.asarray(block['x']), np.asarray(block['y'])
        bz = block.get('z', None)
        if self.sid is None and not getattr(r, 'projected', True):
            # reader without projection: the whole mesh is the device source (blocks must span it)
            zz = np.atleast_1d(bz) if bz is not None and np.size(bz) > 1 else None
            if (len(by), len(bx)) != r.lon.shape:
                raise NotImplementedError('a reader without projection must hand out blocks of its whole mesh')
            dom = (float(r.xmin), float(r.xmax), float(r.ymin), float(r.ymax), float(r.zmin), float(r.zmax))
            self.sid = self.ctx.add_grid_curvilinear(r.lon, r.lat, z=zz, domain=dom)
            sid, ctx = self.sid, self.ctx
            r._device_lookup = lambda lon, lat: ctx.lonlat2xy(sid, lon, lat)
            if r.start_time is not None:
                self.ctx.set_time_coverage(self.sid, _epoch(r.start_time), _epoch(r.end_time), r.always_valid)
        elif self.sid is None:
            proj = projection.parse_proj4(r.proj4)
            zz = np.atleast_1d(bz) if bz is not None and np.size(bz) > 1 else None
            # modulate_longitude (variables.py:259-280) decides on the TRUE longitudes of the domain's corners: some negative ->
            # np.mod(lon + 180, 360) - 180, else np.mod(lon, 360) (a rotated-pole reader's x is modulated the same way once more
            # for the coverage test: crs.is_geographic, :246).  In float64 the two branches agree on [0, 180); in the float32
            # arithmetic of a run's first get_environment (odr_ctx_set_position_class) they do not.
            exlons, _ = r.xy2lonlat(np.array([r.xmin, r.xmin, r.xmax, r.xmax], dtype=np.float64),
                                    np.array([r.ymin, r.ymax, r.ymax, r.ymin], dtype=np.float64))
            lon_mode = 1 if np.min(exlons) < 0 else 2
            dom = (float(r.xmin), float(r.xmax), float(r.ymin), float(r.ymax), float(r.zmin), float(r.zmax))
            if extent is not None:     # blocks cut to the simulation extent: the source covers what the blocks cover
                dom = (max(dom[0], float(np.min(bx))), min(dom[1], float(np.max(bx))), max(dom[2], float(np.min(by))),
                       min(dom[3], float(np.max(by))), dom[4], dom[5])
            self.sid = self.ctx.add_grid(bx, by, z=zz, proj=proj, lon_mode=lon_mode, domain=dom)
            if r.start_time is not None:
                self.ctx.set_time_coverage(self.sid, _epoch(r.start_time), _epoch(r.end_time), r.always_valid)
        else:
            g = self.ctx._grids[self.sid]
            if (len(by), len(bx)) != (g['ny'], g['nx']):
                raise ValueError('reader %s changed its block shape between time levels' % r.name)
        self._bind_convolution(block)
        free = [s for s in range(self.NSLOTS) if s not in self.slots.values() and s not in self.staged.values()]
        slot = free[0]
        t_ep = _epoch(time) if time is not None else 0.0
        if self.world > 1 and rccl_shapes is not None:
            # the level's arrays in ONE broadcast on the upload stream, straight into the staging memory of the block
            # preparation (odr_block_broadcast); staged like an asynchronous upload
            for v, m in getattr(self, '_dist_members', {}).items():
                self.ctx.declare_members(self.sid, v, m)
            if rccl_arrays is not None:
                # rank 0: the level through page-locked staging arrays of this binding (two sets in turn, as the asynchronous
                # upload of a one-process run): its copy into the device's staging memory is a DMA transfer the host does not
                # wait behind (pageable memory would go through the library's bounce buffer, synchronously)
                self._ring = 1 - getattr(self, '_ring', 1)
                rccl_arrays = {v: self._page_locked(v, a) for v, a in rccl_arrays.items()}
            self.ctx.block_broadcast(self.sid, slot, t_ep, rccl_arrays, rccl_shapes, root=0, content_ids=getattr(self, '_level_cids', None))
            if asynchronous:
                self.staged[k] = slot
            else:
                self.ctx.commit_block(self.sid, slot)
                self.slots[k] = slot
            return
        if asynchronous:
            if not self._pinned:     # page-lock the reader's in-memory arrays once: uploads become DMA transfers
                self._pinned = True
                self._pinned_ranges = []
                for v in self.variables:
                    a = getattr(r, 'arrays', {}).get(v)
                    if isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags['C_CONTIGUOUS']:
                        try:
                            self.ctx.pin(a)
                            self._pinned_ranges.append((a.ctypes.data, a.ctypes.data + a.nbytes))
                        except Exception:
                            pass
            # what is not a contiguous float32 piece of page-locked memory (a window cut out of the reader's arrays, a
            # masked or float64 array, ensemble lists) is copied into page-locked staging arrays of this binding, two
            # sets in turn: the upload then is an asynchronous DMA transfer for these as well (pageable memory would go
            # through the library's bounce buffer, synchronously)
            self._ring = 1 - getattr(self, '_ring', 1)
            self.ctx.upload_block_async(self.sid, slot, t_ep, {v: self._page_locked(v, block[v]) for v in self.variables},
                                        content_ids=self._static_ids())
            self.staged[k] = slot
            return
        if getattr(r, 's_levels', False):
            # ROMS-type reader: the block arrives on s-levels and is regridded to the z levels on the device
            # (reader_ROMS_native.py:617-684); the float32 result never visits the host
            if getattr(self, 'sgrid', None) is None:
                from .device import SigmaGrid
                self.sgrid = SigmaGrid(self.ctx, r.h, r.hc, r.Cs_r, Vtransform=r.Vtransform)
            arrays, nzv = {}, {}
            for i, v in enumerate([v for v in self.variables if v in block['s_level_variables']]):
                arrays[v] = self.sgrid.zslice(_dev(block[v]), bz, slot=i)
                nzv[v] = len(bz)
            for v in self.variables:
                if v not in arrays:
                    arrays[v] = _dev(block[v])
                    nzv.setdefault(v, block[v].shape[0] if len(block[v].shape) == 3 else 1)
            self.ctx.upload_block_device(self.sid, slot, _epoch(time) if time is not None else 0.0, arrays, nzv,
                                         content_ids={v: i for v, i in (self._static_ids() or {}).items() if v not in block.get('s_level_variables', ())})
        elif self.world > 1:
            for v, m in getattr(self, '_dist_members', {}).items():
                self.ctx.declare_members(self.sid, v, m)
            arrays = {v: _dev(block[v]) for v in self.variables}
            nzv = {v: (block[v].shape[0] if len(block[v].shape) == 3 else 1) for v in self.variables}
            self.ctx.upload_block_device(self.sid, slot, _epoch(time) if time is not None else 0.0, arrays, nzv,
                                         content_ids=getattr(self, '_level_cids', None))
            self._tensors = None
        else:
            arrays = {v: block[v] for v in self.variables}
            self.ctx.upload_block(self.sid, slot, _epoch(time) if time is not None else 0.0, arrays, content_ids=self._static_ids())
        self.slots[k] = slot
