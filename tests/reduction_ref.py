"""NumPy reference of the sixteen global reductions over the active elements (odr_reduce_local / odr_reduce_scalars, and
what the movers read from the cache): written from the reference project's lines, not from the kernel --

  advect_wind          physics_methods.py:738-780   surface = z >= -|wind_drift_depth|; wdf = wdf*(wdd + z)/wdd in float64
                                                    (wind_drift_factor is a float32 array, wind_drift_depth a float64 one),
                                                    left alone for wind_drift_depth == 0 and put back where z > 0;
                                                    wdf[surface].max(); speed = sqrt(x*x + y*y) of the float32 wind, the
                                                    float32 current subtracted first with drift:relative_wind;
                                                    surface.sum() == 0, wdf max == 0, speed.max() == 0 -> return
  stokes_drift         physics_methods.py:799-804   max(stokes_x + stokes_y) == 0 -> return   (float32 sum)
  horizontal_diffusion basemodel/__init__.py:1754   D.max() == 0 -> return
  vertical_mixing      oceandrift.py:430            MLD.max() sizes the wind-parameterised profile

over the elements the reference still holds when it gets there: status 0 (deactivated elements are removed before).

ONE DEPARTURE, pinned here and not changed: the device ignores NaN (fmax; `> 0` / `== 0` votes in the step launch), where
`ndarray.max()` propagates it.  This reference ignores NaN too (np.fmax), so a NaN in z or in a sampled variable leaves the
extreme of the finite values; an element whose z is NaN is not at the surface (NaN >= x is False in the reference as well).

Slots (the R_* order of odr_kernels.hip.h; minima are stored negated so that every slot but the two counts is a maximum):
  0 n_active   1 -lon_min  2 lon_max  3 -lat_min  4 lat_max  5 -z_min  6 z_max  7 D_max  8 stokes_sum_max
  9 wind_speed_max (surface elements, never relative)  10 wdf_surface_max  11 n_surface  12 hs_max  13 tp_max
  14 rel_wind_speed_max (the speed advect_wind tests: relative when asked for and both current components are there)
  15 mld_max
A variable that is absent leaves its slot at -inf; without the wind there is no surface bookkeeping at all (n_surface 0).
"""
import numpy as np

U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
XW, YW = 'x_wind', 'y_wind'
SX, SY = 'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity'
HD = 'horizontal_diffusivity'
HS = 'sea_surface_wave_significant_height'
TP = 'sea_surface_wave_period_at_variance_spectral_density_maximum'
MLD = 'ocean_mixed_layer_thickness'
ENV_NAMES = (U, V, XW, YW, SX, SY, HD, HS, TP, MLD)

KEYS = ['n_active', 'lon_min', 'lon_max', 'lat_min', 'lat_max', 'z_min', 'z_max', 'D_max', 'stokes_sum_max',
        'wind_speed_max', 'wdf_surface_max', 'n_surface', 'hs_max', 'tp_max', 'rel_wind_speed_max', 'mld_max']
COUNTS = (0, 11)
NEGATED = ('lon_min', 'lat_min', 'z_min')


def _max(a):
    """maximum ignoring NaN, -inf for nothing (or nothing but NaN), as float64"""
    return float(np.fmax.reduce(np.asarray(a, dtype=np.float64), initial=-np.inf))


def raw16(lon, lat, z, status, wdf, env, wind_drift_depth, relative_wind):
    act = np.asarray(status) == 0
    lon, lat, z = (np.asarray(a, dtype=np.float64)[act] for a in (lon, lat, z))
    wdf32 = np.asarray(wdf, dtype=np.float32)[act]
    e = {k: np.asarray(v, dtype=np.float32)[act] for k, v in env.items() if v is not None}
    raw = np.full(16, -np.inf)
    raw[0] = float(act.sum())
    raw[11] = 0.0
    raw[1], raw[2] = _max(-lon), _max(lon)
    raw[3], raw[4] = _max(-lat), _max(lat)
    raw[5], raw[6] = _max(-z), _max(z)
    if HD in e:
        raw[7] = _max(e[HD])
    if SX in e and SY in e:
        raw[8] = _max(e[SX] + e[SY])                      # float32 + float32
    if HS in e:
        raw[12] = _max(e[HS])
    if TP in e:
        raw[13] = _max(e[TP])
    if MLD in e:
        raw[15] = _max(e[MLD])
    if XW in e and YW in e:
        wdd = abs(float(wind_drift_depth))
        with np.errstate(all='ignore'):
            surface = z >= -wdd
            f = wdf32.astype(np.float64)
            if wdd != 0:
                f = f * (wdd + z) / wdd
                f[z > 0] = wdf32[z > 0]
            x, y = e[XW][surface], e[YW][surface]
            raw[11] = float(surface.sum())
            raw[10] = _max(f[surface])
            raw[9] = _max(np.sqrt(x * x + y * y))
            if relative_wind and U in e and V in e:
                x, y = x - e[U][surface], y - e[V][surface]
            raw[14] = _max(np.sqrt(x * x + y * y))
    return raw


def as_dict(raw):
    """what Particles.reduction_dict does: the slots by name, the minima with their sign back"""
    d = dict(zip(KEYS, (float(v) for v in raw)))
    for k in NEGATED:
        d[k] = -d[k]
    return d


def combine(rows):
    """rows of several particle sets -> the row of their union (counts summed, maxima maximised)"""
    rows = np.asarray(rows, dtype=np.float64)
    out = rows.max(axis=0)
    for k in COUNTS:
        out[k] = rows[:, k].sum()
    return out
