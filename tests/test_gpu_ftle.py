"""GPU: odr_ftle_map / OpenDriftSimulation.calculate_ftle on the device.

* The cell launch against the host build of the same header (tests/ftle_host.py; tests/test_ftle_device_arithmetic.py pins that one to
  the reference's physics_methods.ftle): the host build is given the displacement planes the call itself reports, the maps are
  compared BIT FOR BIT.  Grids (nx x ny): 2 x 2, 2 x 65, 65 x 2, 3 x 3, 63 x 5, 64 x 5, 65 x 5 (a wave of 64 cells along x and its
  neighbours), 257 x 3, 129 x 131 (more than one workgroup each way), 66 x 4 and 64 x 3 (a workgroup is 64 x 4 cells; 63 / 65 x 5
  above are the other neighbours of that tile).  A block of uniform displacement (-inf), NaN elements in a corner, on an edge and in
  the interior, host and device pointers.
* The displacement launch against opendrift_amd.projection.Proj on the host for latlong, the double gyre's stereographic sphere and a
  polar stereographic ellipsoid.  Measure: max |device - host| over both planes / the largest |coordinate| of the grid.  Measured on
  an MI355X: 0 (latlong), 3.91e-16 (gyre), 1.20e-15 (polar); the bound is 4 x the largest, ftle_host.PROJECTION_BOUND = 4.8e-15
  (DESIGN.md 8h).
* calculate_ftle end to end with the parameters of the reference's example_double_gyre_LCS.py on 100 x 50 cells against a NumPy
  evaluation of the same formulas (np.gradient, float32 J and D, np.linalg.eigvalsh) on the test's own forward and backward run():
  identical masks, finite cells within ftle_host.ARITHMETIC_BOUND; and the order contract: trajectory k is cell k in both directions.
* Every refusal of odr_ftle_map, with nothing launched."""
import ctypes as C
from datetime import datetime, timedelta

import numpy as np
import pytest

import ftle_host as fh
from opendrift_amd import _abi, projection

pytestmark = pytest.mark.gpu

GYRE = '+proj=stere +lat_0=0 +lon_0=0 +lat_ts=0 +units=m +a=6.371e+06 +e=0 +no_defs'
POLAR = '+proj=stere +ellps=WGS84 +lat_0=90 +lat_ts=60 +lon_0=70 +x_0=3369600 +y_0=1844800 +units=m +no_defs'
PROJECTIONS = {'latlong': ('+proj=latlong', (3.0, 59.0), 0.05), 'gyre': (GYRE, (0.0, 0.0), 0.02), 'polar': (POLAR, (1.0e6, 4.0e5), 800.0)}
SHAPES = [(2, 2), (2, 65), (65, 2), (3, 3), (63, 5), (64, 5), (65, 5), (257, 3), (129, 131), (66, 4), (64, 3)]      # nx, ny
_FIELDS = {}


def field(name, nx, ny):
    """(Proj, xs, ys, delta, float32 lon [ny, nx], lat): the grid of a projection, moved by a sheared and folded map in the
    projection's coordinates, taken back to lon / lat on the host and rounded to float32.  Made once, never written to."""
    key = (name, nx, ny)
    if key not in _FIELDS:
        proj4, (x0, y0), delta = PROJECTIONS[name]
        p = projection.Proj(proj4)
        xs, ys = x0 + np.arange(nx) * delta, y0 + np.arange(ny) * delta
        X, Y = np.meshgrid(xs, ys)
        u, v = (X - x0) / delta, (Y - y0) / delta
        bx = X + delta * (0.8 * u + 1.7 * v + 2.5 * np.sin(0.4 * u + 0.2 * v))
        by = Y + delta * (-0.3 * u + 0.4 * v + 2.0 * np.cos(0.3 * u - 0.25 * v))
        lon, lat = p(bx, by, inverse=True)
        lon, lat = np.ascontiguousarray(lon, np.float32), np.ascontiguousarray(lat, np.float32)
        for a in (lon, lat, xs, ys):
            a.setflags(write=False)
        _FIELDS[key] = (p, xs, ys, delta, lon, lat)
    return _FIELDS[key]


def same_bits(got, want, what):
    """bit for bit; a NaN must be a NaN at the same place (its sign and payload are the processor's: x86 and gfx950 differ)"""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN at other places' % what
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not differ.any(), '%s: %d of %d cells differ' % (what, differ.sum(), got.size)


def device_and_host(ctx, p, xs, ys, delta, T, lon, lat):
    got, disp = ctx.ftle_map(p.params, xs, ys, delta, T, lon, lat, displacement=True)
    assert disp.shape == (2, len(ys), len(xs)) and disp.dtype == np.float64
    return got, fh.ftle_map(disp[0], disp[1], delta, T), disp


@pytest.mark.parametrize('name', ['latlong', 'gyre', 'polar'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_device_equals_host_build(ctx, shape, name):
    nx, ny = shape
    p, xs, ys, delta, lon, lat = field(name, nx, ny)
    got, want, disp = device_and_host(ctx, p, xs, ys, delta, 15.0, lon, lat)
    assert np.isfinite(want).all()
    same_bits(got, want, '%s %d x %d' % (name, nx, ny))
    again = ctx.ftle_map(p.params, xs, ys, delta, -15.0, lon, lat)      # a second call, and the sign of the duration
    same_bits(again, got, 'second call')


def test_block_of_uniform_displacement_is_minus_inf(ctx):
    """positions and axes that float32 holds exactly, so that the block's displacement is the same in every cell: -inf where the
    whole stencil lies inside"""
    nx, ny = 65, 9
    xs, ys = 2.0 + np.arange(nx) * 0.25, 58.0 + np.arange(ny) * 0.25
    p, _, _, _, lon, lat = field('latlong', nx, ny)
    lon, lat = lon.copy(), lat.copy()
    lon[2:6, 60:65] = (xs[60:65] + 0.5)[None, :]      # up to the right edge, across the wave boundary
    lat[2:6, 60:65] = (ys[2:6] - 0.75)[:, None]
    got, want, disp = device_and_host(ctx, p, xs, ys, 0.25, 15.0, lon, lat)
    same_bits(got, want, 'block')
    assert (disp[0][2:6, 60:65] == 0.5).all() and (disp[1][2:6, 60:65] == -0.75).all()
    inf = np.zeros((ny, nx), bool)
    inf[3:5, 61:65] = True      # at the grid's right edge the end difference stays inside the block
    assert np.array_equal(np.isneginf(got), inf) and not np.isnan(got).any()


@pytest.mark.parametrize('name', ['latlong', 'polar'])
def test_nan_elements(ctx, name):
    """elements that never had a position: NaN in every cell whose stencil reads them, the others untouched"""
    nx, ny = 129, 7
    p, xs, ys, delta, lon0, lat0 = field(name, nx, ny)
    clean = ctx.ftle_map(p.params, xs, ys, delta, 15.0, lon0, lat0)
    lon, lat = lon0.copy(), lat0.copy()
    holes = [(0, 0), (ny - 1, nx - 1), (0, 64), (3, 0), (3, 63), (4, 100)]
    for k, (j, i) in enumerate(holes):
        (lon if k % 2 else lat)[j, i] = np.nan
    got, want, disp = device_and_host(ctx, p, xs, ys, delta, 15.0, lon, lat)
    same_bits(got, want, 'NaN elements')
    for j, i in holes:
        assert np.isnan(disp[0][j, i]) and np.isnan(disp[1][j, i])      # either coordinate missing: no position
    nan = np.zeros((ny, nx), bool)
    for j, i in holes:
        for jj, ii in ((j - 1, i), (j + 1, i), (j, i - 1), (j, i + 1)):
            if 0 <= jj < ny and 0 <= ii < nx:
                nan[jj, ii] = True
        if j in (0, ny - 1) or i in (0, nx - 1):
            nan[j, i] = True
    assert np.array_equal(np.isnan(got), nan)
    same_bits(got[~nan], clean[~nan], 'cells away from the holes')


def test_device_pointers(ctx):
    """the positions as device arrays: the float32 environment slots of a particle set with one element per cell hold them"""
    nx, ny = 129, 131
    p, xs, ys, delta, lon, lat = field('polar', nx, ny)
    want = ctx.ftle_map(p.params, xs, ys, delta, 15.0, lon, lat)
    n = nx * ny
    P = ctx.particles(n)
    P.append(np.zeros(n), np.zeros(n))
    P.env_upload(0, lon.ravel())
    P.env_upload(1, lat.ravel())
    ctx.sync()
    dlon, dlat = P.device_ptr('env:0'), P.device_ptr('env:1')
    same_bits(ctx.ftle_map(p.params, xs, ys, delta, 15.0, dlon, dlat), want, 'device pointers')
    same_bits(ctx.ftle_map(p.params, xs, ys, delta, 15.0, dlon, lat), want, 'device and host arrays mixed')
    P.close()
    assert ctx.ftle_last_kernel_ms() > 0


@pytest.mark.parametrize('name', ['latlong', 'gyre', 'polar'])
def test_displacement_against_the_host_projection(ctx, name):
    nx, ny = 129, 131
    p, xs, ys, delta, lon, lat = field(name, nx, ny)
    _, disp = ctx.ftle_map(p.params, xs, ys, delta, 15.0, lon, lat, displacement=True)
    X, Y = np.meshgrid(xs, ys)
    bx, by = p(lon.astype(np.float64), lat.astype(np.float64))
    scale = max(np.abs(bx).max(), np.abs(by).max())
    m = max(np.abs(disp[0] - (bx - X)).max(), np.abs(disp[1] - (by - Y)).max()) / scale
    print('%s: displacement measure %.3g (bound %.3g), scale %.4g, displacement up to %.4g' % (
        name, m, fh.PROJECTION_BOUND, scale, np.abs(disp).max()))
    assert np.abs(disp).max() > 10 * delta      # a displacement worth the name
    assert m <= fh.PROJECTION_BOUND


def _gyre_model():
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.readers import DoubleGyreReader
    r = DoubleGyreReader(epsilon=.25, omega=0.628, A=.1)
    o = OceanDrift(loglevel=50)
    o.set_config('environment:fallback:land_binary_mask', 0)
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.add_reader(r)
    return o, r


def test_double_gyre_end_to_end(ctx):
    """example_double_gyre_LCS.py: DoubleGyreReader(epsilon=.25, omega=0.628, A=.1), runge-kutta4, time_step 0.5 s, duration 15 s,
    delta .02 -> 100 x 50 cells"""
    from opendrift_amd.oceandrift import last_valid
    o, r = _gyre_model()
    t0, dt, dur, delta = r.initial_time + timedelta(seconds=3), timedelta(seconds=.5), timedelta(seconds=15), .02
    lcs = o.calculate_ftle(time=t0, time_step=dt, duration=dur, delta=delta)
    xs, ys = np.arange(0., 2., delta), np.arange(0., 1., delta)
    X, Y = np.meshgrid(xs, ys)
    assert lcs['lon'].shape == (50, 100) and lcs['RLCS'].shape == lcs['ALCS'].shape == (1, 50, 100) and lcs['time'] == [t0]
    assert isinstance(lcs['RLCS'], np.ma.MaskedArray) and lcs['RLCS'].dtype == np.float64
    want = {}
    for key, start, step in (('RLCS', t0, dt), ('ALCS', t0 + dur, -dt)):      # the test's own runs over the same grid
        m, _ = _gyre_model()
        m.seed_elements(lcs['lon'].ravel(), lcs['lat'].ravel(), time=start, z=0)
        res = m.run(duration=dur, time_step=step)
        assert res['lon'].shape == (5000, 31)
        bx, by = r.proj(last_valid(res['lon']).astype(np.float64).reshape(X.shape), last_valid(res['lat']).astype(np.float64).reshape(X.shape))
        want[key] = fh.numpy_ftle(bx - X, by - Y, delta, 15.0)
        m._release_device()
    for key in ('RLCS', 'ALCS'):
        got = lcs[key][0]
        assert np.array_equal(np.ma.getmaskarray(got), ~np.isfinite(want[key])), key
        meas = fh.measure(got.data.astype(np.float32), want[key], 15.0)
        print('%s: %d masked, values %.4g .. %.4g, measure %.3g (bound %.3g)' % (key, np.ma.getmaskarray(got).sum(), got.min(), got.max(), meas,
                                                                             fh.ARITHMETIC_BOUND))
        assert meas <= fh.ARITHMETIC_BOUND, key
        assert got.max() - got.min() > 0.05      # ridges: exponents of the order of 1 / T apart
    # the order contract: the backward map is its own, not the forward one and not a map of flipped rows
    a, f = lcs['ALCS'][0].filled(np.nan), lcs['RLCS'][0].filled(np.nan)
    assert not np.allclose(a, f, atol=1e-3, equal_nan=True)
    assert not np.allclose(a, want['RLCS'], atol=1e-3, equal_nan=True)
    assert not np.allclose(a, a[::-1, ::-1], atol=1e-3, equal_nan=True)
    assert not np.allclose(a[::-1, ::-1], want['ALCS'], atol=1e-3, equal_nan=True)
    # the original model is untouched and can still run with the same reader
    assert o.mode == 'Config' and o.P is None
    o.seed_elements(lcs['lon'].ravel()[:7], lcs['lat'].ravel()[:7], time=t0)
    assert o.run(duration=dur, time_step=dt)['lon'].shape == (7, 31)


def test_constant_current_gives_fully_masked_maps(ctx):
    """a ConstantReader current (here: no current at all, on a grid that float32 holds exactly, so that the displacement is the same
    in every cell to the last bit): lambda = 0 and -inf everywhere, both maps fully masked"""
    from opendrift_amd.oceandrift import OceanDrift
    from opendrift_amd.readers import ConstantReader
    o = OceanDrift(loglevel=50)
    o.add_reader(ConstantReader({'x_sea_water_velocity': 0.0, 'y_sea_water_velocity': 0.0, 'land_binary_mask': 0.0}))
    t0 = datetime(2024, 1, 1)
    lcs = o.calculate_ftle(reader='+proj=latlong', domain=[2.0, 5.0, 58.0, 60.0], delta=0.25, time=[t0, t0 + timedelta(hours=1)],
                           time_step=600, duration=3600)
    assert lcs['RLCS'].shape == lcs['ALCS'].shape == (2, 8, 12)
    for key in ('RLCS', 'ALCS'):
        assert np.ma.getmaskarray(lcs[key]).all(), key
        assert np.isneginf(lcs[key].data).all(), key


def test_refusals_launch_nothing(ctx):
    nx, ny = 65, 5
    p, xs, ys, delta, lon, lat = field('polar', nx, ny)
    ctx.ftle_map(p.params, xs, ys, delta, 15.0, lon, lat)
    ms = ctx.ftle_last_kernel_ms()
    assert ms > 0
    from opendrift_amd.device import proj_desc
    desc = proj_desc(p.params)
    curvi = _abi.ProjDesc(3, 6378137.0, 0.0, 0.0, 0.0, 90.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    out = np.full((ny, nx), 7.0, np.float32)
    xs, ys = np.array(xs), np.array(ys)
    bad_x, inf_y = xs.copy(), ys.copy()
    bad_x[3], inf_y[-1] = np.nan, np.inf

    def call(proj=desc, nx=nx, ny=ny, xs=xs, ys=ys, delta=delta, T=15.0, lon=lon, lat=lat, out=out):
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
        return ctx.lib.odr_ftle_map(ctx.h, None if proj is None else C.byref(proj), nx, ny, ptr(xs, dp), ptr(ys, dp), delta, T,
                                    None if lon is None else C.c_void_p(lon.ctypes.data), None if lat is None else C.c_void_p(lat.ctypes.data),
                                    ptr(out, fp), None)
    refused = [dict(nx=1), dict(ny=1), dict(nx=0), dict(ny=-3), dict(nx=65536, ny=32768), dict(xs=bad_x), dict(ys=inf_y),
               dict(delta=np.nan), dict(delta=np.inf), dict(delta=0.0), dict(delta=-800.0), dict(T=0.0), dict(T=np.nan), dict(T=-np.inf),
               dict(proj=None), dict(xs=None), dict(ys=None), dict(lon=None), dict(lat=None), dict(out=None), dict(proj=curvi)]
    for kw in refused:
        assert call(**kw) == -1, kw
        assert ctx.lib.odr_last_error()
    assert (out == 7.0).all() and ctx.ftle_last_kernel_ms() == ms      # nothing ran, nothing was written
    assert call() == 0 and np.isfinite(out).all()
    with pytest.raises(ValueError):
        ctx.ftle_map(p.params, xs[:1], ys, delta, 15.0, lon[:, :1], lat[:, :1])
