"""GPU: odr_geod_npts / odr_points_in_polygon / odr_polygon_points and the model's seed_cone / seed_within_polygon on the device.

The polygon placement and the crossing rule are held to the host build of the same header BIT FOR BIT (tests/seed_host.py;
tests/test_seed_host.py pins that build to the reference's own points_within_polygon, tests/golden/c35_seed_geometry.npz, and to
matplotlib): every golden case, and the shapes at which the kernels can go wrong --
  rings of 255, 256, 257 and 513 edges (one LDS tile of 256 less one, exactly, plus one; two tiles plus one);
  grids of 1 x 1, 7 x 5 (under one wave), 13 x 5 (one wave plus one), 15 x 17, 16 x 16 and 257 x 1 (one workgroup of 256 -1, 0, +1);
  a 51 x 44 grid in a star (nine workgroups whose inside counts differ: the scan and the ranks);
  number < L, number == L, L < number < 2 L and number > 2 L for L inside points; the border and the centre branch.
odr_geod_npts is held to the oracle's C direct solve along the same line within the 1e-11 deg of tests/test_gpu_parity.py."""
import ctypes as C
from datetime import datetime, timedelta

import numpy as np
import pytest

import seed_host as sh
from conftest import golden

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
CASES = ['square_10', 'square_1000', 'wkt_100', 'star65_64', 'star65_257', 'star65_4097', 'star1025_1000', 'seam_500', 'sliver_3',
         'tiny_square_1', 'tiny_tri_2']


def same_placement(ctx, lons, lats, number, what):
    got = ctx.points_within_polygon(lons, lats, number, info=True)
    want = sh.points_within_polygon(lons, lats, number, info=True)
    assert got[2] == want[2], (what, got[2], want[2])
    for a, b, name in zip(got[:2], want[:2], ('lon', 'lat')):
        assert a.dtype == np.float64 and a.shape == (number, )
        assert np.array_equal(a, b), '%s %s: %d values differ, largest difference %g' % (what, name, (a != b).sum(), np.abs(a - b).max())
    return got


@pytest.mark.parametrize('case', CASES)
def test_golden_cases_equal_the_host_build(ctx, case):
    g = golden('c35_seed_geometry.npz')
    number = int(g[case + '_number'])
    lon, lat, info = same_placement(ctx, g[case + '_lons'], g[case + '_lats'], number, case)
    assert (info['nx'], info['ny'], info['n_inside']) == (int(g[case + '_nx']), int(g[case + '_ny']), int(g[case + '_n_inside']))
    dlon, dlat = np.abs(lon - g[case + '_lon']).max(), np.abs(lat - g[case + '_lat']).max()
    print('%s: |lon - C35| %.3g deg, |lat - C35| %.3g deg' % (case, dlon, dlat))
    assert dlon <= sh.C35_LON_BOUND_DEG and dlat <= sh.C35_LAT_BOUND_DEG


def box(nx, ny):
    """a lon / lat box of nx x ny hundredths of a degree (of arc) at 60 N"""
    w = nx * 0.01 / np.cos(np.radians(60.0))
    return [4.0, 4.0 + w, 4.0 + w, 4.0], [60.0, 60.0, 60.0 + ny * 0.01, 60.0 + ny * 0.01]


@pytest.mark.parametrize('nx, ny, number', [(1, 1, 1), (7, 5, 35), (13, 5, 65), (15, 17, 255), (16, 16, 256), (257, 1, 258)])
def test_grid_sizes_about_a_wave_and_a_workgroup(ctx, nx, ny, number):
    lons, lats = box(nx, ny)
    info = same_placement(ctx, lons, lats, number, '%d x %d' % (nx, ny))[2]
    assert (info['nx'], info['ny']) == (nx, ny) and 0 < info['n_inside'] <= nx * ny


def test_nine_workgroups_and_every_relation_of_number_to_the_inside_count(ctx):
    star = sh.star_ring(65, 4.5, 60.2, 0.3, 65)
    lon, lat, info = same_placement(ctx, *star, 1097, 'number == L')
    assert (info['nx'], info['ny'], info['n_inside']) == (51, 44, 1097)
    mask = sh.points_within_polygon(*star, 1097, mask=True)[2]['mask'].ravel()
    per_wg = [int(mask[k:k + 256].sum()) for k in range(0, mask.size, 256)]
    assert len(per_wg) == 9 and len(set(per_wg)) >= 5, per_wg      # the offsets of the scan differ from any multiple of one count
    g = golden('c35_seed_geometry.npz')
    info = same_placement(ctx, g['star1025_1000_lons'], g['star1025_1000_lats'], 1000, 'number < L')[2]
    assert info['n_inside'] == 1001
    info = same_placement(ctx, g['square_10_lons'], g['square_10_lats'], 10, 'L < number < 2 L')[2]
    assert info['n_inside'] == 8
    lon, lat, info = same_placement(ctx, [5.0, 5.53, 5.3332], [59.0, 59.77, 59.4988], 6, 'number > 2 L')
    assert info == dict(n_inside=1, nx=17, ny=50) and (lon == lon[0]).all() and (lat == lat[0]).all()      # in the third workgroup of four
    assert same_placement(ctx, g['sliver_3_lons'], g['sliver_3_lats'], 3, 'border')[2]['n_inside'] == 0
    assert same_placement(ctx, g['tiny_tri_2_lons'], g['tiny_tri_2_lats'], 2, 'centre')[2]['nx'] == 6
    # a second call gives the same bits, and the launches were timed
    again = ctx.points_within_polygon(*star, 1097)
    assert np.array_equal(again[0], same_placement(ctx, *star, 1097, 'again')[0]) and ctx.polygon_points_last_kernel_ms() > 0


@pytest.mark.parametrize('m', [4, 255, 256, 257, 513])
def test_points_in_polygon_equals_the_host_build(ctx, m):
    vx, vy = sh.star_ring(m, 4.5, 60.2, 0.3, m)
    x, y = sh.probe_points(vx, vy, 3000, 100 + m)      # random points, the vertices, edge midpoints, shared x or y
    got = ctx.points_in_polygon(x, y, vx, vy)
    want = sh.points_in_polygon(x, y, vx, vy)
    assert got.dtype == bool and 0.2 < want.mean() < 0.8
    assert np.array_equal(got, want), '%d of %d flags differ' % ((got != want).sum(), len(x))
    for n in (1, 63, 65, 257):      # under a wave, a wave plus one, a workgroup plus one
        assert np.array_equal(ctx.points_in_polygon(x[:n], y[:n], vx, vy), want[:n])


@pytest.mark.parametrize('npts', [1, 63, 64, 65, 1000])
def test_geod_npts_against_the_oracle(ctx, npts):
    from oracle import oracle as orc
    lines = [(4.4, 60.5, 4.4001, 60.50005), (4.4, 60.5, 4.5, 60.6), (176.5, -15.0, -177.0, -10.0), (-20.0, 50.0, -9.0, 54.5),
             (179.98, 70.0, -179.97, 70.01)]      # 10 m, 12 km, 900 km across the seam, 900 km, 2 km across the seam
    for lon1, lat1, lon2, lat2 in lines:
        lon, lat = ctx.geod_npts(lon1, lat1, lon2, lat2, npts)
        assert lon.shape == lat.shape == (npts, ) and lon.dtype == np.float64
        az12, s12 = (float(np.ravel(v)[0]) for v in ctx.geod_inv(lon1, lat1, lon2, lat2)[::2])
        dist = np.arange(1, npts + 1) * (s12 / (npts + 1))      # both ends excluded, s12 / (npts + 1) apart
        lo, la, _ = orc.geod_fwd(np.full(npts, lon1), np.full(npts, lat1), np.full(npts, az12), dist)
        dlon = np.abs((lon - lo + 180.0) % 360.0 - 180.0).max()
        print('%d points on (%g, %g) - (%g, %g): |dlon| %.3g deg, |dlat| %.3g deg' % (npts, lon1, lat1, lon2, lat2, dlon, np.abs(lat - la).max()))
        assert dlon < 1e-11 and np.abs(lat - la).max() < 1e-11
        assert (np.abs(lon) <= 180).all()
        # the points lie strictly between the ends and in order: the distance from point 1 grows by s12 / (npts + 1)
        d1 = ctx.geod_inv(lon1, lat1, lon, lat)[2]
        assert np.abs(d1 - dist).max() < 1e-6 and d1[0] > 0 and d1[-1] < s12


def test_invalid_arguments(ctx):
    dp, lib = C.POINTER(C.c_double), ctx.lib
    sq = [np.array(v, np.float64) for v in ([2, 3, 3, 2], [60, 60, 61, 61])]
    out = [np.zeros(10), np.zeros(10)]
    ni, nx, ny = C.c_int64(), C.c_int32(), C.c_int32()
    ctx.points_within_polygon(*sq, 10)
    ms = ctx.polygon_points_last_kernel_ms()
    assert ms > 0

    def call(m=4, lons=sq[0], lats=sq[1], number=10, o=out):
        return lib.odr_polygon_points(ctx.h, m, lons.ctypes.data_as(dp), None if lats is None else lats.ctypes.data_as(dp), number,
                                      None if o is None else o[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp), C.byref(ni), C.byref(nx),
                                      C.byref(ny))
    assert call(m=2) == -1 and call(number=0) == -1 and call(lats=None) == -1 and call(o=None) == -1
    assert call(lons=np.array([2, np.inf, 3, 2.0])) == -1 and call(lats=np.array([60, 60, np.nan, 61.0])) == -1
    assert call(lats=np.array([-1, -1, 1, 1.0])) == -1                    # no Albers cone
    assert call(m=3, lons=np.array([2, 3, 2.0]), lats=np.array([60, 61, 60.0])) == -1      # no area
    big = [np.array([0, 120, 120, 0.0]), np.array([10, 10, 80, 80.0])]
    assert call(lons=big[0], lats=big[1], number=1 << 31) == -1             # a grid of 2^31 points or more: refused before any write
    assert lib.odr_points_in_polygon(ctx.h, 1, None, None, 4, None, None, None) == -1
    assert lib.odr_geod_npts(ctx.h, 0.0, 0.0, 1.0, 1.0, 5, None, None) == -1
    assert lib.odr_geod_npts(ctx.h, 0.0, 91.0, 1.0, 1.0, 5, out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp)) == -1
    assert ctx.polygon_points_last_kernel_ms() == ms      # nothing was launched by any of them
    with pytest.raises(ValueError):
        ctx.points_within_polygon([2, 3, 3], [60, 60, 61], 0)
    with pytest.raises(ValueError):
        ctx.points_in_polygon([1.0], [1.0], [0, 1], [0, 1])
    assert call() == 0 and ni.value == 8 and (nx.value, ny.value) == (2, 4)
    assert ctx.geod_npts(0.0, 0.0, 1.0, 1.0, 0)[0].shape == (0, )


def _run(o, number):
    res = o.run(time_step=600, steps=2)
    assert res['lon'].shape[0] == number and np.isfinite(res['lon'][:, -1]).all()
    assert o.num_elements_active() == number


def _within_one_float32_ulp(sched, want64):
    want = np.float32(want64)
    return (np.abs(sched - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()


@pytest.mark.parametrize('model', ['OceanDrift', 'Leeway'])
def test_model_seed_cone_and_polygon_then_run(has_gpu, model, objectprop_path):
    from opendrift_amd import readers
    from opendrift_amd.leeway import Leeway
    from opendrift_amd.oceandrift import OceanDrift
    g = golden('c35_seed_geometry.npz')
    env = {'x_sea_water_velocity': 0.3, 'y_sea_water_velocity': 0.2, 'x_wind': 5.0, 'y_wind': -3.0}

    def new():
        o = Leeway(objectprop_path, loglevel=50, seed=0) if model == 'Leeway' else OceanDrift(loglevel=50, seed=0)
        o.add_reader(readers.ConstantReader(env))
        o.set_config('environment:constant:land_binary_mask', 0)
        return o, (dict(object_type=1) if model == 'Leeway' else dict(wind_drift_factor=.02))

    o, kw = new()
    np.random.seed(0)
    o.seed_cone(lon=[4.4, 4.5], lat=[60.5, 60.6], time=[T0, T0], number=100, **kw)
    assert o.num_elements_scheduled() == 100
    assert _within_one_float32_ulp(o._sched['lon'], g['cone_run_lon']) and _within_one_float32_ulp(o._sched['lat'], g['cone_run_lat'])
    assert round(float(o._sched['lon'][50]), 2) == 4.45      # the reference's own test_seed_cone
    _run(o, 100)

    o, kw = new()
    np.random.seed(0)
    o.seed_cone(lon=[176.5, -177.0], lat=[-15.0, -10.0], time=[T0, T0 + timedelta(hours=12)], number=500, **kw)      # radius 0: no draws
    assert _within_one_float32_ulp(o._sched['lon'], g['cone_seam_lon']) and _within_one_float32_ulp(o._sched['lat'], g['cone_seam_lat'])

    o, kw = new()
    np.random.seed(0)
    o.seed_within_polygon(g['wkt_100_lons'], g['wkt_100_lats'], number=100, time=T0, **kw)
    assert o.num_elements_scheduled() == 100
    assert _within_one_float32_ulp(o._sched['lon'], g['wkt_100_lon']) and _within_one_float32_ulp(o._sched['lat'], g['wkt_100_lat'])
    _run(o, 100)

    o, kw = new()
    np.random.seed(0)
    o.seed_cone(lon=4.7, lat=60.1, time=T0, radius=[0.0, 5000.0], number=50, **kw)      # the perturbation by radius on the device
    d = ctx_distance(o, float(np.float32(4.7)), float(np.float32(60.1)))      # positions are stored as float32
    assert d[0] < 1e-6 and d[1:].max() > 100 and d.max() < 5 * 5000      # radius 0 at the first element
    _run(o, 50)


def ctx_distance(o, lon, lat):
    return o.ctx.geod_inv(lon, lat, o._sched['lon'], o._sched['lat'])[2]
