"""GPU: odr_geod_inverse / odr_trajectory_lengths / OpenDriftSimulation.get_trajectory_lengths on the device against the host build
of the same header (tests/geodinv_host.py; tests/test_geodinv_host.py pins that one to the known answers and to the reference's
values), the known answers themselves (tests/golden/geodesic_inverse_kat.npz) and the reference's own get_trajectory_lengths
(tests/golden/c34_trajectory_lengths.npz).

The header uses no math-library function and no contraction the compiler picks, so the device gives the host build's bits.

Sizes: 1, 63, 64, 65 trajectories (a tile of 64 and its neighbours), 513 (more than one slab of tiles, a last tile of one row) x 2, 3,
65 output times (one interval, two, exactly one tile of 64), and 66 and 131 output times (a second tile of one interval, a third of
two)."""
import ctypes as C
from datetime import datetime, timedelta

import numpy as np
import pytest

import geodinv_host as gh
from conftest import golden

pytestmark = pytest.mark.gpu
_CLOUDS = {}


def cloud(ntraj, nt):
    """[trajectory, time] float32 lon, lat: slow drifters (metres per interval), fast ones (up to 300 km), trajectories that stand
    still, jumps to anywhere on the globe (poles, the seam and near-antipodal pairs among them: every branch of the inverse), NaN
    heads and tails.  Made once per size and never written to."""
    if (ntraj, nt) not in _CLOUDS:
        rng = np.random.default_rng(1000 * nt + ntraj)
        shape = (ntraj, nt)
        kind = rng.integers(0, 4, (ntraj, 1))
        step = np.where(kind == 0, 10 ** rng.uniform(-3, 3, shape), np.where(kind == 1, rng.uniform(1e3, 3e5, shape), 0.0))
        az = rng.uniform(0, 2 * np.pi, shape)
        lat0, lon0 = rng.uniform(-70, 70, (ntraj, 1)), rng.uniform(-180, 180, (ntraj, 1))
        lat = np.clip(lat0 + np.cumsum(step * np.cos(az), 1) / 111.2e3, -89.5, 89.5)
        lon = lon0 + np.cumsum(step * np.sin(az), 1) / (111.2e3 * np.cos(np.radians(lat0)))
        jump = (rng.uniform(size=shape) < 0.08) | (kind == 3)
        lat[jump] = rng.choice([-90.0, 90.0, 0.0, 37.25, -37.25], jump.sum()) + rng.choice([0.0, 1e-4, 0.3], jump.sum())
        lon[jump] = rng.choice([-180.0, 180.0, 0.0, 12.5, -167.5, 179.75], jump.sum()) + rng.choice([0.0, 1e-4, 0.3], jump.sum())
        lat = np.clip(lat, -90, 90)
        lon = (lon + 180.0) % 360.0 - 180.0
        t = np.arange(nt)[None, :]
        gone = (t < np.where(rng.uniform(size=ntraj) < 0.3, rng.integers(0, nt + 1, ntraj), 0)[:, None]) \
            | (t >= np.where(rng.uniform(size=ntraj) < 0.3, rng.integers(0, nt + 1, ntraj), nt)[:, None])
        lon[gone] = np.nan
        lat[gone] = np.nan
        _CLOUDS[ntraj, nt] = (np.ascontiguousarray(lon, np.float32), np.ascontiguousarray(lat, np.float32))
        for a in _CLOUDS[ntraj, nt]:
            a.setflags(write=False)
    return _CLOUDS[ntraj, nt]


def same(got, want, what):
    for g, w, name in zip(got, want, ('total_length', 'distances', 'speeds')):
        assert g.dtype == np.float64 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), '%s %s: %d values differ, largest difference %g' % (what, name, (g != w).sum(), np.abs(g - w).max())


@pytest.mark.parametrize('nt', [2, 3, 65, 66, 131])
@pytest.mark.parametrize('ntraj', [1, 63, 64, 65, 513])
def test_device_equals_host_build(ctx, ntraj, nt):
    lon, lat = cloud(ntraj, nt)
    for dt in (3600.0, -900.0):
        got = ctx.trajectory_lengths(lon, lat, dt)
        want = gh.trajectory_lengths(lon, lat, dt)
        same(got, want, 'dt %g' % dt)
        assert np.array_equal(got[0], np.cumsum(got[1], 0)[-1, :])
    if ntraj >= 513 and nt >= 65:
        d = want[1]
        assert (d > 19e6).any() and ((d > 0) & (d < 1)).any() and (d == 0).any()


def test_kat_through_geod_inv(ctx):
    rows = golden('geodesic_inverse_kat.npz')['rows']
    az12, az21, dist = ctx.geod_inv(rows[:, 1], rows[:, 0], rows[:, 5], rows[:, 4])
    land = gh.landing_error_m(az12, dist, rows[:, 2], rows[:, 3])
    print('max |s12 - KAT| %.3g m, landing error %.3g m' % (np.abs(dist - rows[:, 3]).max(), land.max()))
    assert np.abs(dist - rows[:, 3]).max() <= gh.KAT_S12_BOUND_M
    assert land.max() <= gh.KAT_LANDING_BOUND_M
    azi1, azi2, s12 = gh.inverse(rows[:, 1], rows[:, 0], rows[:, 5], rows[:, 4])
    assert np.array_equal(dist, s12) and np.array_equal(az12, azi1)
    assert np.array_equal(az21, np.where(azi2 > 0, azi2 - 180.0, azi2 + 180.0))      # pyproj's back azimuth
    back = ctx.geod_inv(rows[:, 5], rows[:, 4], rows[:, 1], rows[:, 0])[2]
    assert np.abs(back - dist).max() <= gh.KAT_S12_BOUND_M


def test_geod_inv_special_values(ctx):
    nan = np.nan
    out = ctx.geod_inv([nan, 10, 10, 10, 10], [50, nan, 50, 90.5, 50], [11, 11, nan, 11, 11], [51, 51, 51, 51, -91])
    assert all(np.isnan(o).all() for o in out)
    az12, az21, dist = ctx.geod_inv([10.0, -180.0], [50.0, 20.0], [10.0, 180.0], [50.0, 20.0])
    assert (dist == 0).all() and (az12 == 0).all() and (az21 == 180).all()
    az12, az21, dist = ctx.geod_inv(10.0, 50.0, [[10.0, 11.0], [12.0, 13.0]], 50.0)      # broadcasting keeps the shape
    assert dist.shape == (2, 2) and dist[0, 0] == 0 and (np.diff(dist.ravel()) > 0).all()


def _model(g, dt):
    from opendrift_amd.oceandrift import OceanDrift
    o = OceanDrift(loglevel=50)
    o.result = dict(time=list(range(g['lon'].shape[1])), lon=g['lon'], lat=g['lat'])
    o.time_step_output = timedelta(seconds=dt)
    return o


@pytest.mark.parametrize('case, dt', [('', 3600.0), ('back_', -3600.0)])
def test_c34_through_the_model(has_gpu, case, dt):
    g = golden('c34_trajectory_lengths.npz')
    total, dist, speed = _model(g, dt).get_trajectory_lengths()
    gd = g[case + 'distances']
    print('max |distance - C34| %.3g m, |total - C34| %.3g m' % (np.abs(dist - gd).max(), np.abs(total - g[case + 'total_length']).max()))
    assert np.abs(dist - gd).max() <= gh.C34_DISTANCE_BOUND_M
    assert np.abs(speed - g[case + 'speeds']).max() <= gh.C34_DISTANCE_BOUND_M / 3600.0
    assert np.abs(total - g[case + 'total_length']).max() <= gd.shape[0] * gh.C34_DISTANCE_BOUND_M
    assert np.array_equal(total, np.cumsum(dist, 0)[-1, :])
    same((total, dist, speed), gh.trajectory_lengths(g['lon'], g['lat'], dt), 'C34')      # whose zeros tests/test_geodinv_host.py checks


def test_device_pointers(ctx):
    """the inputs as device arrays: the float32 environment slots of a particle set with one element per entry hold them"""
    lon, lat = cloud(513, 65)
    want = gh.trajectory_lengths(lon, lat, 3600.0)
    n = lon.size
    P = ctx.particles(n)
    P.append(np.zeros(n), np.zeros(n))
    P.env_upload(0, lon.ravel())
    P.env_upload(1, lat.ravel())
    ctx.sync()
    ptr = [P.device_ptr('env:%d' % k) for k in range(2)]
    same(ctx.trajectory_lengths(ptr[0], ptr[1], 3600.0, shape=lon.shape), want, 'device pointers')
    same(ctx.trajectory_lengths(ptr[0], lat, 3600.0, shape=lon.shape), want, 'device and host arrays mixed')
    P.close()


def test_three_slabs(ctx, monkeypatch):
    """513 trajectories x 65 times: a budget of 200 rows of 2 * 65 * 4 B makes three slabs of whole trajectories"""
    lon, lat = cloud(513, 65)
    whole = ctx.trajectory_lengths(lon, lat, 3600.0)
    monkeypatch.setenv('ODR_TRAJ_SLAB_BYTES', str(200 * 2 * 65 * 4))
    same(ctx.trajectory_lengths(lon, lat, 3600.0), whole, 'three slabs')
    assert np.array_equal(ctx.trajectory_lengths(lon, lat, 3600.0, segments=False), whole[0])
    monkeypatch.setenv('ODR_TRAJ_SLAB_BYTES', '1')      # one trajectory per slab
    lon, lat = cloud(65, 3)
    same(ctx.trajectory_lengths(lon, lat, 3600.0), gh.trajectory_lengths(lon, lat, 3600.0), 'one trajectory per slab')
    monkeypatch.setenv('ODR_TRAJ_SLAB_BYTES', '0')
    with pytest.raises(ValueError):
        ctx.trajectory_lengths(lon, lat, 3600.0)


def test_totals_only_and_second_call(ctx):
    lon, lat = cloud(513, 131)
    one = ctx.trajectory_lengths(lon, lat, 3600.0)
    same(ctx.trajectory_lengths(lon, lat, 3600.0), one, 'second call')
    total = ctx.trajectory_lengths(lon, lat, 3600.0, segments=False)
    assert total.dtype == np.float64 and np.array_equal(total, one[0])
    assert ctx.trajectory_lengths_last_kernel_ms() > 0


def test_invalid_arguments(ctx):
    lon, lat = cloud(65, 3)
    assert ctx.trajectory_lengths(lon, lat, 3600.0)[0].shape == (65, )
    ms = ctx.trajectory_lengths_last_kernel_ms()
    assert ms > 0
    for dt in (0.0, -0.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            ctx.trajectory_lengths(lon, lat, dt)
    with pytest.raises(ValueError):
        ctx.trajectory_lengths(lon[:, :1], lat[:, :1], 3600.0)      # one output time
    dp = C.POINTER(C.c_double)
    total, dist = np.zeros(65), np.zeros((2, 65))
    p = [C.c_void_p(a.ctypes.data) for a in (lon, lat)]

    def call(ntraj=65, nt=3, ptrs=p, tot=total):
        return ctx.lib.odr_trajectory_lengths(ctx.h, ntraj, nt, *ptrs, 3600.0, None if tot is None else tot.ctypes.data_as(dp),
                                              dist.ctypes.data_as(dp), None)
    assert call(ptrs=[None, p[1]]) == -1 and call(ptrs=[p[0], None]) == -1 and call(tot=None) == -1
    assert call(nt=1) == -1 and call(ntraj=-1) == -1
    assert ctx.lib.odr_geod_inverse(ctx.h, 1, None, None, None, None, None, None, None) == -1
    assert ctx.trajectory_lengths_last_kernel_ms() == ms      # nothing was launched by any of them
    assert call() == 0 and np.array_equal(total, gh.trajectory_lengths(lon, lat, 3600.0)[0]) and dist.any()      # speeds NULL alone
    assert call(ntraj=0) == 0


def test_run_then_trajectory_lengths():
    """the C4 scenario of tests/test_gpu_model_api.py, eight steps of 900 s: the lengths of its result are the host build's"""
    from opendrift_amd import readers, synthetic as synth
    from opendrift_amd.oceandrift import OceanDrift
    g = golden('c4_stere_rk4_hdiff_strand.npz')
    names = ['x_sea_water_velocity', 'y_sea_water_velocity', 'x_wind', 'y_wind',
             'sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity', 'land_binary_mask']
    times = [datetime(2020, 1, 1) + timedelta(seconds=float(t)) for t in g['g_t']]
    o = OceanDrift(loglevel=50, seed=0, rng='numpy')
    o.add_reader(readers.GridReader(g['g_x'], g['g_y'], times, {k: g['g_' + k] for k in names}, proj4=synth.NORKYST_PROJ4))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('environment:constant:horizontal_diffusivity', 10)
    o.set_config('general:coastline_action', 'stranding')
    o.seed_elements(lon=g['lon'][0], lat=g['lat'][0], time=datetime(2020, 1, 1), wind_drift_factor=float(g['wdf']))
    o.run(time_step=900, steps=8)
    r = o.result
    total, dist, speed = o.get_trajectory_lengths()
    assert dist.shape == (8, r['lon'].shape[0]) and total.shape == (r['lon'].shape[0], )
    same((total, dist, speed), gh.trajectory_lengths(r['lon'], r['lat'], 900.0), 'run')
    moving = dist[0] > 0
    assert moving.any() and (speed[0][moving] < 10).all() and (total[moving] > 0).all()
