"""GPU: readers.ShapeReader on the device -- odr_shape_contains and odr_shape_sample (csrc/odr_shape.hip.h) against the host build of
the same header, value for value, on the golden cases a to d (tests/golden/c37_shape_landmask.npz, the reference's reader with
matplotlib's predicate) and on the smallest shapes at which the index can go wrong (shape_host.edge_shapes), for 1, 63, 64, 65, 257
and 4 133 queries: the edges of a lane, a wave and a workgroup.  The merge by priority on a particle set; the reference's two
OceanDrift runs of case f (status of every element equal, positions within 1e-7 deg); closest_ocean_points equal to case e."""
from datetime import datetime

import numpy as np
import pytest

import shape_host as S
from opendrift_amd import projection, readers
from opendrift_amd.oceandrift import OceanDrift

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
LAND = 'land_binary_mask'


@pytest.fixture(scope='module')
def g():
    return np.load(S.GOLDEN)


def device_shape(ctx, r, nx=0, ny=0):
    return ctx.shape(r.x1, r.y1, r.x2, r.y2, r.poly, r.n_polygons, proj=projection.parse_proj4(r.proj4), invert=r.invert, nx=nx, ny=ny)


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
def test_contains_equals_the_host_build_and_the_reference(ctx, g, case):
    r = S.golden_reader(g, case)
    lon, lat, want = g[case + '_lon'], g[case + '_lat'], g[case + '_mask']
    x, y = (lon, lat) if case != 'c' else r.lonlat2xy(lon, lat)
    for grid in (0, 1, 300):
        D, H = device_shape(ctx, r, grid, grid), S.HostShape(r, grid, grid)
        got = D.contains(x, y)
        assert S.same_mask(got, H.contains(x, y)) and S.same_mask(got, want), (case, grid)
        hs, ds = H.stats(), D.stats()
        assert all(ds[k] == hs[k] for k in ('cells', 'entries', 'longest_list', 'mean_list', 'nudges')), (ds, hs)
        assert ctx.shape_last_kernel_ms() > 0
        D.close()


@pytest.mark.parametrize('name', sorted(S.edge_shapes()) + ['lines_through_vertices'])
def test_edge_shapes_at_lane_wave_and_workgroup_edges(ctx, name):
    polygons, invert, nx, ny = S.edge_shapes()[name] if name != 'lines_through_vertices' else (S.lines_through_vertices(4, 4), False, 4, 4)
    r = readers.ShapeReader(polygons, invert=invert)
    D, H = device_shape(ctx, r, nx, ny), S.HostShape(r, nx, ny)
    if name == 'lines_through_vertices':
        assert D.stats()['nudges'] >= 1
    for n in (1, 63, 64, 65, 257, 4133):
        qx, qy = S.shape_queries(r, n, 20 + n)
        got = D.contains(qx, qy)
        assert got.shape == (n,) and S.same_mask(got, H.contains(qx, qy)) and S.same_mask(got, H.all_edges(qx, qy)), (name, n)
    D.close()


@pytest.mark.parametrize('case', ['a', 'c', 'd'])
def test_sample_merges_by_priority_on_a_particle_set(ctx, g, case):
    """Elements given as lon / lat (case c: the polygons are in UTM 33, the launch projects), a slot pre-filled with 0.25 where the
    index is a multiple of 3 and NaN elsewhere: first -- the reader's value wherever it covers; not first -- only what is missing.
    Outside the box the slot keeps what it has, NaN included: left for the next reader or the fallback."""
    r = S.golden_reader(g, case)
    b = readers.DeviceReaderBinding(ctx, r)
    assert b.sid is None and b.shape is not None and not b.is_grid() and not b.host_eval
    lon, lat, want = g[case + '_lon'], g[case + '_lat'], g[case + '_mask']
    n = len(lon)
    pre = np.where(np.arange(n) % 3 == 0, np.float32(0.25), np.float32(np.nan)).astype(np.float32)
    for first in (True, False):
        P = ctx.particles(n)
        P.append(lon, lat, z=np.zeros(n))
        P.env_upload(LAND, pre)
        b.sample_shape(P, first)
        got = P.env_download(LAND)
        take = np.isfinite(want) & (first | ~np.isfinite(pre))
        assert S.same_mask(got, np.where(take, want, pre)), (case, first)
        assert np.isnan(got).sum() > 300 and (got == 0.25).sum() > (300 if first else 1300)
        P.close()
    P = ctx.particles(n)      # a slot that was never sampled starts as NaN
    P.append(lon, lat, z=np.zeros(n))
    b.sample_shape(P, False)
    assert S.same_mask(P.env_download(LAND), want)
    assert ctx.shape_last_kernel_ms() > 0
    P.close()


def model(g, tag, action, scheme):
    o = OceanDrift(loglevel=50, seed=0, rng='numpy')
    o.add_reader(S.golden_reader(g, 'a'))
    o.add_reader(readers.ConstantReader({'x_sea_water_velocity': float(g['f_u']), 'y_sea_water_velocity': float(g['f_v']), 'x_wind': 0.0,
                                         'y_wind': 0.0}))
    o.set_config('general:coastline_action', action)
    o.set_config('general:coastline_approximation_precision', None)
    o.set_config('seed:ocean_only', False)
    o.set_config('drift:advection_scheme', scheme)
    o.set_config('drift:stokes_drift', False)
    o.set_config('drift:vertical_advection', False)
    o.set_config('drift:vertical_mixing', False)
    o.seed_elements(lon=g['f_%s_lon0' % tag], lat=g['f_%s_lat0' % tag], z=0.0, time=T0, wind_drift_factor=0.0)
    return o


@pytest.mark.parametrize('tag,scheme', [('stranding', 'euler'), ('previous', 'runge-kutta4')])
def test_model_runs_reproduce_the_reference(g, tag, scheme):
    """The reference's OceanDrift with its own shape reader as the only source of land_binary_mask and a constant current that drives
    the elements into the coast, against this model with the polygons on the device.  Every position the reference's reader was
    asked at keeps more than 1e-5 deg from every edge (the golden stores the smallest distance), 100 x the bound asserted here."""
    assert float(g['f_smallest_gap_deg']) > 1e-5
    o = model(g, tag, tag, scheme)
    assert o._run_lane() == 'call_by_call'
    o.run(time_step=float(g['f_dt']), steps=int(g['f_steps']))
    assert o._run_lane() == 'call_by_call'
    n = len(g['f_%s_lon' % tag])
    lon, lat, status = np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1)
    for d in (o.elements, o.elements_deactivated):
        lon[d.ID], lat[d.ID], status[d.ID] = d.lon, d.lat, d.status
    assert np.array_equal(status, g['f_%s_status' % tag])
    assert list(o.status_categories) == [str(c) for c in g['f_%s_categories' % tag]]
    dmax = max(np.abs(lon - g['f_%s_lon' % tag]).max(), np.abs(lat - g['f_%s_lat' % tag]).max())
    print(tag, scheme, 'polygons on the device vs the reference: %.2e deg' % dmax, 'stranded', int((status != 0).sum()))
    assert dmax < 1e-7
    touched = g['f_%s_touched' % tag]
    assert touched.sum() >= n // 4 and (~touched).sum() >= n // 4
    if tag == 'stranding':
        assert np.array_equal(status != 0, touched)
    # the elements that never touched land moved the whole way (0.9 m/s over 2.5 h: 0.146 deg of longitude and more)
    moved = np.hypot(lon - g['f_%s_lon0' % tag], lat - g['f_%s_lat0' % tag])
    assert moved[~touched].min() > 0.14 and moved[touched].min() < 0.02


def test_closest_ocean_points_equals_the_reference(g):
    r = readers.ShapeReader(S.golden_polygons(g, 'a'), land_buffer_distance=0)
    o = OceanDrift(loglevel=50, seed=0)
    o.add_reader(r)
    o.add_reader(readers.ConstantReader({'x_sea_water_velocity': 0.0, 'y_sea_water_velocity': 0.0, 'x_wind': 0.0, 'y_wind': 0.0}))
    o.set_config('seed:ocean_only', True)
    lon, lat = g['e_lon'].astype(np.float64), g['e_lat'].astype(np.float64)
    x, y, d = r.get_nearest_outside(lon, lat, 0)      # (the host: scipy's tree)
    assert np.array_equal(x, g['e_nearest_x']) and np.array_equal(y, g['e_nearest_y']) and np.allclose(d, g['e_nearest_distance'], rtol=1e-14)
    o.seed_elements(lon=lon, lat=lat, time=T0, wind_drift_factor=0.0)
    o.run(time_step=600, steps=1)
    want = np.asarray(g['e_land_indices'])
    moved_lon, moved_lat = o._sched['lon'], o._sched['lat']
    assert np.array_equal(np.float32(moved_lon), g['e_moved_lon']) and np.array_equal(np.float32(moved_lat), g['e_moved_lat'])
    assert 50 < len(want) < 350 and (np.float32(moved_lon)[want] != g['e_lon'][want]).any()
    lo, la, idx = o.closest_ocean_points(lon.copy(), lat.copy())      # the call itself, through the device's k-d tree
    assert np.array_equal(idx, want) and np.array_equal(np.float32(lo), g['e_moved_lon']) and np.array_equal(np.float32(la), g['e_moved_lat'])
