"""CPU: the seeding geometry of csrc/odr_seed.hip.h compiled for the host (tests/seed_host.py) against the reference's own
points_within_polygon (tests/golden/c35_seed_geometry.npz, written by tools/gen_golden_seed.py) and against matplotlib.

Grid sizes, inside counts and the inside flag of every grid point get no tolerance: the generator asserts that no grid point lies
within 1e-9 deg of an edge and that no grid size is within 1 % of its truncation.  Positions are held to 4 x the measured error of
the host build (seed_host.C35_*_BOUND_DEG).  tests/test_gpu_seed.py holds the device to this build bit for bit."""
import numpy as np
import pytest

import seed_host as sh
from conftest import golden


@pytest.fixture(scope='module')
def g():
    return golden('c35_seed_geometry.npz')


CASES = ['square_10', 'square_1000', 'wkt_100', 'star65_64', 'star65_257', 'star65_4097', 'star1025_1000', 'seam_500', 'sliver_3',
         'tiny_square_1', 'tiny_tri_2']


def test_no_case_is_left_out(g):
    assert sorted(CASES) == sorted(str(n) for n in g['poly_names'])
    assert {str(g[c + '_branch']) for c in CASES} >= {'truncate', 'duplicate', 'border', 'centre'}


@pytest.mark.parametrize('case', CASES)
def test_golden(g, case):
    number = int(g[case + '_number'])
    lon, lat, info = sh.points_within_polygon(g[case + '_lons'], g[case + '_lats'], number, mask=True)
    assert (info['nx'], info['ny'], info['n_inside']) == (int(g[case + '_nx']), int(g[case + '_ny']), int(g[case + '_n_inside']))
    assert np.array_equal(info['mask'], g[case + '_mask'])
    assert lon.shape == lat.shape == (number, ) and lon.dtype == lat.dtype == np.float64
    dlon, dlat = np.abs(lon - g[case + '_lon']).max(), np.abs(lat - g[case + '_lat']).max()
    print('%s: |lon - C35| %.3g deg, |lat - C35| %.3g deg' % (case, dlon, dlat))
    assert dlon <= sh.C35_LON_BOUND_DEG and dlat <= sh.C35_LAT_BOUND_DEG


def test_selection_is_cyclic_in_grid_order(g):
    """element k is inside point k mod L; a larger number of the same grid only repeats more"""
    lons, lats = g['square_10_lons'], g['square_10_lats']
    lon, lat, info = sh.points_within_polygon(lons, lats, 10, info=True)
    L = info['n_inside']
    assert L == 8 and np.array_equal(lon[L:], lon[:2]) and np.array_equal(lat[L:], lat[:2])
    assert (np.diff(lat[:L:2]) > 0).all() and (lon[1:L:2] > lon[0:L:2]).all()      # row-major from the south, x fastest
    lons, lats = g['sliver_3_lons'], g['sliver_3_lats']      # the border branch hands the vertices out, in their order
    lon, lat = sh.points_within_polygon(lons, lats, 3)
    assert np.array_equal(lon, lons) and np.array_equal(lat, lats)
    lons, lats = g['tiny_square_1_lons'], g['tiny_square_1_lats']
    lon, lat = sh.points_within_polygon(lons, lats, 1)
    assert lon.tolist() == [2.5] and lat.tolist() == [60.5]      # the centre branch: the mean of the vertices


@pytest.mark.parametrize('m', [4, 20, 66, 1026])
def test_points_in_polygon_equals_matplotlib(m):
    from matplotlib.path import Path
    vx, vy = sh.star_ring(m, 4.5, 60.2, 0.3, m)
    x, y = sh.probe_points(vx, vy, 20000, 100 + m)
    want = Path(np.c_[vx, vy]).contains_points(np.c_[x, y])
    got = sh.points_in_polygon(x, y, vx, vy)
    assert 0.2 < want.mean() < 0.8
    assert np.array_equal(got, want), '%d of %d flags differ' % ((got != want).sum(), len(x))
    assert np.array_equal(sh.crossing_rule(x, y, vx, vy), want)
    # a closed ring (the first vertex again) has a closing edge of no length: the same flags
    assert np.array_equal(sh.points_in_polygon(x, y, np.r_[vx, vx[0]], np.r_[vy, vy[0]]), want)


def test_albers_round_trip_and_hemispheres():
    rng = np.random.default_rng(7)
    for lat1, lat2, lon0 in ((59.0, 61.0, 4.5), (-35.0, -31.0, -150.0), (10.0, 11.0, 179.95)):
        lon, lat = rng.uniform(lon0 - 2, lon0 + 2, 500), rng.uniform(lat1 - 1, lat2 + 1, 500)
        x, y = sh.albers(lat1, lat2, 0.5 * (lat1 + lat2), lon0, lon, lat)
        assert np.abs(x).max() < 3e5 and np.abs(y).max() < 4e5
        lon2, lat2_ = sh.albers(lat1, lat2, 0.5 * (lat1 + lat2), lon0, x, y, forward=False)
        assert np.abs(lon2 - lon).max() < 1e-12 and np.abs(lat2_ - lat).max() < 1e-12
    # equal area: a 0.01 deg cell has the sphere's area R^2 cos(lat) dlon dlat
    d = 0.01
    cx, cy = sh.albers(59.0, 61.0, 60.0, 4.5, [4.0, 4.0 + d, 4.0 + d, 4.0], [60.3, 60.3, 60.3 + d, 60.3 + d])
    area = 0.5 * abs(np.dot(cx, np.roll(cy, -1)) - np.dot(cy, np.roll(cx, -1)))
    exact = 6370997.0 ** 2 * np.radians(d) * (np.sin(np.radians(60.3 + d)) - np.sin(np.radians(60.3)))
    assert abs(area / exact - 1) < 1e-6      # the chords of the cell's curved sides


def test_refusals():
    with pytest.raises(ValueError):      # standard parallels symmetric about the equator: no cone
        sh.points_within_polygon([0, 1, 1, 0], [-1, -1, 1, 1], 10)
    with pytest.raises(ValueError):      # no area
        sh.points_within_polygon([2, 3, 2], [60, 61, 60], 10)
    with pytest.raises(ValueError):
        sh.points_within_polygon([2, 3], [60, 61], 10)
    with pytest.raises(ValueError):
        sh.points_within_polygon([2, 3, 3], [60, 60, 61], 0)
    with pytest.raises(ValueError):
        sh.points_within_polygon([2, 3, np.nan], [60, 60, 61], 5)
    with pytest.raises(ValueError):
        sh.points_within_polygon([2, 3, 3], [60, 60], 5)
