"""CPU: geod_inverse and the trajectory lengths of csrc/odr_geodinv.hip.h in their host build (tests/geodinv_host.py) against the
known answers of the inverse problem (tests/golden/geodesic_inverse_kat.npz, 34-digit direct solves) and against the reference's own
get_trajectory_lengths (tests/golden/c34_trajectory_lengths.npz).  tests/test_gpu_trajectory_lengths.py shows that the device gives the
bits of this host build.  Each test prints what it measured before it asserts."""
import numpy as np
import pytest

import geodinv_host as gh
from conftest import golden


@pytest.fixture(scope='module')
def kat():
    k = golden('geodesic_inverse_kat.npz')
    rows = k['rows']
    azi1, azi2, s12 = gh.inverse(rows[:, 1], rows[:, 0], rows[:, 5], rows[:, 4])
    return dict(rows=rows, cls=k['cls'], azi1=azi1, azi2=azi2, s12=s12)


@pytest.fixture(scope='module')
def c34():
    return golden('c34_trajectory_lengths.npz')


def test_kat_covers_its_classes(kat):
    rows, cls = kat['rows'], kat['cls']
    assert len(rows) >= 200 and rows[:, 3].max() <= 19.9e6      # every line is the unique shortest one
    assert sorted(set(cls.tolist())) == list(range(7))
    assert rows[cls == 0, 3].max() <= 1e3 and rows[cls == 2, 3].min() >= 1e6 and rows[cls == 5, 3].min() >= 19.88e6
    assert (np.abs(rows[cls == 6, 1]) == 180).sum() >= 10


def test_distance_against_the_kat(kat):
    err = np.abs(kat['s12'] - kat['rows'][:, 3])
    for c in range(7):
        print('class %d: max |s12 - KAT| %.3g m' % (c, err[kat['cls'] == c].max()))
    assert gh.KAT_S12_BOUND_M <= 1e-6
    assert err.max() <= gh.KAT_S12_BOUND_M, err.max()


def test_landing_error_against_the_kat(kat):
    land = gh.landing_error_m(kat['azi1'], kat['s12'], kat['rows'][:, 2], kat['rows'][:, 3])
    print('max landing error %.3g m' % land.max())
    assert gh.KAT_LANDING_BOUND_M <= 1e-6
    assert land.max() <= gh.KAT_LANDING_BOUND_M, land.max()


def test_arrival_azimuth_against_the_kat(kat):
    """azi2 is the forward direction at point 2: as an error across the line over the line's own length"""
    long_enough = kat['rows'][:, 3] >= 1.0
    d = np.radians((kat['azi2'] - kat['rows'][:, 6] + 180.0) % 360.0 - 180.0)
    across = np.abs(d) * 6378137.0 * np.abs(np.sin(kat['rows'][:, 3] / 6378137.0))
    print('max azi2 error across the line %.3g m' % across[long_enough].max())
    assert across[long_enough].max() <= gh.KAT_LANDING_BOUND_M


def test_symmetry(kat):
    rows = kat['rows']
    back = gh.inverse(rows[:, 5], rows[:, 4], rows[:, 1], rows[:, 0])[2]
    print('max |s12(1->2) - s12(2->1)| %.3g m' % np.abs(back - kat['s12']).max())
    assert np.abs(back - kat['s12']).max() <= gh.KAT_S12_BOUND_M


def test_nan_and_bad_latitude_give_nan():
    nan = np.nan
    lon1 = [nan, 10, 10, 10, 10, 10, np.inf]
    lat1 = [50, nan, 50, 50, 90.5, 50, 50]
    lon2 = [11, 11, nan, 11, 11, 11, 11]
    lat2 = [51, 51, 51, nan, 51, -91, 51]
    for out in gh.inverse(lon1, lat1, lon2, lat2):
        assert np.isnan(out).all(), out


def test_coincident_points_give_zero():
    lon = np.array([0.0, 10.0, -180.0, 180.0, 77.7, 5.0, -33.0])
    lat = np.array([0.0, 50.0, -45.0, 30.0, 90.0, -90.0, -0.0])
    azi1, azi2, s12 = gh.inverse(lon, lat, lon, lat)
    assert (s12 == 0).all() and (azi1 == 0).all() and (azi2 == 0).all()
    assert gh.inverse(-180.0, 20.0, 180.0, 20.0)[2][0] == 0      # the same point under its two longitudes


def test_exact_lines():
    """a quarter meridian (the series' own value, 10 001 965.729 m) and an equatorial degree (a pi / 180)"""
    azi1, azi2, s12 = gh.inverse([0.0, 0.0], [0.0, 0.0], [0.0, 1.0], [90.0, 0.0])
    assert abs(s12[0] - 10001965.729) < 1e-3 and azi1[0] == 0
    assert abs(s12[1] - 6378137.0 * np.pi / 180) < 1e-8 and azi1[1] == 90 and azi2[1] == 90


@pytest.mark.parametrize('case, dt', [('', 3600.0), ('back_', -3600.0)])
def test_c34(c34, case, dt):
    assert float(c34['dt']) == 3600.0
    total, dist, speed = gh.trajectory_lengths(c34['lon'], c34['lat'], dt)
    gd, gs, gt = c34[case + 'distances'], c34[case + 'speeds'], c34[case + 'total_length']
    nseg = gd.shape[0]
    assert dist.shape == gd.shape == (c34['lon'].shape[1] - 1, c34['lon'].shape[0])
    print('max |distance - C34| %.3g m, |speed - C34| %.3g m/s, |total - C34| %.3g m'
          % (np.abs(dist - gd).max(), np.abs(speed - gs).max(), np.abs(total - gt).max()))
    assert np.abs(dist - gd).max() <= gh.C34_DISTANCE_BOUND_M
    assert np.abs(speed - gs).max() <= gh.C34_DISTANCE_BOUND_M / 3600.0
    assert np.abs(total - gt).max() <= nseg * gh.C34_DISTANCE_BOUND_M
    assert np.array_equal(total, np.cumsum(dist, 0)[-1, :])      # the sequential float64 sum, bit for bit
    assert np.array_equal(speed, dist / dt)
    # What the reference zeroed -- a NaN end, or (forward) faster than 100 m/s -- is exactly 0 here.  Between coincident points the
    # stand-in's shooting inverse leaves 0 or 1e-10 .. 8e-10 m, where geod_inverse (like pyproj's) gives 0.  So: zero where the
    # reference zeroed, zero at coincident pairs, and nowhere else.
    lon, lat = c34['lon'].T, c34['lat'].T
    nan_end = np.isnan(lon[:-1]) | np.isnan(lon[1:])
    coincident = (lon[:-1] == lon[1:]) & (lat[:-1] == lat[1:])
    cut = (gd == 0) & ~nan_end & ~coincident
    assert (gd[nan_end] == 0).all() and coincident.sum() >= 5
    assert cut.mean() >= 0.05 if dt > 0 else not cut.any()
    zeroed = nan_end | cut
    assert np.array_equal(dist == 0, zeroed | coincident)
    assert (speed[zeroed] == 0).all()
    if dt < 0:
        assert (speed <= 0).all() and dist.max() > 360e3      # nothing is cut in a backward run


def test_totals_only(c34):
    total = gh.trajectory_lengths(c34['lon'], c34['lat'], 3600.0, segments=False)
    assert np.array_equal(total, gh.trajectory_lengths(c34['lon'], c34['lat'], 3600.0)[0])
