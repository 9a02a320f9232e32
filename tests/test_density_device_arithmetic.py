"""CPU: the bin search and the classification of csrc/odr_density.hip.h, compiled for the host (tests/density_host.cpp), against the
reference's own maps (tests/golden/c32_density.npz, written by the reference's get_density_array; tools/gen_golden_density.py) and
against np.searchsorted.

Counts and sums of integer-valued float32 weights are exact in float64 whatever the order of the additions: bit for bit.  A sum of
real-valued weights carries the rounding of its order on either side: every bin within 2 (k - 1) 2^-53 sum|w| of the golden, k and
sum|w| of that bin from the golden's inputs (density_host.weighted_bound)."""
import numpy as np
import pytest

import density_host as dh
from conftest import golden


@pytest.fixture(scope='module')
def g():
    return golden('c32_density.npz')


def _inputs(g, single=False):
    a = [g[k] for k in ('lon', 'lat', 'z', 'status')]
    if single:
        t = int(g['single_time_index'])
        a = [np.ascontiguousarray(v[:, t:t + 1]) for v in a]
    return a


def test_golden_is_what_the_generator_promises(g):
    lon, z, status = g['lon'], g['z'], g['status']
    code = int(g['stranded_code'])
    assert lon.dtype == np.float32 and lon.shape == (300, 6)
    assert np.isnan(lon).mean() >= 0.1 and (status == code).mean() >= 0.1 and (z < 0).mean() >= 0.1
    assert (np.isfinite(lon) & (z >= 0) & (status != code)).mean() >= 0.1
    assert (np.signbit(z) & (z == 0)).any() and (np.isnan(z) & np.isfinite(lon)).any()
    assert len(g['lon_array']) != len(g['lat_array']) and min(len(g['lon_array']), len(g['lat_array'])) > 20
    assert g['counts_H'].max() >= 3 and g['counts_H'].shape == (6, len(g['lon_array']) - 1, len(g['lat_array']) - 1)


@pytest.mark.parametrize('case', ['counts', 'nostranded', 'wint', 'single'])
def test_exact_cases_equal_the_reference_bit_for_bit(g, case):
    single = case == 'single'
    edges = (g['single_lon_array'], g['single_lat_array']) if single else (g['lon_array'], g['lat_array'])
    weight = g['mass_int'] if case == 'wint' else None
    code = -1 if case == 'nostranded' else int(g['stranded_code'])
    got = dh.density_map(*_inputs(g, single), *edges, weight, code)
    for h, name in zip(got, ('H', 'H_submerged', 'H_stranded')):
        want = g['%s_%s' % (case, name)]
        assert h.dtype == want.dtype and h.shape == want.shape
        assert np.array_equal(h, want), '%s %s: %d bins differ' % (case, name, (h != want).sum())
    assert got[0].sum() > 0 and got[1].sum() > 0 and (got[2].sum() > 0) == (case != 'nostranded')


def test_real_weights_within_the_summation_bound(g):
    code = int(g['stranded_code'])
    args = _inputs(g) + [g['lon_array'], g['lat_array']]
    got = dh.density_map(*args, g['mass'], code)
    bound = dh.weighted_bound(*args, g['mass'], code)
    for h, b, name in zip(got, bound, ('H', 'H_submerged', 'H_stranded')):
        want = g['wreal_' + name]
        err = np.abs(h - want)
        print(name, 'largest error / bound over the bins with k > 1: %.3g' % (err[b > 0] / b[b > 0]).max(), 'bins with k > 1:', (b > 0).sum())
        assert (err <= b).all(), '%s: %d bins outside the bound' % (name, (err > b).sum())
        assert (b > 0).sum() > 20


def test_classes_literally_from_the_masks():
    z = np.array([0.0, -0.0, -1.0, np.nan, 2.0, 0.0, -3.0, np.nan], np.float32)
    status = np.array([0, 0, 0, 0, 2, 2, 2, np.nan], np.float32)
    want = np.array([1, 1, 2, 3, 1 | 4, 1 | 4, 2 | 4, 3], np.int32)
    assert np.array_equal(dh.classes(z, status, 2), want)
    assert np.array_equal(dh.classes(z, status, -1), want & 3)      # no 'stranded' category
    assert np.array_equal(dh.classes(z, status, 0), np.array([1 | 4, 1 | 4, 2 | 4, 3 | 4, 1, 1, 2, 3], np.int32))


def _edge_sets():
    rng = np.random.default_rng(5)
    lat = np.float32(60.0)
    d = 400.0 / 111000.0
    yield 'arange', np.arange(lat - d, np.float32(60.4) + d, d)      # what get_density_array builds
    yield 'arange_wide', np.arange(-179.3, 179.9, 0.0107)
    yield 'two', np.array([-1.5, 2.25])
    yield 'uneven', np.cumsum(rng.uniform(1e-3, 5.0, 300)) - 200.0
    yield 'clustered', np.sort(np.concatenate([np.linspace(0, 1, 50), 0.5 + np.arange(1, 40) * 1e-12]))


@pytest.mark.parametrize('name,edges', list(_edge_sets()), ids=[k for k, _ in _edge_sets()])
def test_bin_equals_searchsorted(name, edges):
    rng = np.random.default_rng(11)
    assert (np.diff(edges) > 0).all()
    span = edges[-1] - edges[0]
    v = rng.uniform(edges[0] - 0.05 * span, edges[-1] + 0.05 * span, 1000000)
    v[::7] = v[::7].astype(np.float32)      # what the kernel sees: widened float32
    on = [edges[0], edges[len(edges) // 2], edges[-1], edges[1], edges[-2]]
    near = [np.nextafter(e, s) for e in on for s in (-np.inf, np.inf)]
    special = np.array(on + near + [np.nan, np.inf, -np.inf, 1000.0], np.float64)
    v = np.concatenate([special, edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), v])
    got, want = dh.bins(v, edges), dh.searchsorted_bins(v, edges)
    assert np.array_equal(got, want), 'first difference at v = %r' % v[np.nonzero(got != want)[0][0]]
    assert got[0] == 0 and got[1] == len(edges) // 2 if len(edges) > 2 else True
    assert got[2] == len(edges) - 2                                  # a value equal to the last edge: the last bin
    k = len(on) + len(near)
    assert (got[k:k + 3] == -1).all()                                # NaN, +inf, -inf
    assert (got >= 0).sum() > 100 and (got < 0).sum() > 100


def test_restatement_equals_histogram2d(g):
    """searchsorted_bins is np.histogram2d's bin: the golden's inputs through np.histogram2d itself give the golden."""
    code = int(g['stranded_code'])
    got = dh.histogram2d_maps(*_inputs(g), g['lon_array'], g['lat_array'], None, code)
    for h, name in zip(got, ('H', 'H_submerged', 'H_stranded')):
        assert np.array_equal(h, g['counts_' + name])
