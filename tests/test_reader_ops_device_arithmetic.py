"""CPU: the evaluator of csrc/odr_combine.hip.h (comb_program, comb_add, comb_num, comb_blend, comb_gauss_weight, comb_take, comb_check)
compiled for the host, against NumPy doing what the reference's operator classes do with arrays of the same dtype.

Bounds: sums, number-ops and blends are single correctly rounded operations on either side: bit for bit.  The Gaussian weight goes
through exp(), whose last bit may differ between math libraries: one float64 ulp of the weight, plus what 1e-8 m of distance move
it by (d f = f d / std^2 dd); the distance behind it is the device's inverse geodesic against the golden's pyproj distances: 1e-8 m
(tests/test_geodinv_host.py holds it to that)."""
import numpy as np
import pytest

import combine_host as H
from opendrift_amd import _abi as A

SRC, UNI, ADD, GT, GE, NADD, NMUL, NDIV = (A.COMBINE_SOURCE, A.COMBINE_UNIFORM, A.COMBINE_ADD, A.COMBINE_GAUSS_TERM, A.COMBINE_GAUSS_END,
                                           A.COMBINE_NUM_ADD, A.COMBINE_NUM_MUL, A.COMBINE_NUM_DIV)
Z = (0.0, 0.0, 0.0)


@pytest.fixture(scope='module')
def leaves():
    """Four leaves of 1000 float32-representable values over 60 binades, with NaN and infinities among them."""
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((4, 1000)) * 2.0 ** rng.integers(-30, 30, (4, 1000))).astype(np.float32)
    v[0, ::97] = np.nan
    v[1, ::89] = np.nan
    v[2, 5] = np.inf
    return v


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


@pytest.mark.parametrize('cls', [(True, True), (True, False), (False, True), (False, False)])
def test_sum_keeps_the_numpy_dtype(leaves, cls):
    a, b = (leaves[k] if c else leaves[k].astype(np.float64) for k, c in enumerate(cls))
    with np.errstate(invalid='ignore', over='ignore'):
        want = a + b
    got, f32 = H.run_program([(SRC, 0, Z), (SRC, 1, Z), (ADD, 0, Z)], leaves[:2], cls)
    assert f32.all() == (want.dtype == np.float32) and f32.all() == f32.any()
    assert same(got.astype(want.dtype), want) and same(got, want.astype(np.float64))      # (a float32-class value is exactly a float)
    assert np.isnan(got[::97]).all() and np.isnan(got[::89]).all()      # missing where an operand is missing


@pytest.mark.parametrize('kind,n', [(NADD, 5), (NADD, -3), (NMUL, 0.9), (NMUL, 2.5), (NDIV, 2), (NDIV, 3.0)])
@pytest.mark.parametrize('f32', [True, False])
def test_number_ops_are_float64_operations_on_a_masked_operand(leaves, kind, n, f32):
    """number o MaskedArray(float32) is float64 in the reference (golden part 1 asserts it): here too, whatever the class."""
    x = np.ma.masked_invalid(leaves[0] if f32 else leaves[0].astype(np.float64))
    want = n + x if kind == NADD else n * x if kind == NMUL else x / n
    assert want.dtype == np.float64
    got, cls = H.run_program([(SRC, 0, Z), (kind, 0, (n, 0, 0))], leaves[:1], [f32])
    assert not cls.any()
    assert same(got, np.ma.filled(want, np.nan))
    if f32 and n == 0.9:      # ... and not the float32 product
        assert (got.astype(np.float32) != np.float32(0.9) * leaves[0])[np.isfinite(leaves[0])].sum() > 100


def test_nested_sums_and_the_mean_of_two(leaves):
    a, b, c, d = leaves
    with np.errstate(invalid='ignore', over='ignore'):
        want = (a + b) + (c.astype(np.float64) + d)      # float32 sum + float64 sum
        mean = (a + b).astype(np.float64) / 2      # (float64 division of the float32 sum)
    prog = [(SRC, 0, Z), (SRC, 1, Z), (ADD, 0, Z), (SRC, 2, Z), (SRC, 3, Z), (ADD, 0, Z), (ADD, 0, Z)]
    got, cls = H.run_program(prog, leaves, [True, True, False, True])
    assert not cls.any() and same(got, want)
    got, cls = H.run_program([(SRC, 0, Z), (SRC, 1, Z), (ADD, 0, Z), (NDIV, 0, (2, 0, 0))], leaves, [True] * 4)
    assert same(got, mean.astype(np.float64))
    # a left-deep chain of eight leaves holds two values at a time
    chain = [(SRC, 0, Z)] + [op for k in range(1, 8) for op in ((SRC, k % 4, Z), (ADD, 0, Z))]
    got, cls = H.run_program(chain, leaves, [True] * 4)
    with np.errstate(invalid='ignore', over='ignore'):
        acc = a
        for k in range(1, 8):
            acc = acc + leaves[k % 4]
    assert cls.all() and same(got.astype(np.float32), acc)


def test_programs_that_are_refused(leaves):
    five = [(SRC, 0, Z)] * 4
    for prog, reason in ((five, 'more than two saved temporaries'), ([(SRC, 0, Z), (ADD, 0, Z)], 'two operands'),
                         ([(SRC, 0, Z), (SRC, 1, Z)], 'more than one value'), ([(SRC, 9, Z)], 'names no source'),
                         ([(SRC, 0, Z), (NMUL, 0, (2, 0, 0)), (SRC, 1, Z), (ADD, 0, Z)], 'is the root'),
                         ([(SRC, 0, Z), (GT, 0, (4.5, 60.0, 0.0)), (GE, 0, Z)], 'standard deviation above zero'),
                         ([(SRC, 0, Z), (GT, 0, (4.5, 60.0, 10.0))], 'without its end'), ([(SRC, 0, Z)] * 40, '1 .. 32'),
                         ([(UNI, 8, Z)], 'beyond the eight'), ([(99, 0, Z)], 'unknown kind')):
        with pytest.raises(ValueError, match=reason):
            H.run_program(prog, leaves, [True] * 4)


def test_gaussian_weight_and_blend_against_the_goldens_distances():
    g = np.load(H.GOLDEN)
    for tag in ('in', 'all'):
        lon, lat = g['q_%s_lon' % tag], g['q_%s_lat' % tag]
        for k in range(2):
            lon_c, lat_c, std = float(g['ts%d_lon' % k]), float(g['ts%d_lat' % k]), float(g['std'][k])
            f, d = H.gauss_weight(lon, lat, lon_c, lat_c, std)
            want_d = g['gauss_distance_%s_%d' % (tag, k)]
            assert np.abs(d - want_d).max() < 1e-8
            want_f = np.exp(-np.power(want_d / std, 2.) / 2)
            assert (np.abs(f - want_f) <= np.spacing(want_f) + 2 * (want_d / std ** 2) * 1e-8 * want_f).all()
            # the blend over the golden's own leaf values: a (1 - f) + b f, float64 whatever a's class
            a = np.float32(np.sin(np.arange(len(lon))))
            b = 3.25
            got, cls = H.run_program([(SRC, 0, Z), (GT, 0, (lon_c, lat_c, std)), (GE, 0, Z)], [a], [True], lon, lat, uniform=[b])
            assert not cls.any() and same(got, a * (1 - f) + b * f)
    assert H.gauss_weight([4.5], [60.0], 4.5, 60.0, 100.0)[0][0] == 1.0      # at the centre: the measurement itself


def test_blend_with_two_measurements_sums_the_weights():
    """The device program takes several terms (c = a (1 - sum f) + sum b f, readerops.py:117-123); the Python surface hands it one."""
    lon, lat = np.array([4.5, 4.6, 4.8, 5.5]), np.array([60.0, 60.1, 60.2, 61.0])
    a = np.array([1.0, 2.0, 3.0, 4.0])
    f0, f1 = H.gauss_weight(lon, lat, 4.5, 60.0, 12000.0)[0], H.gauss_weight(lon, lat, 4.8, 60.2, 7000.0)[0]
    got, _ = H.run_program([(SRC, 0, Z), (GT, 0, (4.5, 60.0, 12000.0)), (GT, 1, (4.8, 60.2, 7000.0)), (GE, 0, Z)], [a], [False], lon, lat,
                           uniform=[10.0, -20.0])
    assert same(got, a * (1 - (f0 + f1)) + (10.0 * f0 + -20.0 * f1))


def test_both_merge_rules():
    val = np.float32([1, np.nan, 2, np.inf, 3, 4])
    cur = np.float32([9, 9, np.nan, np.nan, np.inf, -9])
    assert list(H.take(val, cur, True)) == [True, False, True, False, True, True]      # first: a finite value replaces
    assert list(H.take(val, cur, False)) == [False, False, True, False, True, False]   # elsewhere: fills what is missing
