"""CPU: the cell function and the gradient stencil of csrc/odr_ftle.hip.h, compiled for the host (tests/ftle_host.py), against the
reference's own physics_methods.ftle (tests/golden/c33_ftle.npz (a), written by tools/gen_golden_ftle.py) and against np.gradient.

Measure: max over EVERY finite reference cell of |host - reference| / (1 / |T| + |reference|); -inf and NaN cells must sit at the
same places.  Measured 8.71e-08 over the fields of (a) (1.04e-07 over the maps of (b), tests/test_ftle_host_api.py) on the CPU the
golden was written on; the bound is 4 x the larger, ftle_host.ARITHMETIC_BOUND = 4.16e-07.  The difference is the
reference's float32 eigenvalue (LAPACK), square root and logarithm against one float64 closed form rounded once."""
import numpy as np
import pytest

import ftle_host as fh
from conftest import golden

CASES = ['sheared', 'block', 'small22', 'small29', 'negative']


@pytest.fixture(scope='module')
def g():
    return golden('c33_ftle.npz')


def test_bound_is_four_times_the_measured_value():
    assert fh.ARITHMETIC_BOUND == 4 * fh.ARITHMETIC_MEASURED
    assert fh.ARITHMETIC_BOUND < 100 * 6e-8      # beyond that the restatement would be wrong, not imprecise


@pytest.mark.parametrize('case', CASES)
def test_host_build_equals_reference(g, case):
    dX, dY, T = g['a_%s_dX' % case], g['a_%s_dY' % case], float(g['a_%s_duration' % case])
    want = g['a_%s_ftle' % case]
    got = fh.ftle_map(dX, dY, float(g['a_delta']), T)
    assert got.dtype == np.float32 and got.shape == want.shape == dX.shape
    m = fh.measure(got, want, T)      # asserts identical places of -inf and NaN
    print('%s: %d x %d cells, %d -inf, measure %.3g (bound %.3g)' % (case, dX.shape[0], dX.shape[1], np.isneginf(want).sum(), m,
                                                                    fh.ARITHMETIC_BOUND))
    assert m <= fh.ARITHMETIC_BOUND
    if case == 'block':
        assert np.isneginf(got).sum() == 6
    else:
        assert np.isfinite(got).all()


def test_negative_duration_is_its_absolute_value(g):
    a = fh.ftle_map(g['a_sheared_dX'], g['a_sheared_dY'], float(g['a_delta']), 15.0)
    b = fh.ftle_map(g['a_sheared_dX'], g['a_sheared_dY'], float(g['a_delta']), -15.0)
    assert np.array_equal(a, b)


def test_nan_in_the_stencil_gives_nan(g):
    """the one deviation from the reference, whose LAPACK call raises: corner, edge, interior"""
    for (j, i) in ((0, 0), (0, 17), (11, 20)):
        dX, dY = g['a_sheared_dX'].copy(), g['a_sheared_dY'].copy()
        dX[j, i] = np.nan
        got = fh.ftle_map(dX, dY, float(g['a_delta']), 15.0)
        ny, nx = dX.shape
        want = np.zeros((ny, nx), bool)      # the cells whose np.gradient stencil holds (j, i)
        for jj, ii in ((j, i), (j - 1, i), (j + 1, i), (j, i - 1), (j, i + 1)):
            if 0 <= jj < ny and 0 <= ii < nx:
                want[jj, ii] = True
        want[j, i] = j in (0, ny - 1) or i in (0, nx - 1)      # an interior cell's central differences do not read the cell itself
        assert np.array_equal(np.isnan(got), want), (j, i)
        assert np.array_equal(got[~want], fh.ftle_map(g['a_sheared_dX'], dY, float(g['a_delta']), 15.0)[~want])


@pytest.mark.parametrize('shape', [(2, 2), (2, 5), (3, 3), (65, 7)])
def test_gradient_stencil_is_np_gradient_bit_for_bit(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    f = rng.normal(0, 1, shape) * 10.0 ** rng.integers(-3, 4, shape)
    got, want = fh.gradient(f), np.gradient(f)
    for axis in (0, 1):
        assert want[axis].dtype == np.float64
        assert np.array_equal(got[axis].view(np.uint64), want[axis].view(np.uint64)), (shape, axis)
