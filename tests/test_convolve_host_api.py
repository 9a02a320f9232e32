"""CPU: the reader surface of set_convolution_kernel (readers/basereader/structured.py:163-192) -- what the argument means, what is
refused, and that a reader that never calls it is what it was."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from opendrift_amd import _abi, readers

T0 = datetime(2020, 1, 1)
U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'


def _arrays(nt=2, ny=6, nx=7, nz=None, seed=0):
    rng = np.random.default_rng(seed)
    shape = (nt, ny, nx) if nz is None else (nt, nz, ny, nx)
    return {U: rng.normal(size=shape).astype(np.float32), V: rng.normal(size=shape).astype(np.float32)}


def _times(nt=2):
    return [T0 + timedelta(hours=k) for k in range(nt)]


def _every_kind():
    x, y = np.linspace(3, 5, 7), np.linspace(59, 61, 6)
    lon, lat = np.meshgrid(x, y)
    grid = readers.GridReader(x, y, _times(), _arrays())
    curv = readers.CurvilinearGridReader(lon, lat, _times(), _arrays())
    look = readers.GridReader(np.arange(7.0), np.arange(6.0), _times(), _arrays(), proj4='+proj=eqc', lon=lon, lat=lat)
    sigma = readers.SigmaGridReader(x, y, _times(), _arrays(nz=3), {}, h=np.full((6, 7), 50.0), hc=10.0, Cs_r=np.array([-0.9, -0.5, -0.1]))
    return grid, curv, look, sigma


def test_every_structured_reader_has_the_method_and_starts_without_a_kernel():
    kinds = _every_kind()
    assert [type(r).__name__ for r in kinds] == ['GridReader', 'CurvilinearGridReader', 'NodeLookupGridReader', 'SigmaGridReader']
    for r in kinds:
        assert r.convolve is None and 'convolve' not in vars(r)
        r.set_convolution_kernel(3)
        assert r.convolve == 3
        r.set_convolution_kernel(None)
        assert r.convolve is None
    assert not hasattr(readers.ConstantReader({U: 1.0}), 'set_convolution_kernel')


def test_an_int_means_the_box_mean_formed_as_the_reference_forms_it():
    for n in (1, 2, 3, 5, np.int64(4), np.int32(7)):
        k = readers.convolution_weights(n)
        ones = np.ones((n, n))
        assert k.dtype == np.float64 and np.array_equal(k, ones / ones.sum())
    given = np.array([[1.0, 2.0, 3.0], [0.0, -1.0, 0.5]])
    assert np.array_equal(readers.convolution_weights(given), given)        # taken as given: not normalised
    assert np.array_equal(readers.convolution_weights(given.tolist()), given)


def test_none_switches_it_off_and_an_untouched_block_is_the_same_object():
    block = {k: v[0] for k, v in _arrays().items()}
    before = {k: v.copy() for k, v in block.items()}
    assert readers.convolve_block(block, None) is block
    for k in block:
        assert block[k] is not None and np.array_equal(block[k], before[k])
    r = _every_kind()[0]
    r.set_convolution_kernel(np.ones((3, 3)))
    r.set_convolution_kernel(None)
    assert r.convolve is None
    out = r.get_variables([U, V], T0)
    assert np.array_equal(out[U], r.arrays[U][0])      # get_variables hands out the raw block: the convolution is the upload's


def test_a_kernel_that_does_not_fit_is_refused_by_name():
    r = _every_kind()[0]
    m = _abi.CONVOLVE_MAX_EDGE
    assert m >= 15
    r.set_convolution_kernel(m)
    r.set_convolution_kernel(np.ones((m, 1)))
    for bad in (m + 1, np.ones((m + 1, 3)), np.ones((2, m + 1))):
        with pytest.raises(ValueError, match='grid_reader.*at most %d x %d' % (m, m)):
            r.set_convolution_kernel(bad)
    for bad in (np.ones(3), np.ones((2, 2, 2)), 0):
        with pytest.raises(ValueError, match='2-D array of weights'):
            r.set_convolution_kernel(bad)
    assert r.convolve.shape == (m, 1)      # a refused kernel leaves the one in force


def test_every_variable_but_the_coordinates_is_convolved():
    rng = np.random.default_rng(1)
    land = (rng.uniform(size=(5, 6)) < 0.5).astype(np.float32)
    depth = rng.uniform(10, 90, (5, 6)).astype(np.float32)
    env = {'x': np.arange(6.0), 'y': np.arange(5.0), 'z': np.array([0.0, -5.0]), 'time': T0, 'land_binary_mask': land.copy(),
           'sea_floor_depth_below_sea_level': depth.copy(), U: rng.normal(size=(2, 5, 6)).astype(np.float32)}
    u = env[U].copy()
    readers.convolve_block(env, 3)
    assert np.array_equal(env['x'], np.arange(6.0)) and np.array_equal(env['z'], [0.0, -5.0]) and env['time'] == T0
    assert ((env['land_binary_mask'] > 0) & (env['land_binary_mask'] < 1)).any()      # the mask becomes fractional
    assert not np.array_equal(env['sea_floor_depth_below_sea_level'], depth)
    # a 3-D variable: the kernel's first axis over z, its second over y, x not smoothed -- a field that varies along x only is kept
    ramp = np.broadcast_to(np.arange(6, dtype=np.float32), (2, 5, 6)).copy()
    assert np.array_equal(readers.convolve_block({U: ramp.copy()}, 4)[U], ramp)
    assert not np.array_equal(env[U], u)
    masked = np.ma.masked_array(depth.copy(), mask=np.zeros_like(depth, bool))
    masked.mask[2, 3] = True
    got = readers.convolve_block({'sea_floor_depth_below_sea_level': masked}, 3)['sea_floor_depth_below_sea_level']
    assert np.isnan(got).sum() == 9      # a masked entry counts as NaN and spreads over its footprint
    with pytest.raises(NotImplementedError, match='ensemble members'):
        readers.convolve_block({U: [u[0], u[1]]}, 3)
