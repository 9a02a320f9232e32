"""CPU: the arithmetic of StructuredReader.set_convolution_kernel -- readers.convolve_block (NumPy) and the host build of
csrc/odr_convolve.hip.h (tests/convolve_host.cpp: the kernels' own routines, walked tile by tile and strip by strip) -- against what
the reference's __convolve_block__ made of the same blocks (golden C41 part a, tools/gen_golden_reader_convolution.py), bit for
bit, and against scipy.ndimage.convolve where SciPy is installed."""
import numpy as np
import pytest

import convolve_host as H
from opendrift_amd import _abi, readers

CASES = H.block_cases()
IDS = [c[0] for c in CASES]


def test_the_golden_holds_the_cases_the_device_can_get_wrong():
    g = H.golden()
    t = H.tile_edge()
    assert int(g['tile']) == t and H.max_edge() == _abi.CONVOLVE_MAX_EDGE >= 15
    shapes = {name: next(iter(raw.values())).shape[-2:] for name, _, raw, _ in CASES}
    assert {t - 1, t, t + 1} <= {s[0] for s in shapes.values()} and {t - 1, t, t + 1} <= {s[1] for s in shapes.values()}
    assert shapes['n5'][0] == 2 and any(a.ndim == 3 and a.shape[0] == 2 for a in CASES[IDS.index('n3')][2].values())
    assert any(a.ndim == 3 and a.shape[0] == 1 for _, _, raw, _ in CASES for a in raw.values())
    assert any(a.shape[-2] % H.strip() for _, _, raw, _ in CASES for a in raw.values() if a.ndim == 3)      # a strip that ends early
    k35 = CASES[IDS.index('k35')][1]
    assert k35.shape == (3, 5) and (k35 == 0).sum() == 1
    for name, conv, raw, out in CASES:
        for v, a in raw.items():
            if v != 'land_binary_mask':
                assert np.isnan(a).sum() >= 2 and (a == np.float32(1e10)).any() and (a == np.float32(9.99e9)).any(), (name, v)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_convolve_block_equals_the_reference(case):
    name, conv, raw, out = case
    env = {v: a.copy() for v, a in raw.items()}
    env.update(x=np.arange(3.0), y=np.arange(2.0), z=0, time=None)
    got = readers.convolve_block(env, conv)
    assert got is env and np.array_equal(env['x'], np.arange(3.0)) and env['z'] == 0
    for v in raw:
        assert got[v].dtype == np.float32 and H.same_bits(got[v], out[v]), (name, v)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_host_build_of_the_kernels_equals_the_reference(case):
    name, conv, raw, out = case
    k = readers.convolution_weights(conv)
    for v, a in raw.items():
        got = H.convolve(a, k)
        assert H.same_bits(got, out[v]), (name, v, np.argwhere(H.bits(got) != H.bits(out[v]))[:4])


def test_a_nan_under_a_zero_weight_does_not_spread():
    g = H.golden()
    k = CASES[IDS.index('k35')][1]
    want = g['a_zero_out']
    assert np.isnan(want).sum() == k.size - 1
    assert H.same_bits(H.convolve(g['a_zero_raw'], k), want)
    assert H.same_bits(readers.convolve_block({'x_wind': g['a_zero_raw'].copy()}, k)['x_wind'], want)


def test_kernels_up_to_the_largest_edge_and_grids_smaller_than_the_halo():
    """Host build against the NumPy restatement (itself pinned above): the largest kernel, an even-sized one of another width than
    height, on grids smaller than the kernel along either axis and on one of several tiles and strips."""
    rng = np.random.default_rng(5)
    m = H.max_edge()
    for ky, kx in ((m, m), (m, 2), (1, m), (6, 9)):
        k = rng.normal(size=(ky, kx))
        for shape in ((2, 3), (5, 70), (67, 4), (2, 2, 35), (3, 19, 33), (1, 5, 9)):
            a = rng.normal(size=shape).astype(np.float32)
            a.flat[3] = np.nan
            assert H.same_bits(H.convolve(a, k), readers.convolve_block({'v': a.copy()}, k)['v']), (ky, kx, shape)


def test_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(6)
    asym = CASES[IDS.index('k35')][1]
    for conv in (2, 3, 4, 5, asym):
        k = readers.convolution_weights(conv)
        for shape, dtype in (((9, 11), np.float32), ((9, 11), np.float64), ((4, 9, 11), np.float32), ((1, 7, 5), np.float64), ((2, 33), np.float32)):
            a = rng.normal(size=shape).astype(dtype)
            a.flat[7] = np.nan
            want = ndimage.convolve(a, k if a.ndim == 2 else k[:, :, None], mode='nearest')
            got = readers.convolve_block({'v': a.copy()}, conv)['v']
            assert got.dtype == want.dtype and H.same_bits(got, want), (np.shape(conv), shape, dtype)
            if dtype == np.float32:
                assert H.same_bits(H.convolve(a, k), want), (np.shape(conv), shape)
