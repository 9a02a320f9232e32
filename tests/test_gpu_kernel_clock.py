"""GPU: the device time of a unit's last call (Context.*_last_kernel_ms) belongs to the CONTEXT and is read lazily
(KernelClock, csrc/odr_host.h).

* Two contexts on device 0: what one measures does not move the other's figure; the three launches of a density map in slabs of one
  trajectory are summed (the clock's event pool grows), and the maps equal np.histogram2d.
* The launch of a *_sample call is read when the time is asked for, once: a second read returns the same value; the bare query with no
  point makes it exactly 0.
* A refused call leaves the figure (density and the projected map; ftle, seed and trajectory lengths have this in their own files).
  The wrapper raises ValueError for the library's ODR_ERR_INVALID, which is what a refusal of the arguments returns.
* A measurement nobody read goes with its context."""
from datetime import timedelta

import numpy as np
import pytest

import combine_host as H
from opendrift_amd import readers
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu
LAND, SSH = 'land_binary_mask', 'sea_surface_height'


def ftle_3x3(c):
    xs = ys = 3.0 + 0.05 * np.arange(3)
    X, Y = np.meshgrid(xs, ys)
    out = c.ftle_map(None, xs, ys, 0.05, 3600.0, (X + 0.3 * (Y - 3.0)).astype(np.float32), (Y + 0.01).astype(np.float32))
    assert out.shape == (3, 3)
    return out


def five_elements(c):
    P = c.particles(5)
    P.append([0.2, 0.6, 1.5, 0.1, 0.8], [0.1, 0.3, 0.2, 0.8, 0.8])
    return P


def test_the_figure_belongs_to_the_context(ctx, monkeypatch):
    A, B = ctx, Context(device=0, seed=1)
    try:
        ftle_3x3(A)
        kept = A.ftle_last_kernel_ms()
        assert kept > 0
        monkeypatch.setenv('ODR_DENSITY_SLAB_BYTES', '1')      # one trajectory per slab: three launches
        lon = np.array([[0.5, 1.5], [2.5, 0.5], [1.5, 1.5]], np.float32)
        lat = np.array([[10.5, 11.5], [10.5, 10.5], [11.5, 11.5]], np.float32)
        z = np.array([[0.0, -1.0], [0.0, 0.0], [-2.0, -1.0]], np.float32)
        edges = (np.arange(4.0), 10.0 + np.arange(3.0))
        Hs, Hsub, Hstr = B.density_map(lon, lat, z, np.zeros((3, 2), np.float32), *edges)
        assert A.ftle_last_kernel_ms() == kept
        assert B.ftle_last_kernel_ms() == 0.0
        assert B.density_last_kernel_ms() > 0
        for t in range(2):
            up = z[:, t] >= 0
            assert np.array_equal(Hs[t], np.histogram2d(lon[up, t], lat[up, t], bins=edges)[0]), t
            assert np.array_equal(Hsub[t], np.histogram2d(lon[~up, t], lat[~up, t], bins=edges)[0]), t
        assert Hs.sum() == 3 and Hsub.sum() == 3 and not Hstr.any()
    finally:
        B.close()


def twice_the_same(read):
    first = read()
    assert first > 0 and read() == first


def test_a_sample_is_read_lazily_and_once(ctx):
    P = five_elements(ctx)
    r = readers.ShapeReader([np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])])
    shape = ctx.shape(r.x1, r.y1, r.x2, r.y2, r.poly, r.n_polygons)
    P.shape_sample(shape, True)
    twice_the_same(ctx.shape_last_kernel_ms)
    land = P.env_download(LAND)      # inside, inside, outside the box (never sampled: NaN), inside, outside
    assert list(land[[0, 1, 3, 4]]) == [1.0, 1.0, 1.0, 0.0] and np.isnan(land[2])
    assert shape.contains([], []).shape == (0,)
    assert ctx.shape_last_kernel_ms() == 0.0
    shape.close()

    mesh = ctx.umesh([0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0])
    mesh.set_level(0, 0.0, SSH, np.arange(4.0), False)
    P.umesh_sample(mesh, 0, [SSH], [True])
    twice_the_same(ctx.umesh_last_kernel_ms)
    assert list(P.env_download(SSH)[[0, 1, 3, 4]]) == [0.0, 1.0, 2.0, 3.0]      # the nearest node's value
    assert mesh.nearest([], []).shape == (0,)
    assert ctx.umesh_last_kernel_ms() == 0.0
    mesh.close()
    P.close()

    g = np.load(H.GOLDEN)
    expr, _ = H.cases(g)['a+b']
    b = readers.DeviceReaderBinding(ctx, expr, variables=H.WIND)
    P = ctx.particles(5)
    P.append(g['q_in_lon'][:5], g['q_in_lat'][:5], z=g['q_z'][:5])
    b.sample_combined(P, H.WIND, [True] * len(H.WIND), H.T0 + timedelta(seconds=int(g['call_seconds'])))
    twice_the_same(ctx.combined_last_kernel_ms)
    for v in H.WIND:
        assert H.same_bits(P.env_download(v), g['r_in_a+b_' + v][:5]), v
    P.close()


@pytest.mark.parametrize('unit', ['density', 'proj'])
def test_a_refusal_leaves_the_figure(ctx, unit):
    lon = np.array([[0.5, 1.5], [2.5, 0.5]], np.float32)
    lat, z = lon + 10, np.zeros((2, 2), np.float32)
    if unit == 'density':
        call, read = (lambda xe: ctx.density_map(lon, lat, z, z, xe, 10.0 + np.arange(4.0))), ctx.density_last_kernel_ms
    else:
        call, read = (lambda xe: ctx.density_map_proj(None, lon, lat, z, z, xe, 10.0 + np.arange(4.0))), ctx.conc_last_kernel_ms
    assert call(np.arange(4.0))[0].sum() == 4
    ms = read()
    assert ms > 0
    with pytest.raises(ValueError, match='not strictly increasing'):
        call(np.array([0.0, 2.0, 1.0, 3.0]))
    assert read() == ms


def test_an_unread_measurement_goes_with_its_context(ctx):      # (ctx: the fixture decides whether there is a GPU to test on)
    c = Context(device=0, seed=0)
    want = ftle_3x3(c)
    P = five_elements(c)
    r = readers.ShapeReader([np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])])
    shape = c.shape(r.x1, r.y1, r.x2, r.y2, r.poly, r.n_polygons)
    P.shape_sample(shape, True)
    c.close()      # (the handles of a closed context release nothing)
    c = Context(device=0, seed=0)
    try:
        assert np.array_equal(ftle_3x3(c), want, equal_nan=True) and c.ftle_last_kernel_ms() > 0
    finally:
        c.close()
