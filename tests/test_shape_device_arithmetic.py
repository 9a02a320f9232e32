"""CPU: the arithmetic of csrc/odr_shape.hip.h on its host build (tests/shape_host.cpp).  On every kept query of the golden cases a
to d (tests/golden/c37_shape_landmask.npz: the reference's reader with matplotlib's predicate) three answers must be EQUAL: the
indexed query, the definition over all edges (shape_contains_all_edges) and the golden mask -- with the automatic grid, with one
cell, and with grids far coarser and far finer than the automatic one.  The same on the smallest shapes at which the index can go
wrong (shape_host.edge_shapes): a single triangle, nx = ny = 1, cells that hold only toggles, empty cells, overlapping squares, a
hole with an island, invert, a MultiPolygon given through __geo_interface__, queries outside the box or not finite (NaN) and exactly
on the right and top bound; and a grid whose lines, before the origin is shifted, pass through vertices and along edges."""
import numpy as np
import pytest

import shape_host as S
from opendrift_amd import readers


@pytest.fixture(scope='module')
def g():
    return np.load(S.GOLDEN)


def test_the_golden_file_kept_its_conditions(g):
    for case in 'abcd':
        assert float(g[case + '_min_edge_distance']) > 1e-9 and float(g[case + '_dropped']) < 0.05
    assert float(g['f_smallest_gap_deg']) > 1e-5


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd'])
@pytest.mark.parametrize('grid', [0, 1, 7, 300])
def test_index_definition_and_reference_agree(g, case, grid):
    r = S.golden_reader(g, case)
    lon, lat, want = g[case + '_lon'], g[case + '_lat'], g[case + '_mask']
    x, y = (lon, lat) if case != 'c' else r.lonlat2xy(lon, lat)
    H = S.HostShape(r, grid, grid)
    got, definition = H.contains(x, y), H.all_edges(x, y)
    s = H.stats()
    print(case, grid, s, 'land', int(np.nansum(got)), 'outside', int(np.isnan(got).sum()))
    assert S.same_mask(got, definition)
    assert S.same_mask(got, want)
    assert S.same_mask(r.mask(lon, lat), want)      # ShapeReader's own host answer: the same rule in NumPy
    if grid == 0:
        assert 1.5 * len(r.x1) <= s['cells'] <= 4 * len(r.x1)      # a small multiple of the edge count
        assert s['longest_list'] < len(r.x1) / 4


@pytest.mark.parametrize('name', sorted(S.edge_shapes()))
def test_edge_shapes(name):
    polygons, invert, nx, ny = S.edge_shapes()[name]
    r = readers.ShapeReader(polygons, invert=invert)
    H = S.HostShape(r, nx, ny)
    qx, qy = S.shape_queries(r, 4133, 11)
    got = H.contains(qx, qy)
    assert S.same_mask(got, H.all_edges(qx, qy)) and S.same_mask(got, r.mask(qx, qy))
    x0, x1, y0, y1 = r.box
    outside = ~(np.isfinite(qx + qy) & (qx >= x0) & (qx <= x1) & (qy >= y0) & (qy <= y1))
    assert np.array_equal(np.isnan(got), outside) and outside.sum() > 500 and not outside[-3] and not outside[-1]
    assert 0 < (got == 1).sum() < (~outside).sum()
    s = H.stats()
    if nx:
        assert (s['nx'], s['ny']) == (nx, ny)


def test_expected_values_on_the_shapes():
    sh = S.edge_shapes()
    polygons, invert, nx, ny = sh['overlapping_squares']
    H = S.HostShape(readers.ShapeReader(polygons), nx, ny)
    assert list(H.contains([1.0, 3.0, 5.0, 5.0, 1.0], [1.0, 3.0, 5.0, 1.0, 5.0])) == [1, 1, 1, 0, 0]      # the intersection is land
    polygons, invert, nx, ny = sh['hole_with_island']
    r = readers.ShapeReader(polygons)
    for grid in (0, 1, 2, 9, 40):
        H = S.HostShape(r, grid, grid)
        assert list(H.contains([1.0, 2.5, 4.5, 9.0, 4.5, 9.5], [1.0, 2.5, 4.5, 9.0, 9.0, 1.0])[:5]) == [1, 0, 1, 0, 0], grid      # ring, lake, island, corner, top
        assert np.isnan(H.contains([9.5, np.nan], [1.0, 1.0])).all()
    polygons, invert, nx, ny = sh['inverted']
    H = S.HostShape(readers.ShapeReader(polygons, invert=True), nx, ny)
    assert S.same_mask(H.contains([1.0, 2.5, 4.5, 9.5], [1.0, 2.5, 4.5, 1.0]), [0, 1, 0, np.nan])


def test_cells_with_toggles_only_and_empty_cells():
    polygons, invert, nx, ny = S.edge_shapes()['toggle_and_empty_cells']
    H = S.HostShape(readers.ShapeReader(polygons), nx, ny)
    edges, toggles = H.cell_counts()
    assert ((edges == 0) & (toggles == 1)).sum() >= 20      # deep inside the ring of land
    assert ((edges == 0) & (toggles == 0)).sum() >= 9       # deep inside the lake
    s = H.stats()
    jj, ii = np.nonzero((edges == 0) & (toggles == 1))
    cx, cy = s['x0'] + (ii + 0.5) * s['dx'], s['y0'] + (jj + 0.5) * s['dy']
    assert (H.contains(cx, cy) == 1).all()
    jj, ii = np.nonzero((edges == 0) & (toggles == 0))
    cx, cy = s['x0'] + (ii + 0.5) * s['dx'], s['y0'] + (jj + 0.5) * s['dy']
    inside = (cx > 0) & (cx < 16) & (cy > 0) & (cy < 16)
    assert inside.sum() >= 9 and (H.contains(cx[inside], cy[inside]) == 0).all()


def test_the_origin_is_shifted_off_vertices_and_axis_parallel_edges():
    polygons = S.lines_through_vertices(4, 4)
    r = readers.ShapeReader(polygons)
    H = S.HostShape(r, 4, 4)
    s = H.stats()
    assert s['nudges'] >= 1      # the first origin put lines through vertices and along edges
    lx, ly = s['x0'] + np.arange(5) * s['dx'], s['y0'] + np.arange(5) * s['dy']
    assert not np.isin(np.r_[r.x1, r.x2], lx).any() and not np.isin(np.r_[r.y1, r.y2], ly).any()
    qx, qy = S.shape_queries(r, 4133, 12)
    # with queries on the old lines too
    inner = polygons[0][1][0]
    qx[:6], qy[:6] = inner[:, 0], inner[:, 1] + 0.25
    qx[6:12], qy[6:12] = inner[:, 0] + 0.25, inner[:, 1]
    got = H.contains(qx, qy)
    assert S.same_mask(got, H.all_edges(qx, qy)) and S.same_mask(got, r.mask(qx, qy))
    assert S.HostShape(readers.ShapeReader([polygons[0][0]]), 4, 4).stats()['nudges'] == 0


def test_sample_merges_by_priority():
    r = readers.ShapeReader([np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0], [0.0, 4.0]])])
    H = S.HostShape(r)
    x, y = np.array([1.0, 1.0, 5.0, 5.0, 1.0]), np.array([1.0, 1.0, 1.0, 1.0, np.nan])
    pre = np.array([0.0, np.nan, 0.0, np.nan, 0.5], np.float32)
    assert S.same_mask(H.sample(x, y, True, pre), [1, 1, 0, np.nan, 0.5])       # first: overwrites where it covers
    assert S.same_mask(H.sample(x, y, False, pre), [0, 1, 0, np.nan, 0.5])      # behind another reader: fills what is missing


def test_bad_input_is_refused():
    class E:
        x1, y1, x2, y2 = np.array([0.0, 1.0]), np.array([0.0, 0.0]), np.array([1.0, 1.0]), np.array([0.0, 0.0])
        poly, n_polygons, invert = np.array([0, 0], np.int32), 1, False
    with pytest.raises(ValueError, match='zero length'):
        S.HostShape(E)
    E.y2 = np.array([0.0, np.inf])
    with pytest.raises(ValueError, match='not finite'):
        S.HostShape(E)
    E.y2, E.poly = np.array([0.0, 1.0]), np.array([0, 3], np.int32)
    with pytest.raises(ValueError, match='does not exist'):
        S.HostShape(E)
