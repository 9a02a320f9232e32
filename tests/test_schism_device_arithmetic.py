"""CPU: the arithmetic of opendrift_amd/csrc/odr_schism.hip.h, compiled for the host (tests/schism_host.cpp), against scipy's cKDTree
-- the reference's index -- and against the reference's own answers (tests/golden/c41_schism.npz, written by
tools/gen_golden_schism.py from the reference's reader).

The three nearest and their distances EQUAL cKDTree.query(k=3) bit for bit, in 2-D over the nodes and in 3-D over the columnar cloud
(the same 2-D tree, pruned on the horizontal distance); with duplicated nodes any of the tied indices is accepted and the distances
must be equal.  Values -- weights, time blend, rotation with the reference's own cosine and sine -- are bit-equal to the golden, NaN
placement included."""
from datetime import timedelta

import numpy as np
import pytest
from scipy.spatial import cKDTree

import schism_host as S


@pytest.fixture(scope='module')
def g():
    return np.load(S.GOLDEN)


def zcor_for(n, L, seed, nan_levels=True):
    """[n, L] float32: monotonic columns over depths 20 .. 80 m; a third of the columns lose 1 .. L - 1 levels below the sea bed."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(20, 80, n)
    s = 1.0 - np.arange(L) / max(L - 1, 1) if L > 1 else np.array([0.5])
    z = (rng.uniform(-0.5, 0.5, n)[:, None] - depth[:, None] * s[None, :]).astype(np.float32)
    if nan_levels and L > 1:
        for node in np.flatnonzero(rng.random(n) < 0.34):
            z[node, :rng.integers(1, L)] = np.nan
    return z


def queries(px, py, n, seed):
    rng = np.random.default_rng(seed)
    w, h = max(np.ptp(px), 1.0), max(np.ptp(py), 1.0)
    return rng.uniform(px.min() - 0.1 * w, px.max() + 0.1 * w, n), rng.uniform(py.min() - 0.1 * h, py.max() + 0.1 * h, n), -rng.uniform(-2, 90, n)


@pytest.mark.parametrize('n', [3, 4, 5, 1023, 1024, 1025])
def test_nearest3_in_the_plane_equals_ckdtree(n):
    px, py = S.graded_points(n, 100 + n)
    qx, qy, _ = queries(px, py, 2000, 200 + n)
    idx, dist = S.HostMesh(px, py).nearest3(qx, qy)
    want_d, want_i = cKDTree(np.c_[px, py]).query(np.c_[qx, qy], 3)
    assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)
    assert (np.diff(dist, axis=1) >= 0).all()


@pytest.mark.parametrize('L', [1, 2, 6])
@pytest.mark.parametrize('n', [3, 4, 5, 1023, 1024, 1025])
def test_nearest3_over_the_columns_equals_ckdtree(n, L):
    px, py = S.graded_points(n, 300 + n)
    z = zcor_for(n, L, 400 + n + L)
    if n <= 5:
        z[:3, -1] = np.float32([-0.25, 0.0, 0.125])      # (three finite points at the least)
    qx, qy, qz = queries(px, py, 2000, 500 + n + L)
    idx, dist = S.HostMesh(px, py).nearest3(qx, qy, qz, z)
    cx, cy, cz = S.cloud(px, py, z)
    want_d, want_i = cKDTree(np.c_[cx, cy, cz]).query(np.c_[qx, qy, qz], 3)
    assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)


def test_a_column_of_one_finite_level_and_columns_without_any():
    px, py = S.graded_points(500, 7)
    z = zcor_for(500, 6, 8)
    z[::3, :5] = np.nan      # one finite level
    z[1::7, :] = np.nan      # none at all: the node is not in the cloud
    qx, qy, qz = queries(px, py, 2000, 9)
    idx, dist = S.HostMesh(px, py).nearest3(qx, qy, qz, z)
    cx, cy, cz = S.cloud(px, py, z)
    want_d, want_i = cKDTree(np.c_[cx, cy, cz]).query(np.c_[qx, qy, qz], 3)
    assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)


def test_queries_that_are_not_finite_have_no_neighbour():
    px, py = S.graded_points(300, 11)
    z = zcor_for(300, 6, 12)
    M = S.HostMesh(px, py)
    bad = np.array([np.nan, np.inf, -np.inf])
    for idx, dist in (M.nearest3(bad, np.full(3, py[0])), M.nearest3(np.full(3, px[0]), bad),
                      M.nearest3(np.full(3, px[0]), np.full(3, py[0]), bad[:1].repeat(3), z)):
        assert (idx == -1).all() and np.isinf(dist).all()
    # an infinite depth is infinitely far from every point: none compares
    idx, dist = M.nearest3(px[:2], py[:2], [np.inf, -np.inf], z)
    assert (idx == -1).all()


def test_duplicated_nodes_tie_and_the_distances_are_equal():
    px, py = S.graded_points(600, 5)
    px, py = np.concatenate([px, px[:300]]), np.concatenate([py, py[:300]])
    z = zcor_for(900, 6, 6)
    z[600:] = z[:300]
    qx, qy, qz = queries(px, py, 2000, 7)
    M = S.HostMesh(px, py)
    for (idx, dist), pts, q in ((M.nearest3(qx, qy), np.c_[px, py], np.c_[qx, qy]),
                                (M.nearest3(qx, qy, qz, z), np.c_[S.cloud(px, py, z)], np.c_[qx, qy, qz])):
        want_d, want_i = cKDTree(pts).query(q, 3)
        assert np.array_equal(dist, want_d)
        assert (idx != want_i).any()      # ties do exist, and either index of a tie is right:
        diff = pts[idx] - q[:, None, :]
        d2 = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]
        if pts.shape[1] == 3:
            d2 = d2 + diff[..., 2] * diff[..., 2]
        assert np.array_equal(np.sqrt(d2), want_d)
        assert all(len(set(row)) == 3 for row in idx[:200])


def test_the_column_walk_equals_a_search_over_the_whole_cloud():
    px, py = S.graded_points(1500, 21)
    z = zcor_for(1500, 6, 22)
    qx, qy, qz = queries(px, py, 2000, 23)
    idx, dist, seen = S.HostMesh(px, py).nearest3(qx, qy, qz, z, visits=True)
    cx, cy, cz = S.cloud(px, py, z)
    want_i, want_d = S.brute3(cx, cy, cz, qx, qy, qz)
    assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)
    plane = S.HostMesh(px, py).nearest3(qx, qy, visits=True)[2]
    print('tree nodes visited per query: %.1f over the columns, %.1f in the plane, of %d' % (seen.mean(), plane.mean(), len(px)))
    assert seen.mean() < 4 * plane.mean()


def test_the_hull_test_is_the_shape_readers(g):
    r = S.golden_reader(g, 'a')
    M = S.HostMesh(r.x, r.y, r.hull_x, r.hull_y)
    got = M.covers(g['a_x'], g['a_y'])
    assert np.array_equal(got, r.covers_positions(g['a_x'], g['a_y']))
    inside_time = np.isin(g['a_group'], [0, 1, 2, 3, 4])
    assert np.array_equal(got[inside_time], np.isfinite(g['a_' + S.DEPTH][inside_time]))      # the reference's coverage
    assert not M.covers([np.nan, r.x[0]], [r.y[0], np.inf]).any()


def level_planes(f, case, name, k):
    key = {S.U_: 'u' if case == 'a' else 'du', S.V_: 'v' if case == 'a' else 'dv', S.W_: 'w', S.SSH: 'elev', S.DEPTH: 'depth'}[name]
    return f[key] if f[key].ndim == 1 else f[key][k]


@pytest.mark.parametrize('case', ['a', 'b'])
def test_golden_neighbours_and_values_bit_for_bit(g, case):
    r = S.golden_reader(g, case)
    f = S.mesh_fields(len(r.x))
    M = S.HostMesh(r.x, r.y, r.hull_x, r.hull_y)
    x, y = g[case + '_x'], g[case + '_y']      # the positions as the reference searched with them
    z, group = g[case + '_z'].astype(np.float64), g[case + '_group']
    names = [str(n) for n in g['names_' + case]]
    checked = 0
    for gi, sec in enumerate(g['query_seconds']):
        m = group == gi
        t = S.T0 + timedelta(seconds=int(sec))
        if not r.covers_time(t):
            for n in names:
                assert np.isnan(g['%s_%s' % (case, n)][m]).all()
            continue
        kb, ka, w = r.time_weight(t, names)
        assert w == float(g[case + '_w'][gi]) and (ka is None) == (int(sec) % S.LEVEL_SECONDS == 0)
        cov = M.covers(x[m], y[m])
        k = np.flatnonzero(m)[cov]
        idx, dist = M.nearest3(x[k], y[k])
        assert np.array_equal(idx, g[case + '_i2'][k]) and np.array_equal(dist, g[case + '_d2'][k])
        if case == 'a':
            for key, lev in (('b', kb), ('a', ka)):
                if lev is None:
                    continue
                idx, dist = M.nearest3(x[k], y[k], z[k], f['zcor'][lev])
                assert np.array_equal(idx, g['a_i3' + key][k]) and np.array_equal(dist, g['a_d3' + key][k])
        zb, za = (f['zcor'][kb], f['zcor'][ka if ka is not None else kb]) if case == 'a' else (None, None)
        for n in names:
            before, after = level_planes(f, case, n, kb), None if ka is None else level_planes(f, case, n, ka)
            got = M.sample(x[m], y[m], z[m], before, after, w, zb=zb, za=za)
            assert S.same_bits(got, g['%s_%s' % (case, n)][m]), (case, int(sec), n)
            checked += int(np.isfinite(got).sum())
        if case == 'a':      # the pair, rotated with the cosine and sine the reference used
            pair = lambda lev: [level_planes(f, case, S.U_, lev), level_planes(f, case, S.V_, lev)]
            u, v = M.sample(x[m], y[m], z[m], pair(kb), None if ka is None else pair(ka), w, zb=zb, za=za, cs=g['a_cs'][m], sn=g['a_sn'][m])
            assert S.same_bits(u, g['a_rot_u'][m]) and S.same_bits(v, g['a_rot_v'][m]), int(sec)
            assert np.nanmax(np.abs(u - g['a_' + S.U_][m])) > 1e-3      # the rotation is not a no-op on this mesh
    assert checked > 8000
    on_node = g[case + '_d2'][:int(g[case + '_n_on_node']), 0]      # queries exactly ON a node: the 1e-10 floor
    on_node = on_node[np.isfinite(on_node)]                         # (but those of the groups outside the time coverage)
    assert len(on_node) >= 6 and (on_node == 0).all()


def test_a_nan_neighbour_gives_nan_and_the_merge_rule(g):
    r = S.golden_reader(g, 'a')
    f = S.mesh_fields(len(r.x))
    M = S.HostMesh(r.x, r.y, r.hull_x, r.hull_y)
    dry = np.flatnonzero(np.isnan(f['elev'][0]))[:5]
    x, y = r.x[dry] + 0.5, r.y[dry] + 0.5
    assert M.covers(x, y).all()
    assert np.isnan(M.sample(x, y, np.zeros(5), f['elev'][0])).all()
    # a NaN value keeps what the slot has, first or not; a finite one replaces a finite one only when the reader is first
    have = np.float32([1, 2, 3, 4, 5])
    assert S.same_bits(M.sample(x, y, np.zeros(5), f['elev'][0], out=have), have)
    depth = M.sample(x, y, np.zeros(5), f['depth'])
    assert np.isfinite(depth).all()
    assert S.same_bits(M.sample(x, y, np.zeros(5), f['depth'], out=have, first=False), have)
    assert S.same_bits(M.sample(x, y, np.zeros(5), f['depth'], out=have, first=True), depth)
    hole = np.float32([np.nan, 2, np.nan, 4, 5])
    assert S.same_bits(M.sample(x, y, np.zeros(5), f['depth'], out=hole, first=False), np.where(np.isnan(hole), depth, hole))
