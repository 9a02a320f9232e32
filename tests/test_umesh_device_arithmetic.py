"""CPU: the unstructured-mesh arithmetic of opendrift_amd/csrc/odr_umesh.hip.h, compiled for the host (tests/umesh_host.cpp), against
scipy's cKDTree -- the reference's index -- and against the reference's own answers (tests/golden/c36_unstructured.npz, written by
tools/gen_golden_umesh.py from the reference's reader).

Indices must EQUAL the reference's except where NumPy's float64 dx*dx + dy*dy of the two candidates are equal or adjacent floats
(umesh_host.unexcused_mismatches); with the random inputs used here no such case exists, and the tests assert that the count of
excused mismatches is 0 too.  Un-rotated values and sigma indices are bit-equal to the golden, NaN placement included.  Rotated
pairs: within one float32 ulp of max(|u|, |v|) -- one rounding of a float64 product whose angle agrees to ~1e-9 rad."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import umesh_host as U

SIZES = [1, 2, 3, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2000]      # one below, at and above powers of two: the last tree level


def ckd(px, py, qx, qy):
    return cKDTree(np.c_[px, py]).query(np.c_[qx, qy], k=1)[1]


@pytest.mark.parametrize('n', SIZES)
def test_nearest_equals_ckdtree_on_a_graded_mesh(n):
    px, py = U.graded_points(n, 100 + n)
    qx, qy = U.queries(px, py, 4133, 200 + n)      # 2 % of them up to 1e4 box sizes away
    got = U.HostIndex(px, py).nearest(qx, qy)
    bad, excused = U.unexcused_mismatches(px, py, qx, qy, got, ckd(px, py, qx, qy))
    assert (bad, excused) == (0, 0)
    assert np.array_equal(got, U.brute_nearest(px, py, qx, qy))


def test_the_tree_is_left_balanced_and_complete():
    for n in SIZES:
        px, py = U.graded_points(n, n)
        tx, ty, ident = U.HostIndex(px, py).layout()
        assert sorted(ident) == list(range(n))
        assert np.array_equal(tx, px[ident]) and np.array_equal(ty, py[ident])
        for k in range(n):      # every node splits its subtree on the axis of its depth
            axis = (int(np.floor(np.log2(k + 1)))) & 1
            c, ck = (ty, ty[k]) if axis else (tx, tx[k])
            for child, side in ((2 * k + 1, -1), (2 * k + 2, 1)):
                stack = [child] if child < n else []
                while stack:
                    j = stack.pop()
                    assert (c[j] - ck) * side >= 0
                    stack += [m for m in (2 * j + 1, 2 * j + 2) if m < n]
            if n > 300:      # (the whole check is quadratic: the first levels of the larger trees)
                if k > 30:
                    break


def test_duplicated_points_give_the_same_distances():
    px, py = U.graded_points(600, 5)
    px, py = np.concatenate([px, px[:300], px[:100]]), np.concatenate([py, py[:300], py[:100]])
    qx, qy = U.queries(px, py, 3001, 6)
    qx[:50], qy[:50] = px[:50], py[:50]      # on the duplicated points themselves
    got, d2 = U.HostIndex(px, py).nearest(qx, qy, distances=True)
    want = ckd(px, py, qx, qy)
    assert np.array_equal(U.dist2(px[got], py[got], qx, qy), U.dist2(px[want], py[want], qx, qy))
    assert np.array_equal(d2, U.dist2(px[got], py[got], qx, qy))


def test_queries_that_are_not_finite_find_nothing():
    px, py = U.graded_points(100, 1)
    got = U.HostIndex(px, py).nearest([np.nan, np.inf, px[3], -np.inf], [py[0], py[0], np.nan, np.inf])
    assert list(got) == [-1, -1, -1, -1]


@pytest.fixture(scope='module')
def g():
    return np.load(U.GOLDEN)


def mesh_of(g, case):
    x, y, xc, yc = g['x'], g['y'], g['xc'], g['yc']
    if case == 'b':
        (x, y), (xc, yc) = U.latlong_mesh(x, y), U.latlong_mesh(xc, yc)
    return x, y, xc, yc


def positions(g, case):
    if case == 'a':
        return g['a_x'], g['a_y']
    lon = g['b_lon']
    return np.mod(lon + 180, 360) - 180, g['b_lat']


@pytest.mark.parametrize('case', ['a', 'b'])
def test_golden_indices(g, case):
    x, y, xc, yc = mesh_of(g, case)
    qx, qy = positions(g, case)
    for px, py, key in ((x, y, 'node'), (xc, yc, 'face')):
        got = U.HostIndex(px, py).nearest(qx, qy)
        bad, excused = U.unexcused_mismatches(px, py, qx, qy, got, g['%s_%s' % (case, key)])
        print(case, key, 'mismatches', bad, 'excused', excused)
        assert (bad, excused) == (0, 0)


@pytest.mark.parametrize('case', ['a', 'b'])
def test_golden_values_and_sigma_indices_bit_for_bit(g, case):
    x, y, xc, yc = mesh_of(g, case)
    f = U.mesh_fields(len(x), len(xc))
    qx, qy = positions(g, case)
    z, group = g[case + '_z'].astype(np.float64), g[case + '_group']
    box = [x.min(), x.max(), y.min(), y.max()]
    node, face = U.HostIndex(x, y).nearest(qx, qy), U.HostIndex(xc, yc).nearest(qx, qy)
    seconds, last = g['query_seconds'], U.LEVEL_SECONDS * (U.N_TIMES - 1)
    sigma_keys = {'x_sea_water_velocity': 'sig_face_lay', 'sea_water_temperature': 'sig_node_lev', 'sea_water_salinity': 'sig_node_lay'}
    for name in [str(n) for n in g['names']]:
        on_faces = name in f['face_arrays']
        a = (f['face_arrays'] if on_faces else f['node_arrays'])[name]
        lay = a.shape[1] == U.N_SIGLAY
        sigma = f[('siglay' if lay else 'siglev') + ('_center' if on_faces else '')]
        h = f['h_center' if on_faces else 'h']
        out, sig = np.full(len(qx), np.nan, np.float32), np.full(len(qx), -1, np.int32)
        for k, sec in enumerate(seconds):
            m = group == k
            if sec < 0 or sec > last:      # outside the time coverage: the model does not ask the reader
                continue
            level = min(U.N_TIMES - 1, int((2 * sec + U.LEVEL_SECONDS) // (2 * U.LEVEL_SECONDS)))      # nearest, midway: the later
            out[m], sig[m] = U.sample(qx[m], qy[m], z[m], (face if on_faces else node)[m], box, a[level], sigma, h)
        assert U.same_bits(out, g['%s_%s' % (case, name)]), name
        if name in sigma_keys:
            assert np.array_equal(sig, g['%s_%s' % (case, sigma_keys[name])]), name
    assert np.isnan(g[case + '_x_sea_water_velocity']).sum() > 1000      # outside the box, outside the time range


def test_golden_rotation_within_one_float32_ulp(g):
    u, v, rot = g['a_x_sea_water_velocity'], g['a_y_sea_water_velocity'], g['a_rot']
    ok = np.isfinite(u)
    ur, vr = U.rotate(u[ok], v[ok], np.cos(rot[ok]), np.sin(rot[ok]))
    bound = U.ulp32(np.maximum(np.abs(u[ok]), np.abs(v[ok])))
    du, dv = np.abs(ur.astype(np.float64) - g['a_rot_u'][ok]), np.abs(vr.astype(np.float64) - g['a_rot_v'][ok])
    print('rotated u, v against the reference: %.3g, %.3g of one float32 ulp of max(|u|, |v|)' % ((du / bound).max(), (dv / bound).max()))
    assert (du <= bound).all() and (dv <= bound).all()
    assert np.abs(ur - u[ok]).max() > 1e-3      # the rotation is not a no-op on this mesh


def test_the_merge_rule():
    x = np.zeros(4)
    data = np.array([5.0, np.nan], np.float32)
    cur = np.array([1.0, np.nan, 1.0, np.nan], np.float32)
    idx = np.array([0, 0, 1, 1], np.int32)
    box = [-1, 1, -1, 1]
    first, _ = U.sample(x, x, x, idx, box, data, first=True, out=cur)
    second, _ = U.sample(x, x, x, idx, box, data, first=False, out=cur)
    assert U.same_bits(first, [5, 5, 1, np.nan]) and U.same_bits(second, [1, 5, 1, np.nan])
    outside, _ = U.sample(x + 2, x, x, idx, box, data, first=True, out=cur)
    assert U.same_bits(outside, cur)
    notfinite, _ = U.sample(x + np.inf, x - np.inf, x, idx, box, data, first=True, out=cur)      # x + y is NaN
    assert U.same_bits(notfinite, cur)


def test_sigma_index_takes_the_first_minimum():
    sigma = np.array([[0.0], [-0.25], [-0.5], [-0.75], [-1.0]], np.float32)
    h = np.array([8.0], np.float32)
    data = np.arange(5, dtype=np.float32)[:, None]
    z = np.array([0.5, 0.0, -1.0, -3.0, -7.9, -100.0])      # -1 is midway between levels 0 and 1, -3 between 1 and 2
    n = len(z)
    out, sig = U.sample(np.zeros(n), np.zeros(n), z, np.zeros(n, np.int32), [-1, 1, -1, 1], data, sigma, h)
    assert list(sig) == [0, 0, 0, 1, 4, 4] and list(out) == [0, 0, 0, 1, 4, 4]
