"""GPU: readers.SchismReader on the device -- odr_schism_nearest3 and odr_schism_sample (csrc/odr_schism.hip.h) against scipy's
cKDTree, against the reference's own answers (tests/golden/c41_schism.npz) and against the host mirror: neighbours and distances bit
for bit, values bit for bit with their NaN placement; the merge rule; the ABI's refusals; the priority rule next to a GridReader; a
time level that changes mid-run; the reference's OceanDrift runs within 1e-7 deg; the device lane against the host-evaluated lane;
repeatability.

Shapes: 3 and 4 nodes; one below, at and above a power of two (the last tree level); the graded mesh; 2^20 + 77 queries (two
launches of the bare query); element counts 1, 63, 64, 65 and 1025 (wave and workgroup edges of a one-lane-per-element launch)."""
from datetime import timedelta

import numpy as np
import pytest
from scipy.spatial import cKDTree

import schism_host as S
from opendrift_amd import readers
from opendrift_amd._abi import OdrError, check
from opendrift_amd.oceandrift import OceanDrift

pytestmark = pytest.mark.gpu
T0, U_, V_, W_, SSH, DEPTH = S.T0, S.U_, S.V_, S.W_, S.SSH, S.DEPTH


@pytest.fixture(scope='module')
def g():
    return np.load(S.GOLDEN)


def hull_of(px, py):
    from scipy.spatial import ConvexHull
    ring = ConvexHull(np.c_[px, py]).vertices
    return px[ring], py[ring]


def zcor_for(n, L, seed):
    rng = np.random.default_rng(seed)
    z = (rng.uniform(-0.5, 0.5, n)[:, None] - rng.uniform(20, 80, n)[:, None] * (1.0 - np.arange(L) / (L - 1))[None, :]).astype(np.float32)
    for node in np.flatnonzero(rng.random(n) < 0.34)[1:]:
        z[node, :rng.integers(1, L)] = np.nan
    return z


def queries(px, py, n, seed):
    rng = np.random.default_rng(seed)
    w, h = np.ptp(px), np.ptp(py)
    return rng.uniform(px.min() - 0.1 * w, px.max() + 0.1 * w, n), rng.uniform(py.min() - 0.1 * h, py.max() + 0.1 * h, n), -rng.uniform(-2, 90, n)


@pytest.mark.parametrize('n', [3, 4, 1023, 1024, 1025, 2000])
def test_nearest3_equals_ckdtree(ctx, n):
    px, py = S.graded_points(n, 100 + n)
    z = zcor_for(n, 6, 300 + n)
    qx, qy, qz = queries(px, py, 4133, 200 + n)
    mesh = ctx.schism(px, py, *hull_of(px, py), n_levels=6)
    mesh.set_zcor(1, 0.0, z)
    idx, dist = mesh.nearest3(qx, qy)
    want_d, want_i = cKDTree(np.c_[px, py]).query(np.c_[qx, qy], 3)
    assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)
    assert ctx.schism_last_kernel_ms() > 0
    idx, dist, seen = mesh.nearest3(qx, qy, qz, slot=1, visits=True)
    want_d, want_i = cKDTree(np.c_[S.cloud(px, py, z)]).query(np.c_[qx, qy, qz], 3)
    assert np.array_equal(idx, want_i) and np.array_equal(dist, want_d)
    host = S.HostMesh(px, py).nearest3(qx, qy, qz, z, visits=True)      # the host build of the same header
    assert np.array_equal(idx, host[0]) and np.array_equal(dist, host[1]) and np.array_equal(seen, host[2])
    mesh.close()


def test_nearest3_over_two_launches_and_queries_that_are_not_finite(ctx):
    px, py = S.graded_points(600, 5)
    z = zcor_for(600, 6, 6)
    n = (1 << 20) + 77
    rng = np.random.default_rng(8)
    qx, qy, qz = rng.uniform(px.min(), px.max(), n), rng.uniform(py.min(), py.max(), n), -rng.uniform(0, 85, n)
    qx[-3:], qy[-3:] = [np.nan, np.inf, px[0]], [py[0], py[0], -np.inf]
    mesh = ctx.schism(px, py, *hull_of(px, py), n_levels=6)
    mesh.set_zcor(0, 0.0, z)
    for (idx, dist), pts, q in ((mesh.nearest3(qx, qy), np.c_[px, py], np.c_[qx, qy]),
                                (mesh.nearest3(qx, qy, qz), np.c_[S.cloud(px, py, z)], np.c_[qx, qy, qz])):
        assert (idx[-3:] == -1).all() and np.isinf(dist[-3:]).all()
        want_d, want_i = cKDTree(pts).query(q[:-3], 3, workers=16)
        assert np.array_equal(idx[:-3], want_i) and np.array_equal(dist[:-3], want_d)
    idx, dist = mesh.nearest3(px[:2], py[:2], [np.nan, -np.inf])      # a depth that is not finite
    assert (idx == -1).all()
    mesh.close()


def sample(b, ctx, variables, t, lon, lat, z, first=True, preset=None):
    P = ctx.particles(len(lon))
    P.append(lon, lat, z=z)
    for v, a in (preset or {}).items():
        P.env_upload(v, a)
    b.sample_mesh(P, variables, [first] * len(variables), t)
    out = {v: P.env_download(v) for v in variables} if b.reader.covers_time(t) or preset else \
        {v: np.full(len(lon), np.nan, np.float32) for v in variables}      # nothing was launched: the slots were never written
    P.close()
    return out


def agree(have, want, stable=None, bound=None):
    """The criterion for values sampled through longitude and latitude: NaN where the golden has NaN; the golden's bits wherever
    the golden flags the answer as independent of the last bits of the projection (`stable`; None: everywhere); at the others the
    golden's float32 or its neighbour (bound None: one ulp of the value).  Returns (values that differ, unflagged among them)."""
    have, want = np.asarray(have, np.float32), np.asarray(want, np.float32)
    stable = np.ones(len(want), bool) if stable is None else stable
    assert np.array_equal(np.isnan(have), np.isnan(want))
    ok = np.isfinite(want)
    differ = ok & (have != want)
    bound = S.ulp32(want) if bound is None else bound
    assert not (differ & stable).any(), (int((differ & stable).sum()), int(ok.sum()))
    assert (np.abs(have[differ].astype(np.float64) - want[differ]) <= bound[differ]).all()
    return int(differ.sum()), int((ok & ~stable).sum())


@pytest.mark.parametrize('case', ['a', 'b'])
def test_particles_sampling_equals_the_reference(ctx, g, case):
    """Un-rotated values against the golden (u without v and v alone are not rotated), at a level, between levels, midway: every
    value of the geographic mesh (b) bit for bit; of the UTM mesh (a) bit for bit at the queries the golden flags a_stable.  The
    elements are given by longitude and latitude, and the device's UTM series and the reference's differ in the last bits of x, y
    (5e-9 m): at the 5 % of the covered queries where a shift of 2e-8 m carries one of the five values across a float32 rounding
    boundary in the REFERENCE ITSELF (tools/gen_golden_schism.py asks it), the golden's float32 or its neighbour is right.  With
    the positions the reference searched with, the same arithmetic gives the golden's bits at every query
    (tests/test_schism_device_arithmetic.py)."""
    r = S.golden_reader(g, case)
    b = readers.DeviceReaderBinding(ctx, r)
    assert b.sid is None and b.mesh is not None and not b.is_grid()
    names = [str(n) for n in g['names_' + case]]
    rest = [n for n in names if n != V_]
    differ = flagged = finite = 0
    for k, sec in enumerate(g['query_seconds']):
        m = g[case + '_group'] == k
        t = T0 + timedelta(seconds=int(sec))
        lon, lat, z = g[case + '_lon'][m], g[case + '_lat'][m], g[case + '_z'][m].astype(np.float64)
        got = {}
        for vs in (rest, [V_]):
            got.update(sample(b, ctx, vs, t, lon, lat, z))
        for n in names:
            want = g['%s_%s' % (case, n)][m]
            d, f = agree(got[n], want, g['a_stable'][m] if case == 'a' else None)
            differ, flagged, finite = differ + d, flagged + f, finite + int(np.isfinite(want).sum())
        if case == 'b':      # a geographic mesh is not rotated
            pair = sample(b, ctx, [U_, V_], t, lon, lat, z)
            assert S.same_bits(pair[U_], got[U_]) and S.same_bits(pair[V_], got[V_])
    print(case, '%d finite values, %d at flagged queries, %d differ from the golden (by one ulp)' % (finite, flagged, differ))
    assert finite > 8000 and flagged < 0.06 * finite and len(b.mesh_slots) <= 4
    assert case == 'a' or differ == 0


def test_rotated_pairs_equal_the_reference(ctx, g):
    """u and v of (a) sampled together: rotated to east / north, against the reference's rotated values bit for bit at the queries
    the golden flags a_rot_stable: those whose rotated float32 values stay when the position moves by 2e-8 m or the angle by
    1.5e-10 rad, over three times what the reference's own numerically formed angle scatters by.  At the others (8 % of the
    covered): within one float32 ulp of max(|u|, |v|), the criterion of the nearest-node reader -- one rounding of a float64
    product."""
    r = S.golden_reader(g, 'a', variables=(U_, V_))
    b = readers.DeviceReaderBinding(ctx, r)
    differ = flagged = finite = 0
    for k, sec in enumerate(g['query_seconds']):
        m = g['a_group'] == k
        t = T0 + timedelta(seconds=int(sec))
        got = sample(b, ctx, [U_, V_], t, g['a_lon'][m], g['a_lat'][m], g['a_z'][m].astype(np.float64))
        bound = S.ulp32(np.maximum(np.abs(g['a_' + U_][m]), np.abs(g['a_' + V_][m])))
        for n, key in ((U_, 'a_rot_u'), (V_, 'a_rot_v')):
            d, f = agree(got[n], g[key][m], g['a_rot_stable'][m], bound)
            differ, flagged, finite = differ + d, flagged + f, finite + int(np.isfinite(g[key][m]).sum())
        if r.covers_time(t):
            assert np.nanmax(np.abs(got[U_] - g['a_' + U_][m])) > 1e-3      # the rotation is not a no-op on this mesh
    print('rotated pairs: %d finite values, %d at flagged queries, %d differ from the golden' % (finite, flagged, differ))
    assert finite > 3000 and flagged < 0.09 * finite


def test_uncovered_slots_are_untouched_and_the_merge_rule(ctx, g):
    r = S.golden_reader(g, 'a')
    b = readers.DeviceReaderBinding(ctx, r)
    m = g['a_group'] == 1
    t = T0 + timedelta(seconds=1200)
    lon, lat, z = g['a_lon'][m], g['a_lat'][m], g['a_z'][m].astype(np.float64)
    want = g['a_' + SSH][m]
    n = int(m.sum())
    have = np.arange(n, dtype=np.float32)
    hole = have.copy()
    hole[::3] = np.nan
    assert np.isnan(want).sum() > 100 and np.isfinite(want).sum() > 100      # outside the hull or a dry neighbour; inside
    mine = sample(b, ctx, [SSH], t, lon, lat, z)[SSH]      # (the values themselves: test_particles_sampling_equals_the_reference)
    assert np.array_equal(np.isnan(mine), np.isnan(want))
    first = sample(b, ctx, [SSH], t, lon, lat, z, first=True, preset={SSH: have})[SSH]
    assert S.same_bits(first, np.where(np.isfinite(want), mine, have))
    second = sample(b, ctx, [SSH], t, lon, lat, z, first=False, preset={SSH: hole})[SSH]
    assert S.same_bits(second, np.where(np.isnan(hole) & np.isfinite(want), mine, hole))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1025])
def test_element_counts_at_the_wave_and_workgroup_edges(ctx, g, n):
    """Against the host mirror bit for bit.  3-D: the covered queries of (a) that the golden flags a_stable (their values do not
    hang on the last bits of the projection), at their own time and repeated up to n; the mirror is asked at the golden's x, y.
    2-D: the geographic mesh of (b), between two levels."""
    for case, names in (('a', [U_, W_, SSH, DEPTH]), ('b', [U_, V_, SSH, DEPTH])):      # (a: u alone is not rotated)
        r = S.golden_reader(g, case)
        b = readers.DeviceReaderBinding(ctx, r)
        if case == 'a':      # the flag holds at the query's own time: the group asked at 1 200 s
            t = T0 + timedelta(seconds=1200)
            pool = np.flatnonzero((g['a_group'] == 1) & np.isfinite(g['a_' + DEPTH]) & g['a_stable'])
            assert len(pool) > 256
            keep = np.resize(pool, n)
        else:
            t = T0 + timedelta(seconds=1500)
            keep = np.flatnonzero(np.isfinite(g['b_' + DEPTH]))[:n]
            assert len(keep) == n
        lon, lat, z = g[case + '_lon'][keep], g[case + '_lat'][keep], g[case + '_z'][keep].astype(np.float64)
        got = sample(b, ctx, names, t, lon, lat, z)
        want = r.get_variables(names, t, g[case + '_x'][keep], g[case + '_y'][keep], z, rotate=False)
        for v in names:
            assert S.same_bits(got[v], want[v]), (case, n, v)


def test_abi_errors(ctx, g):
    r = S.golden_reader(g, 'a')
    f = S.mesh_fields(len(r.x))
    N = len(r.x)
    with pytest.raises(ValueError, match='node coordinates'):
        ctx.schism(r.x, r.y[:-1], r.hull_x, r.hull_y)
    with pytest.raises(ValueError, match='2 nodes'):
        ctx.schism(r.x[:2], r.y[:2], r.hull_x, r.hull_y)
    with pytest.raises(ValueError, match='hull of 2'):
        ctx.schism(r.x, r.y, r.hull_x[:2], r.hull_y[:2])
    with pytest.raises(ValueError, match='200 vertical levels'):
        ctx.schism(r.x, r.y, r.hull_x, r.hull_y, n_levels=200)
    with pytest.raises(ValueError, match='not finite'):
        ctx.schism(np.r_[r.x[:-1], np.nan], r.y, r.hull_x, r.hull_y)
    flat = ctx.schism(r.x, r.y, r.hull_x, r.hull_y)      # no vertical levels
    with pytest.raises(ValueError, match='zcor of shape'):
        flat.set_zcor(0, 0.0, f['zcor'][0])
    mesh = ctx.schism(r.x, r.y, r.hull_x, r.hull_y, n_levels=S.N_LEVELS)
    with pytest.raises(ValueError, match='slot 4'):      # a fifth resident level
        mesh.set_level(4, 0.0, SSH, f['elev'][0])
    with pytest.raises(ValueError, match='slot 4'):
        mesh.set_zcor(4, 0.0, f['zcor'][0])
    with pytest.raises(ValueError, match='on a mesh of'):
        mesh.set_level(0, 0.0, SSH, np.zeros(N + 1))
    with pytest.raises(ValueError, match='on a mesh of'):
        mesh.set_level(0, 0.0, U_, np.zeros((N, S.N_LEVELS + 1)))
    with pytest.raises(ValueError, match='fewer|finite entries'):
        mesh.set_zcor(0, 0.0, np.full((N, S.N_LEVELS), np.nan))
    with pytest.raises(ValueError, match='NULL'):
        check(ctx.lib.odr_schism_set_level(ctx.h, mesh.ptr, 0, 0.0, 0, 0, None))
    with pytest.raises(ValueError, match='NULL'):
        check(ctx.lib.odr_schism_set_zcor(ctx.h, mesh.ptr, 0, 0.0, None))
    P = ctx.particles(4)
    P.append([14.0] * 4, [58.6] * 4)
    with pytest.raises(ValueError, match='NULL'):
        check(ctx.lib.odr_schism_sample(ctx.h, P.h, None, 0, -1, 0.0, 1, None, None))
    mesh.set_level(0, 0.0, SSH, f['elev'][0])
    mesh.set_level(0, 0.0, U_, f['u'][0])
    with pytest.raises(ValueError, match='slot 5'):
        P.schism_sample(mesh, 5, None, 0.0, [SSH], [True])
    with pytest.raises(ValueError, match='slot 4'):
        P.schism_sample(mesh, 0, 4, 0.5, [SSH], [True])
    with pytest.raises(ValueError, match='time weight'):
        P.schism_sample(mesh, 0, 0, 1.5, [SSH], [True])
    with pytest.raises(ValueError, match='9 variables'):
        P.schism_sample(mesh, 0, None, 0.0, list(range(9)), [True] * 9)
    with pytest.raises(ValueError, match='given twice'):
        P.schism_sample(mesh, 0, None, 0.0, [SSH] * 2, [True] * 2)
    with pytest.raises(ValueError, match='first flags'):
        P.schism_sample(mesh, 0, None, 0.0, [SSH], [True, False])
    with pytest.raises(OdrError, match='does not hold variable'):
        P.schism_sample(mesh, 0, None, 0.0, ['x_wind'], [True])
    with pytest.raises(OdrError, match='does not hold variable'):      # the level after is empty
        P.schism_sample(mesh, 0, 1, 0.5, [SSH], [True])
    with pytest.raises(OdrError, match='without zcor'):
        P.schism_sample(mesh, 0, None, 0.0, [U_], [True])
    with pytest.raises(OdrError, match='without zcor'):
        mesh.nearest3(r.x[:2], r.y[:2], [0.0, 0.0], slot=2)
    P.close()
    mesh.close()
    flat.close()


def wind_mesh(g):
    """The golden's geographic mesh with a wind on its nodes, [N]: static in time."""
    x, y = S.latlong_mesh(g['x'], g['y'])
    k = np.arange(len(x))
    wind = {'x_wind': (5.0 + S._unit(k, 7)).astype(np.float32), 'y_wind': (-2.0 + S._unit(k, 8)).astype(np.float32)}
    return readers.SchismReader(x, y, [T0, T0 + timedelta(hours=6)], wind, name='wind_mesh')


@pytest.mark.parametrize('mesh_first', [True, False])
def test_priority_next_to_a_grid_reader(g, mesh_first):
    """Elements in both readers, in the mesh alone, in the grid alone, in neither.  The mesh first: its values wherever it covers,
    the grid's elsewhere; the mesh second: it fills only what the grid left without a finite value."""
    mesh = wind_mesh(g)      # 4 .. 4.4 E, 60 .. 60.2 N
    gx, gy = np.linspace(3.8, 4.2, 11), np.linspace(59.8, 60.3, 12)
    times = [T0, T0 + timedelta(hours=6)]
    grid = readers.GridReader(gx, gy, times, {'x_wind': np.full((2, 12, 11), 3.0, np.float32), 'y_wind': np.full((2, 12, 11), 4.0, np.float32)})
    o = OceanDrift(loglevel=50, seed=0)
    o.add_reader([mesh, grid] if mesh_first else [grid, mesh])
    o.set_config('environment:constant:land_binary_mask', 0)
    for v, value in (('x_wind', -7.0), ('y_wind', -8.0)):
        o.set_config('environment:fallback:%s' % v, value if mesh_first else None)
    # (float32 values: the elements hold their seeded positions as float32, as the reference's do)
    lon = np.float32([4.1, 4.15, 4.3, 4.35, 3.9, 4.6][:6 if mesh_first else 5]).astype(np.float64)
    lat = np.float32([60.1, 60.15, 60.1, 60.05, 59.9, 59.9][:6 if mesh_first else 5]).astype(np.float64)
    o.seed_elements(lon=lon, lat=lat, time=T0, wind_drift_factor=0.0)      # nothing moves: no current, no windage
    o.run(time_step=600, steps=2)
    assert o._run_lane() == 'call_by_call'
    e, env = o.elements, o.environment
    assert list(e.ID) == list(range(len(lon))) and np.abs(e.lon - lon).max() < 1e-9 and np.abs(e.lat - lat).max() < 1e-9
    # the environment is that of the run's last get_environment call: the last step's, or a closing one at the end time
    mirror = [mesh.get_variables_interpolated(['x_wind', 'y_wind'], T0 + timedelta(seconds=s), lon, lat, np.zeros(len(lon))) for s in (600, 1200)]
    own = next(c for c in mirror if S.same_bits(env.x_wind[2:4], c['x_wind'][2:4]))
    in_mesh, in_grid = np.isfinite(own['x_wind']), lon < 4.2
    assert list(in_mesh) == [True, True, True, True, False, False][:len(lon)]
    for v, gridval, fallback in (('x_wind', 3.0, -7.0), ('y_wind', 4.0, -8.0)):
        if mesh_first:
            want = np.where(in_mesh, own[v], np.where(in_grid, gridval, fallback))
        else:
            want = np.where(in_grid, gridval, own[v])
        from_mesh = in_mesh if mesh_first else in_mesh & ~in_grid
        have = getattr(env, v)
        assert S.same_bits(have[from_mesh], want[from_mesh].astype(np.float32)), (v, have, want)      # the mesh's values: bit for bit
        assert np.allclose(have, want, rtol=1e-6, atol=0), (v, have, want)
    assert len(set(getattr(env, 'x_wind'))) >= 3


def test_the_time_level_changes_mid_run(ctx, g):
    """Euler steps of 30 minutes across all three levels: the model's run against the same steps made by hand -- the levels
    uploaded to a mesh of its own, one odr_schism_sample per step with the bracketing slots and their weight."""
    r = S.golden_reader(g, 'b', variables=(U_, V_))
    o = OceanDrift(loglevel=50, seed=0)
    o.add_reader(r)
    o.set_config('environment:constant:land_binary_mask', 0)
    lon, lat = np.array([4.0625, 4.125, 4.15625]), np.array([60.0625, 60.125, 60.09375])      # (exact in float32)
    o.seed_elements(lon=lon, lat=lat, time=T0, wind_drift_factor=0.0)
    o.run(time_step=1800, steps=4)
    e = o.elements
    b = next(iter(o.readers.values()))
    assert 2 in b.mesh_slots and len(b.mesh_slots) <= 4
    mesh = ctx.schism(r.x, r.y, r.hull_x, r.hull_y)
    for k in range(3):
        for v in (U_, V_):
            mesh.set_level(k, 3600.0 * k, v, r.level(v, k))
    P = ctx.particles(3)
    P.append(lon, lat)
    for before, after, w in ((0, None, 0.0), (0, 1, 0.5), (1, None, 0.0), (1, 2, 0.5)):
        P.schism_sample(mesh, before, after, w, [U_, V_], [True, True])
        P.update_positions(P.env_download(U_), P.env_download(V_), 1800.0)
    d = P.download()
    assert np.hypot(d['lon'] - lon, d['lat'] - lat).min() > 0.02
    order = np.argsort(e.ID)
    assert np.abs(e.lon[order] - d['lon']).max() < 1e-9 and np.abs(e.lat[order] - d['lat']).max() < 1e-9
    P.close()
    mesh.close()


def model_run(g, tag, scheme, config=(), host=False, **kw):
    three_d = tag.startswith('d')
    r = S.golden_reader(g, 'a' if three_d else 'b')      # every variable the reference's reader had: the sea floor acts on z
    o = OceanDrift(loglevel=50, **kw)
    o.add_reader(HostEvaluated(r) if host else r)
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:advection_scheme', scheme)
    o.set_config('drift:stokes_drift', False)
    o.set_config('drift:vertical_advection', False)
    for key, value in config:
        o.set_config(key, value)
    lon, lat, z = g[tag + '_lon'], g[tag + '_lat'], g[tag + '_z']
    o.seed_elements(lon=lon[0], lat=lat[0], z=z[0], time=T0, wind_drift_factor=0.0)
    return o, lon, lat


@pytest.mark.parametrize('tag,scheme', [('c_euler', 'euler'), ('c_rk4', 'runge-kutta4'), ('d_euler', 'euler')])
def test_model_runs_reproduce_the_reference(g, tag, scheme):
    """The reference's OceanDrift with its own SCHISM reader as the only source of the current against this model with the mesh on
    the device: (c) the geographic mesh with depth-averaged currents, 12 steps of 10 minutes, both schemes; (d) the 3-D mesh, Euler, 4
    steps of 30 minutes, elements at fixed depths.  Every sample of the reference's runs keeps the gap between the third and the
    fourth nearest point that the golden stores."""
    case = tag[0]
    assert float(g[case + '_smallest_gap']) > (1e-6 if case == 'c' else 0.05)
    o, lon, lat = model_run(g, tag, scheme, seed=0, rng='numpy')
    assert o._run_lane() == 'call_by_call'
    o.run(time_step=float(g[case + '_dt']), steps=int(g[case + '_steps']))
    e = o.elements
    assert len(e) == lon.shape[1] and (g[tag + '_status'][-1] == 0).all() and (np.asarray(e.status) == 0).all()
    dmax = max(np.abs(e.lon - lon[-1][e.ID]).max(), np.abs(e.lat - lat[-1][e.ID]).max())
    print(tag, 'mesh on the device vs the reference: %.2e deg' % dmax)
    assert dmax < 1e-7
    assert np.hypot(e.lon - lon[0][e.ID], e.lat - lat[0][e.ID]).min() > 0.02


class HostEvaluated(readers.ContinuousReader):
    """The same reader answered on the host at the element positions (DeviceReaderBinding.evaluate_on_host): its mirror."""

    def __init__(self, r):
        self.r, self.proj4, self.name, self.variables = r, r.proj4, r.name + '_host', list(r.variables)
        self.xmin, self.xmax, self.ymin, self.ymax = r.xmin, r.xmax, r.ymin, r.ymax
        self.start_time, self.end_time, self.times = r.start_time, r.end_time, r.times
        super().__init__()

    def get_variables(self, requested_variables, time=None, x=None, y=None, z=None):
        return self.r.get_variables(requested_variables, time, x, y, z)


def test_a_3d_runge_kutta_run_equals_the_host_evaluated_lane(g):
    """No recording of the reference exists for a 3-D runge-kutta4 run (the gap condition would drop most candidates): the device
    lane against the same model whose reader is evaluated on the host.  The two lanes do not share the projection (the device's
    against this package's Python one) nor the rotation angle, so positions are held to 1e-7 deg, not to their bits."""
    res = []
    for host in (False, True):
        o, lon, lat = model_run(g, 'd_euler', 'runge-kutta4', host=host, seed=0, rng='numpy')
        o.run(time_step=600, steps=12)
        e = o.elements
        order = np.argsort(e.ID)
        assert len(order) == lon.shape[1]
        res.append((e.lon[order].copy(), e.lat[order].copy(), np.asarray(e.status)[order].copy()))
    assert np.array_equal(res[0][2], res[1][2])
    dmax = max(np.abs(res[0][0] - res[1][0]).max(), np.abs(res[0][1] - res[1][1]).max())
    print('3-D runge-kutta4: device lane vs host-evaluated lane: %.2e deg' % dmax)
    assert dmax < 1e-7
    assert np.hypot(res[0][0] - lon[0], res[0][1] - lat[0]).min() > 0.02


def test_runs_are_repeatable_also_with_device_noise_on_the_stage_path(g):
    res = []
    for seed in (5, 5, 6):
        o, lon, lat = model_run(g, 'd_euler', 'runge-kutta4', config=[('drift:current_uncertainty', 0.05)], seed=seed, rng='device')
        o.run(time_step=600, steps=3)
        e = o.elements
        order = np.argsort(e.ID)
        assert len(order) == lon.shape[1]
        res.append((e.lon[order].copy(), e.lat[order].copy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])      # the same seed: the same bits
    assert not np.array_equal(res[0][0], res[2][0])                                             # another seed: other draws
    plain = []
    for _ in range(2):
        o, lon, lat = model_run(g, 'd_euler', 'runge-kutta4', seed=0, rng='numpy')
        o.run(time_step=600, steps=3)
        order = np.argsort(o.elements.ID)
        plain.append((o.elements.lon[order].copy(), o.elements.lat[order].copy()))
    assert np.array_equal(plain[0][0], plain[1][0]) and np.array_equal(plain[0][1], plain[1][1])
    assert np.abs(res[0][0] - plain[0][0]).max() > 1e-5                                         # and the noise moved them
