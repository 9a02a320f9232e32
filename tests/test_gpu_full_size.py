"""GPU: BASELINE.json's FULL sizes (C2 1 M, C3 10 M, C4 6.25 M per GPU, C5 10 M elements) through properties that do not
need the CPU oracle to finish a full-size run:

  * independence / layout invariance: the elements with every k-th ID, stepped on their own in a second particle set,
    end bit-identical to the same IDs inside the full-size run (device Philox numbers are counter-based on the ID; the
    spatial re-sort and the in-place compaction of the full run only permute memory) -- this is also what makes the
    result independent of how the elements are sharded over GPUs;
  * that sub-sample against the CPU oracle on the deterministic part of the step (RK4 advection);
  * time reversal: RK4 forward then backward returns to the start (analytic double gyre, 1 M elements);
  * conservation and invariants: active + deactivated = seeded, IDs unique, z within [sea floor, 0], no NaN,
    stranded elements sit on land cells, the re-sorted layout is ordered by grid cell.
"""
import numpy as np
import pytest

import bench
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu
U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'


def _state_by_id(P, ids=None):
    d = P.download()
    o = np.argsort(d['ID'], kind='stable')
    out = {k: v[o] for k, v in d.items()}
    if ids is not None:
        sel = np.searchsorted(out['ID'], ids)
        ok = (sel < len(out['ID'])) & (out['ID'][np.minimum(sel, len(out['ID']) - 1)] == ids)
        return {k: v[sel[ok]] for k, v in out.items()}, ok
    return out, None


def _leeway_props(P, n, ids):
    r5 = np.random.default_rng(7)
    full = 10_000_000
    ori = (np.arange(full) % 2).astype(np.float32)
    vals = [np.full(full, 0.96), np.where(ori == 0, 0.54, -0.54), np.zeros(full), np.zeros(full),
            np.abs(r5.standard_normal(full)) * 12.0, r5.standard_normal(full) * 9.4, np.full(full, 0.04), ori, np.zeros(full)]
    for slot, v in enumerate(vals):
        P.set_property(slot, v[ids].astype(np.float32))


_SIZES = [('c3', 10_000_000, 3, 499), ('c4', 6_250_000, 3, 311), ('c5', 10_000_000, 3, 499), ('c2', 1_000_000, 20, 97)]
# EXACT under the ids the cases always had; FAST (bench.py's --stage-math default) for the Runge-Kutta workloads.  C5 has no FAST
# case: the Leeway step is Euler, and its launch (odr_env_coast_leeway -> k_step_leeway, opendrift_amd/csrc/odrift.hip:1678-1682)
# never reads the context's stage arithmetic -- stage_math is read by the Runge-Kutta launches only (odr_step.hip:63).
_CASES = [c + ('exact',) for c in _SIZES] + [c + ('fast',) for c in _SIZES if c[0] != 'c5']


@pytest.mark.parametrize('name,n,steps,stride,stage_math', _CASES,
                         ids=['%s-%d-%d-%d' % c[:4] + ('' if c[4] == 'exact' else '-fast') for c in _CASES])
def test_subsample_is_bit_identical_to_the_full_size_run(name, n, steps, stride, stage_math):
    ctx = Context(0, seed=0)
    ctx.set_stage_math(stage_math)
    fields = bench.make_fields(name)
    wl = bench.Workload(name, ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles(name, fields, n, np.random.default_rng(1))
    ids = np.arange(n, dtype=np.int32)
    sub = ids[::stride]
    full, part = ctx.particles(n), ctx.particles(len(sub))
    full.append(lon, lat, z=z, id=ids)
    part.append(lon[sub], lat[sub], z=z[sub], id=sub)
    if name == 'c5':
        _leeway_props(full, n, ids)
        _leeway_props(part, len(sub), sub)
    for k in range(steps):
        wl.step(full, k)      # k = 0 re-sorts the full set by grid cell
        wl.step(part, k)
    a, ok = _state_by_id(full, sub)
    b, _ = _state_by_id(part)
    if name in ('c4', 'c5'):   # stranded elements left the active sets: the same ones in both
        assert np.array_equal(sub[ok], b["ID"]) and (~ok).sum() < len(sub) // 2
        da, db = full.download_deactivated(), part.download_deactivated()
        oa, ob = np.argsort(da['ID']), np.argsort(db['ID'])
        sel = np.isin(da['ID'][oa], db['ID'])
        for key in ('ID', 'lon', 'lat', 'status'):
            assert np.array_equal(da[key][oa][sel], db[key][ob]), key
        assert len(da['ID']) + len(full) == n and len(np.unique(np.concatenate([da['ID'], full.download()['ID']]))) == n
    else:
        assert ok.all()
    for key in ('lon', 'lat', 'z', 'status', 'moving'):
        assert np.array_equal(a[key], b[key]), key
    assert np.isfinite(a['lon']).all() and np.isfinite(a['lat']).all() and np.isfinite(a['z']).all()
    moved = np.abs(a['lon'] - lon[a['ID']]) + np.abs(a['lat'] - lat[a['ID']])
    assert (moved > 0).mean() > 0.9
    if name == 'c3':           # vertical invariants on ALL elements: below the surface, above the sea floor
        d = full.download()
        depth = full.env_download('sea_floor_depth_below_sea_level')
        assert (d['z'] <= 0).all() and (d['z'] >= -depth.astype(np.float64) - 1e-9).all()
        assert len(np.unique(d['ID'])) == n
    full.close(); part.close(); ctx.close()


def test_c3_rk4_subsample_against_the_cpu_oracle():
    """10 M elements, one fused RK4 launch on the full-size block; every 5000th element against the C oracle."""
    from oracle import oracle as orc
    name, n = 'c3', 10_000_000
    ctx = Context(0, seed=0)
    fields = bench.make_fields(name)
    wl = bench.Workload(name, ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles(name, fields, n, np.random.default_rng(2))
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    P.sort_by_cell(wl.sid)
    t = 1234.0
    P.env_coast_advect(wl.vars, t, 'runge-kutta4', wl.dt, coastline='none', store_previous=True, count=False)
    sub = np.arange(0, n, 5000)
    got, ok = _state_by_id(P, sub.astype(np.int32))
    assert ok.all()
    g = fields['g']
    wb = orc.WorldBuilder()
    levels = [(float(g['t'][k]), {orc.VAR[v]: g[v][k] for v in fields['names']}) for k in range(3)]
    wb.add_grid(orc.make_proj(), g['x'], g['y'], levels, z=fields['z'])
    for v in fields['names']:
        wb.set_fallback(orc.VAR[v], {'land_binary_mask': np.nan, 'sea_floor_depth_below_sea_level': 10000.0}.get(v, 0.0))
    w = wb.finish()
    lo, la, zz = lon[sub].copy(), lat[sub].copy(), z[sub].copy()
    u, v = orc.get_environment(w, [orc.VAR[U], orc.VAR[V]], lo, la, zz, t)
    m = len(sub)
    orc.advect_ocean_current(w, 2, lo, la, zz, np.ones(m, np.int32), np.ones(m, np.float32), u, v, t, wl.dt)
    assert np.abs(got['lon'] - lo).max() < 1e-10 and np.abs(got['lat'] - la).max() < 1e-10
    P.close(); ctx.close()


# FAST: its per-step bound of 3e-9 deg is that of C3's 600 s step; the stage positions' direct move errs with the square of the
# displacement, so C4's 900 s step takes 3e-9 * (900 / 600)^2 = 6.75e-9 deg
@pytest.mark.parametrize('stage_math,bound', [('exact', 2e-9), ('fast', 3e-9 * (900.0 / 600.0) ** 2)])
def test_c4_rk4_subsample_against_the_cpu_oracle(stage_math, bound):
    """6.25 M elements, one fused RK4 launch on the full-size polar-stereographic block; every 3001st element against the C
    oracle (exact arithmetic) on the world of tests/replay.py's C4 scenario.  EXACT at the polar-stereographic tolerance of the
    C4 golden parity (test_gpu_parity.py::test_c4_golden_device, 2e-9 deg): the device's and the oracle's projections agree to
    float64 round-off, not bit for bit, and a stage sample then rounds a float32 velocity the other way now and then (one
    float32 ulp of 0.5 m/s over 900 s is 5e-10 deg) -- all but a few elements in a thousand agree to 1e-10 deg.  FAST at its
    per-step bound (test_gpu_stage_math.py) scaled to the 900 s step."""
    import replay
    from oracle import oracle as orc
    name, n = 'c4', 6_250_000
    ctx = Context(0, seed=0)
    ctx.set_stage_math(stage_math)
    fields = bench.make_fields(name)
    wl = bench.Workload(name, ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles(name, fields, n, np.random.default_rng(5))
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    P.sort_by_cell(wl.sid)
    t = 1234.0
    P.env_coast_advect(wl.vars, t, 'runge-kutta4', wl.dt, coastline='none', store_previous=True, count=False)
    sub = np.arange(0, n, 3001)
    got, ok = _state_by_id(P, sub.astype(np.int32))
    assert ok.all()
    P.close(); ctx.close()
    g = fields['g']
    scen = replay.scenario_c4({'g_' + k: g[k] for k in ['x', 'y', 't'] + fields['names']})
    w = scen.oracle_world()          # (the world points into arrays the scenario keeps: `scen` must stay alive)
    lo, la, zz = lon[sub].copy(), lat[sub].copy(), z[sub].copy()
    u, v = orc.get_environment(w, [orc.VAR[U], orc.VAR[V]], lo, la, zz, t)
    m = len(sub)
    orc.advect_ocean_current(w, 2, lo, la, zz, np.ones(m, np.int32), np.ones(m, np.float32), u, v, t, wl.dt)
    err = np.maximum(np.abs(got['lon'] - lo), np.abs(got['lat'] - la))
    moved = np.hypot(got['lon'] - lon[sub], got['lat'] - lat[sub])
    print('C4 6.25 M %s launch vs oracle: %.2e deg worst, %d of %d elements above 1e-10 deg' %
          (stage_math.upper(), err.max(), (err > 1e-10).sum(), m))
    assert (moved > 0).mean() > 0.9
    assert err.max() < bound
    if stage_math == 'exact':
        assert (err > 1e-10).sum() <= m // 200


def test_c2_time_reversal_one_million():
    """RK4 on the analytic double gyre, 1 M elements: 50 steps forward, 50 steps backward with the same |dt|.  The
    reference's scheme with float32 velocities in a 2 m x 1 m strongly sheared domain is not reversible to round-off
    (its own round trip: 5e-7 deg maximum, 1.5e-7 median, Euler 3e-6 -- measured with the CPU oracle); the device
    must show the same round trip, and every 500th element must equal the oracle's round trip."""
    from oracle import oracle as orc
    n = 1_000_000
    ctx = Context(0, seed=0)
    wl = bench.Workload('c2', ctx, None, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles('c2', None, n, np.random.default_rng(3))
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    steps, dt = 50, wl.dt
    sub = np.arange(0, n, 500)
    wb = orc.WorldBuilder()
    wb.add_double_gyre(A=0.1, epsilon=0.25, omega=0.628, t0=0.0)
    w = wb.finish()
    lo, la, zz = lon[sub].copy(), lat[sub].copy(), z[sub].copy()
    mv, cdf = np.ones(len(sub), np.int32), np.ones(len(sub), np.float32)
    for k in range(steps):
        P.env_sample([U, V], k * dt)
        P.advect('runge-kutta4', k * dt, dt)
        u, v = orc.get_environment(w, [0, 1], lo, la, zz, k * dt)
        orc.advect_ocean_current(w, 2, lo, la, zz, mv, cdf, u, v, k * dt, dt)
    mid = P.download()
    for k in range(steps, 0, -1):
        P.env_sample([U, V], k * dt)
        P.advect('runge-kutta4', k * dt, -dt)
        u, v = orc.get_environment(w, [0, 1], lo, la, zz, k * dt)
        orc.advect_ocean_current(w, 2, lo, la, zz, mv, cdf, u, v, k * dt, -dt)
    end = P.download()
    disp = np.hypot(mid['lon'] - lon, mid['lat'] - lat)
    err = np.hypot(end['lon'] - lon, end['lat'] - lat)
    assert np.median(disp) > 2e-6 and err.max() < 1e-6 and np.median(err) < 3e-7, (np.median(disp), err.max(), np.median(err))
    assert np.abs(end['lon'][sub] - lo).max() < 1e-9 and np.abs(end['lat'][sub] - la).max() < 1e-9
    P.close(); ctx.close()


def test_c4_resorted_layout_is_ordered_and_stranded_elements_are_on_land():
    name, n = 'c4', 6_250_000
    ctx = Context(0, seed=0)
    fields = bench.make_fields(name)
    wl = bench.Workload(name, ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles(name, fields, n, np.random.default_rng(4))
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    for k in range(4):
        wl.step(P, k)
    dead = P.download_deactivated()
    assert len(dead['ID']) > 1000 and (dead['status'] == 1).all() and len(dead['ID']) + len(P) == n
    # the stranded elements sit on land cells of the block (nearest-node landmask, interpolators.py:27-40)
    D = ctx.particles(len(dead['ID']))
    D.append(dead['lon'], dead['lat'])
    land = D.env_sample(['land_binary_mask'], wl.time_of(3), download=True)['land_binary_mask']
    assert (land == 1).all()
    # after a re-sort the memory order follows the grid cells: positions of neighbours in memory are close
    P.sort_by_cell(wl.sid)
    d = P.download()
    x, y = ctx.lonlat2xy(wl.sid, d['lon'], d['lat'])
    g = fields['g']
    cx, cy = (x - g['x'][0]) / (g['x'][1] - g['x'][0]), (y - g['y'][0]) / (g['y'][1] - g['y'][0])
    jump = np.hypot(np.diff(cx), np.diff(cy))
    assert np.median(jump) < 2.0, np.median(jump)          # random order: ~1000 cells
    D.close(); P.close(); ctx.close()
