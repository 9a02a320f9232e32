"""GPU: reader operators on the device -- odr_combined_sample (csrc/odr_combine.hip.h) against the reference's own operator classes
(tests/golden/c38_reader_ops.npz, tools/gen_golden_reader_ops.py).

Part 1, every expression over both sets of positions: BIT FOR BIT after the float32 cast, NaN where the reference has nothing.  Sums,
number-ops and blends are single correctly rounded operations on the operands the project's samplers already reproduce bit for bit;
the Gaussian weight goes through the inverse geodesic and exp(), which agree with the reference's to about 1e-16 relative, 2^29
times finer than the float32 the result is cast to -- a different float32 would need the float64 value within that of a rounding
boundary, which none of the golden's 1 284 blended values is.

Element counts 1, 63, 64, 65, 257 and 321 (the wave and workgroup edges; 321 = 256 + 65) are the first n positions of the set that
every grid covers, where a subset keeps the dtype class of the whole.

Part 2, the reference's two runs: every status equal, positions within the project's 1e-6 deg; the measured maximum is printed
(MI355X: Euler 3.3e-9 deg, runge-kutta4 3.7e-9 deg)."""
from datetime import timedelta

import numpy as np
import pytest

import combine_host as H
from opendrift_amd import readers
from opendrift_amd._abi import OdrError
from opendrift_amd.oceandrift import OceanDrift

pytestmark = pytest.mark.gpu
WIND, CURRENT, T0 = H.WIND, H.CURRENT, H.T0


@pytest.fixture(scope='module')
def g():
    return np.load(H.GOLDEN)


def sample(ctx, expr, variables, lon, lat, z, t, first=True, before=None):
    b = readers.DeviceReaderBinding(ctx, expr, variables=variables)
    P = ctx.particles(len(lon))
    P.append(lon, lat, z=z)
    for v, a in (before or {}).items():
        P.env_upload(v, a)
    b.sample_combined(P, variables, [first] * len(variables), t)
    out = {v: P.env_download(v) for v in variables}
    P.close()
    return out, b


@pytest.mark.parametrize('name', H.CASE_NAMES)
@pytest.mark.parametrize('tag', ['in', 'all'])
def test_golden_expressions_bit_for_bit(ctx, g, tag, name):
    expr, variables = H.cases(g)[name]
    t = T0 + timedelta(seconds=int(g['call_seconds']))
    got, b = sample(ctx, expr, variables, g['q_%s_lon' % tag], g['q_%s_lat' % tag], g['q_z'], t)
    for v in variables:
        want = g['r_%s_%s_%s' % (tag, name, v)]
        diff = np.flatnonzero(~((got[v] == want) | (np.isnan(got[v]) & np.isnan(want))))
        print(tag, name, v, 'finite', int(np.isfinite(want).sum()), 'differing', len(diff), got[v][diff[:3]], want[diff[:3]])
        assert H.same_bits(got[v], want), (tag, name, v, len(diff))
    assert ctx.combined_last_kernel_ms() > 0


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 321])
def test_element_counts_at_the_wave_and_workgroup_edges(ctx, g, n):
    t = T0 + timedelta(seconds=int(g['call_seconds']))
    table = H.cases(g)
    for name in ('a+b', '0.9*a', '(a+b)+(c+a)', 'gauss1'):
        expr, variables = table[name]
        variables = [v for v in variables if v in WIND]
        got, _ = sample(ctx, expr, variables, g['q_in_lon'][:n], g['q_in_lat'][:n], g['q_z'][:n], t)
        for v in variables:
            assert H.same_bits(got[v], g['r_in_%s_%s' % (name, v)][:n]), (n, name, v)


@pytest.mark.parametrize('first', [True, False])
def test_merge_rule_partial_coverage_and_nan_cells(ctx, g, first):
    """Slots that hold 7.0, NaN in every third: first -> every finite value of the expression replaces what is there; not first ->
    only the NaN slots are filled.  Where the expression has nothing (b covers part of the box) the slot keeps what it has."""
    expr, variables = H.cases(g)['a+b']
    lon, lat = g['q_all_lon'], g['q_all_lat']
    before = np.full(len(lon), 7.0, np.float32)
    before[::3] = np.nan
    t = T0 + timedelta(seconds=int(g['call_seconds']))
    got, _ = sample(ctx, expr, CURRENT, lon, lat, g['q_z'], t, first=first, before={v: before for v in CURRENT})
    for v in CURRENT:
        want = g['r_all_a+b_' + v]
        have = np.isfinite(want)
        assert 0 < have.sum() < len(lon)
        take = have if first else have & np.isnan(before)
        assert H.same_bits(got[v], np.where(take, want, before)), v


def test_abi_refusals(ctx, g):
    a, b, c, d, ts = H.golden_readers(g)
    from opendrift_amd import _abi as A
    with pytest.raises(ValueError, match='names no source'):
        ctx.combined([(A.COMBINE_SOURCE, 3, (0, 0, 0))])
    with pytest.raises(ValueError, match='more than two saved temporaries'):
        ctx.combined([(A.COMBINE_UNIFORM, 0, (0, 0, 0))] * 4 + [(A.COMBINE_ADD, 0, (0, 0, 0))] * 3)
    bind = readers.DeviceReaderBinding(ctx, a + c, variables=WIND)
    P = ctx.particles(4)
    P.append([4.5] * 4, [60.0] * 4)
    t0 = readers._epoch(T0)
    prog = ctx.combined([(A.COMBINE_SOURCE, bind.leaves[1][1].sid, (0, 0, 0)), (A.COMBINE_UNIFORM, 0, (0, 0, 0)), (A.COMBINE_ADD, 0, (0, 0, 0))])
    with pytest.raises(ValueError, match='uniform leaf 0, 0 were given'):
        P.combined_sample(prog, ['x_wind'], [True], t0)
    with pytest.raises(ValueError, match='given twice'):
        P.combined_sample(prog, ['x_wind', 'x_wind'], [True, True], t0, [[1.0], [1.0]])
    P.combined_sample(prog, ['x_wind'], [True], t0, [[1.5]])
    assert list(P.env_download('x_wind')) == [11.5] * 4      # the constant reader's 10 + the uniform leaf
    # a gridded leaf without a resident level: refused, not sampled
    grid = readers.DeviceReaderBinding(ctx, a, variables=WIND)
    grid.ensure_levels(T0, T0, times=[T0])
    grid.ctx.drop_block(grid.sid, grid.slots.pop(0))
    for k in list(grid.staged):
        grid.ctx.drop_block(grid.sid, grid.staged.pop(k))
    with pytest.raises(OdrError, match='holds no time level'):
        P.combined_sample(ctx.combined([(A.COMBINE_SOURCE, grid.sid, (0, 0, 0))]), ['x_wind'], [True], t0)
    P.close()


def run_readers(g):
    times = [T0 + timedelta(seconds=float(s)) for s in g['seconds']]
    x, y = g['d_x'], g['d_y']
    onshore = readers.ConstantReader({'x_wind': 10.0, 'y_wind': 0.0})
    wind = readers.GridReader(x, y, times, {v: 8 * g['a_' + v] for v in WIND}, name='wind')
    current = readers.GridReader(x, y, times, {v: g['b_' + v] for v in CURRENT}, name='current')
    tide = readers.GridReader(g['a_x'] - 0.3, g['a_y'] - 0.1, times, {v: 0.5 * g['b_' + v] for v in CURRENT}, name='tide')
    background = readers.GridReader(x, y, times, {v: g['a_' + v][:, ::-1, ::-1].copy() for v in WIND + CURRENT}, name='background')
    return onshore, wind, current, tide, background


def model(g, scheme, reader_list, wdf):
    o = OceanDrift(loglevel=50, seed=0, rng='numpy')
    o.add_reader(reader_list)
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:advection_scheme', scheme)
    o.set_config('drift:stokes_drift', False)
    o.seed_elements(lon=g['run_lon'], lat=g['run_lat'], time=T0, wind_drift_factor=wdf)
    return o


def compare(o, g, tag):
    e = o.elements
    lon, lat, status = g['run_%s_lon' % tag], g['run_%s_lat' % tag], g['run_%s_status' % tag]
    assert len(e) == lon.shape[1] and (status[-1] == 0).all() and np.array_equal(np.asarray(e.status), status[-1][e.ID])
    dmax = max(np.abs(e.lon - lon[-1][e.ID]).max(), np.abs(e.lat - lat[-1][e.ID]).max())
    print(tag, 'reader expression on the device vs the reference: %.2e deg' % dmax)
    assert dmax < 1e-6
    assert np.hypot(e.lon - lon[0][e.ID], e.lat - lat[0][e.ID]).min() > 1e-3      # every element moved 1000 x the bound


def test_euler_run_with_constant_plus_gridded_wind_and_a_shared_leaf(g):
    """[onshore + wind, wind, current] of the gallery example: the wind reader is a leaf AND a reader of its own -- one binding,
    one source id, its levels uploaded once; the run crosses the second time level (10 steps of 10 minutes, hourly levels)."""
    onshore, wind, current, _, _ = run_readers(g)
    o = model(g, 'euler', [onshore + wind, wind, current], float(g['run_wdf']))
    assert o._run_lane() == 'call_by_call'
    o.run(time_step=float(g['run_dt']), steps=int(g['run_steps']))
    compare(o, g, 'euler')
    comb, own = o.readers['Combined(constant_reader | wind)'], o.readers['wind']
    shared = [(r, b, mine) for r, b, mine in comb.leaves if r is wind]
    assert len(shared) == 1 and shared[0][1] is own and not shared[0][2]
    assert [mine for _, _, mine in comb.leaves] == [True, False]
    assert 2 in own.slots and len(own.slots) + len(own.staged) <= own.NSLOTS      # the level change reached the shared leaf
    assert len({b.sid for b in (own, o.readers['current'], comb.leaves[0][1])}) == 3


def test_rk4_run_with_tide_plus_background_takes_the_stage_split(g):
    _, _, _, tide, background = run_readers(g)
    o = model(g, 'runge-kutta4', [tide + background, background], 0.0)
    seen = []
    inner = readers.DeviceReaderBinding.sample_combined

    def recording(self, P, variables, first, time):
        seen.append((time, tuple(variables), len(P)))
        return inner(self, P, variables, first, time)
    readers.DeviceReaderBinding.sample_combined = recording
    try:
        o.run(time_step=float(g['run_dt']), steps=int(g['run_steps']))
    finally:
        readers.DeviceReaderBinding.sample_combined = inner
    compare(o, g, 'rk4')
    dt = timedelta(seconds=float(g['run_dt']))
    stage = [t for t, vs, n in seen if set(vs) == set(CURRENT) and T0 <= t <= T0 + dt]
    # the main-loop call at t0, then the stages at t0 + dt / 2 (twice) and t0 + dt
    assert stage.count(T0 + dt / 2) == 2 and T0 + dt in stage and T0 in stage
    owned = [b for _, b, mine in o.readers['Combined(tide | background)'].leaves if mine]
    assert len(owned) == 1 and 2 in owned[0].slots      # the leaf made for the expression followed the run to its third level
