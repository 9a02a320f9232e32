"""GPU: PlastDrift -- the kernels of csrc/odr_plast.hip.h against their host build (bit for bit) and, through it, against the
reference's own values; the decisions of get_environment with a wave reader; the refusal of a negative scale; the device
generator; and the model run end to end against the reference's own PlastDrift (golden c40_plastdrift.npz,
tools/gen_golden_plastdrift.py)."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden
from opendrift_amd import readers
from opendrift_amd.plastdrift import PlastDrift

import plast_host
from test_plast_device_arithmetic import FETCH_OF, environment_case, same_bits, tables
from test_plastdrift_host_api import HS, SX, SY, TABLES

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)


def _particles(ctx, n, inactive=None, tv=None):
    P = ctx.particles(n)
    P.append(np.linspace(3, 4, n), np.full(n, 60.0), z=np.linspace(-5, -1, n), terminal_velocity=tv)
    if inactive is not None and inactive.any():
        P.deactivate(inactive, 5)
    return P


@pytest.mark.parametrize('case', sorted(FETCH_OF))
def test_stokes_from_wind_equals_the_host_build_and_the_reference(ctx, case):
    xw, yw, sx, sy, hs = environment_case(golden('c40_plastdrift.npz'), case)
    t = tables()[FETCH_OF[case]]
    P = _particles(ctx, len(xw))
    P.env_upload('x_wind', xw)
    P.env_upload('y_wind', yw)
    P.stokes_from_wind(t['stokes'], t['hs'])
    got = [P.env_download(v) for v in (SX, SY, HS)]
    P.close()
    for a, b, c in zip(got, plast_host.stokes_from_wind(xw, yw, t['stokes'], t['hs']), (sx, sy, hs)):
        assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.parametrize('n', [1, 65, 3001])
def test_partial_waves_several_workgroups_and_inactive_elements(ctx, n):
    """One lane, one lane past a wave, twelve workgroups with a ragged end; every third element is not active: it keeps its
    Stokes drift, wave height and z, the others get what the host build computes."""
    rng = np.random.default_rng(n)
    t = tables()['25000']
    xw, yw = (rng.uniform(-25, 25, n).astype(np.float32) for _ in range(2))
    K = rng.uniform(0, 0.05, n).astype(np.float32)
    tv = np.exp(rng.uniform(np.log(1e-4), np.log(0.1), n)).astype(np.float32)
    E = rng.standard_exponential(n)
    off = np.arange(n) % 3 == 2 if n > 1 else np.zeros(1, bool)
    P = _particles(ctx, n, off, tv)
    old = {v: rng.uniform(1, 2, n).astype(np.float32) for v in (SX, SY, HS)}
    for v, a in dict(old, x_wind=xw, y_wind=yw, ocean_vertical_diffusivity=K).items():
        P.env_upload(v, a)
    z0 = P.download()['z']
    for which, stokes, hs in (('stokes', t['stokes'], None), ('hs', None, t['hs'])):       # the two groups are launch arguments
        P.stokes_from_wind(stokes, hs)
        want = dict(zip((SX, SY, HS), plast_host.stokes_from_wind(xw, yw, t['stokes'], t['hs'])))
        for v in (SX, SY, HS):
            touched = ~off & ((v != HS) if which == 'stokes' else np.True_)      # after the second launch: all three
            assert same_bits(P.env_download(v), np.where(touched, want[v], old[v])), (which, v)
    P.plast_depth(draws=E)
    z = P.download()['z']
    want, refused = plast_host.depth(K, tv, E)
    assert not refused and same_bits(z, np.where(off, z0, want))
    P.close()


def test_wave_maxima_are_the_plain_maxima_over_the_active_elements(ctx):
    n = 700
    rng = np.random.default_rng(2)
    off = np.arange(n) % 3 == 2
    P = _particles(ctx, n, off)
    assert P.wave_maxima() == (-np.inf, -np.inf, -np.inf)                  # nothing sampled
    a = {SX: -rng.uniform(0.1, 1, n).astype(np.float32), SY: np.zeros(n, np.float32), HS: rng.uniform(0, 3, n).astype(np.float32)}
    a[HS][np.argmax(a[HS])], a[SX][2] = 0, 5.0                             # the largest values sit on elements that are not active
    off[np.argmax(a[HS])] = True
    for v, arr in a.items():
        P.env_upload(v, arr)
    P.deactivate(off, 5)
    assert P.wave_maxima() == tuple(float(a[v][~off].max()) for v in (SX, SY, HS))
    assert P.wave_maxima()[0] < 0 and P.wave_maxima()[1] == 0              # all negative / all zero: what the sum's maximum cannot tell
    r = P.reduce_scalars()                                                 # the sixteen public slots are what they were
    assert r['stokes_sum_max'] == float((a[SX] + a[SY])[~off].max()) and r['hs_max'] == float(a[HS][~off].max())
    P.close()


def test_negative_scale_raises_and_leaves_every_z_unchanged(ctx):
    n = 300
    tv = np.full(n, 0.01, np.float32)
    tv[217] = -0.01                                    # one sinking element
    P = _particles(ctx, n, tv=tv)
    P.env_upload('ocean_vertical_diffusivity', np.full(n, 0.02, np.float32))
    z0 = P.download()['z']
    for kw in (dict(draws=np.ones(n)), dict(step=3)):
        with pytest.raises(ValueError, match='scale < 0'):
            P.plast_depth(**kw)
        assert same_bits(P.download()['z'], z0)
    off = np.zeros(n, bool)
    off[217] = True
    P.deactivate(off, 5)                               # ... which no longer counts once it is not active
    P.plast_depth(draws=np.ones(n))
    z = P.download()['z']
    assert z[217] == z0[217] and (np.delete(z, 217) == -(np.float64(np.float32(0.02) / np.float32(0.01)))).all()
    P.close()


def test_device_generator_is_reproducible_and_exponential(ctx):
    n = 100000
    out = []
    for step in (4, 4, 5):
        P = _particles(ctx, n, tv=np.full(n, 0.5, np.float32))
        P.env_upload('ocean_vertical_diffusivity', np.full(n, 0.5, np.float32))      # scale 1
        P.plast_depth(step=step)
        out.append(P.download()['z'])
        P.close()
    assert same_bits(out[0], out[1]) and not np.array_equal(out[0], out[2])          # same seed and step: same bits
    E = -out[0]
    print('mean %.5f, variance %.5f, largest %.2f' % (E.mean(), E.var(), E.max()))
    assert (E >= 0).all() and np.isfinite(E).all()
    assert abs(E.mean() - 1) < 5 / np.sqrt(n)          # the mean of n standard exponentials has the standard deviation 1 / sqrt(n)


def _reader(g, waves=None):
    times = [T0 + timedelta(seconds=900. * k) for k in range(12)]
    one = np.ones((len(times), 1, 1), np.float32)
    fields = {k[2:]: g[k] for k in g.files if k.startswith('g_') and k not in ('g_x', 'g_y')}
    out = [readers.GridReader(g['g_x'], g['g_y'], times, {k: one * v for k, v in fields.items()})]
    if waves:
        out.append(readers.GridReader(g['g_x'], g['g_y'], times, {k: one * v for k, v in waves.items()}))
    return out


def _model(g, case, waves=None, **kw):
    o = PlastDrift(loglevel=50, seed=0, rng='numpy', stokes_tables=TABLES, **kw)
    o.add_reader(_reader(g, waves))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('seed:ocean_only', False)
    o.seed_elements(lon=g[case + '_lon0'], lat=g[case + '_lat0'], z=0.0, time=T0, terminal_velocity=g[case + '_tv'])
    return o


@pytest.mark.parametrize('case,stokes_replaced,hs_replaced', [('c1', False, True), ('c2', True, False), ('c3', False, True),
                                                              ('c4', True, False)])
def test_decisions_of_get_environment_with_a_wave_reader(case, stokes_replaced, hs_replaced):
    """c1 a reader's Stokes drift is left alone; c2 one that is 0 everywhere is replaced; c3 x all negative with y zero is not;
    c4 a wave height above 0 is kept while the absent Stokes drift is derived.  The environment behind one step, by element ID,
    bit for bit the reference's where it was derived from the wind, to the interpolation's float32 round-off where it was sampled."""
    g = golden('c40_plastdrift.npz')
    waves = {v: g['%s_w_%s' % (case, s)] for v, s in ((SX, 'sx'), (SY, 'sy'), (HS, 'hs')) if '%s_w_%s' % (case, s) in g.files}
    o = _model(g, case, waves)
    np.random.seed(40)
    o.run(time_step=900, steps=1)
    e = o.environment
    assert np.array_equal(o.elements.ID, np.arange(len(g[case + '_lon0'])))
    for v, s, replaced in ((SX, 'sx', stokes_replaced), (SY, 'sy', stokes_replaced), (HS, 'hs', hs_replaced)):
        got, want = np.asarray(getattr(e, v)), g['%s_%s' % (case, s)][0]
        if replaced:
            assert same_bits(got, want), v
        else:
            assert np.abs(got - want).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max()), v      # 4 ulp of the largest


@pytest.mark.parametrize('case', ['a', 'd'])
def test_run_numpy_rng_reproduces_the_reference(case):
    """rng='numpy': np.random.standard_exponential(n) is drawn once per step, as the reference's np.random.exponential consumes
    the stream.  Every status equal; positions within 1e-6 degrees; z bit for bit in float64 -- the reference's elements.z is the
    float64 array update_particle_depth assigned from the first step on, and nothing rounds it afterwards in these cases (no sea
    floor is reached).  Compared: the state behind run(), that is behind the interact_with_coastline(final=True) that follows the
    loop there and here; the test below has the steps before the last."""
    g = golden('c40_plastdrift.npz')
    o = _model(g, case)
    steps = g[case + '_lon'].shape[0]
    np.random.seed(40)
    o.run(time_step=900, steps=steps)
    assert o.steps_calculation == steps and o._run_lane() == 'call_by_call'
    n = len(g[case + '_lon0'])
    lon, lat, z, status = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1)
    for d in (o.elements, o.elements_deactivated):
        lon[d.ID], lat[d.ID], z[d.ID], status[d.ID] = d.lon, d.lat, d.z, d.status
    dlon, dlat = np.abs(lon - g[case + '_end_lon']).max(), np.abs(lat - g[case + '_end_lat']).max()
    print('largest differences: lon %.3g lat %.3g deg; z differs in %d of %d elements' % (dlon, dlat, (z != g[case + '_end_z']).sum(), n))
    assert np.array_equal(status, g[case + '_end_status'])
    assert dlon < 1e-6 and dlat < 1e-6
    assert same_bits(z, g[case + '_end_z'])
    if case == 'd':      # elements came back from the land: their positions are the previous ones, and they moved at all
        assert (np.abs(lon - g['d_lon0']) > 1e-4).any()
    # the last step's environment: derived from winds sampled at positions that agree to 1e-6 degrees (a wind gradient of 44 m/s
    # over 6 degrees: 7e-6 m/s, times a factor of 0.02 / a slope of 0.11 m per m/s) plus one float32 rounding of values below 4
    e, ids = o.environment, np.asarray(o.elements.ID)
    for v, s in ((SX, 'sx'), (SY, 'sy'), (HS, 'hs')):
        assert np.abs(np.asarray(getattr(e, v)) - g['%s_%s' % (case, s)][-1][ids]).max() < 2e-6, v


@pytest.mark.parametrize('case', ['a', 'd'])
def test_every_step_of_the_run_reproduces_the_reference(case):
    """The state behind each of the steps 1 .. 7 (the run test above has the last), from a run of that many steps -- the result
    history is float32 and cannot show bits.  z bit for bit in float64 and every status equal behind every step from the first;
    in case (a), where no element reaches the land and the closing coastline interaction of run() moves nothing, the positions
    within 1e-6 degrees too.  In case (d) that interaction moves elements back, so its positions are compared behind the whole
    run only."""
    g = golden('c40_plastdrift.npz')
    n, steps = len(g[case + '_lon0']), g[case + '_lon'].shape[0]
    if case == 'a':
        assert np.array_equal(g['a_end_lon'], g['a_lon'][-1]) and np.array_equal(g['a_end_lat'], g['a_lat'][-1])
    worst = 0.0
    for k in range(1, steps):
        o = _model(g, case)
        np.random.seed(40)
        o.run(time_step=900, steps=k)
        lon, lat, z, status = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1)
        for d in (o.elements, o.elements_deactivated):
            lon[d.ID], lat[d.ID], z[d.ID], status[d.ID] = d.lon, d.lat, d.z, d.status
        assert np.array_equal(status, g[case + '_status'][k - 1]), k
        assert same_bits(z, g[case + '_z'][k - 1]), k
        if case == 'a':
            worst = max(worst, np.abs(lon - g['a_lon'][k - 1]).max(), np.abs(lat - g['a_lat'][k - 1]).max())
        o._release_device()
    print('largest position difference behind the steps 1 .. %d: %.3g deg' % (steps - 1, worst))
    assert worst < 1e-6


def test_run_with_the_device_generator_and_the_random_walk():
    """The defaults a user gets: rng='device'.  Reproducible; the depths are exponential about K / w; 'randomwalk' runs the stock
    mixing instead and leaves different depths."""
    g = golden('c40_plastdrift.npz')

    def run(model=None):
        o = PlastDrift(loglevel=50, seed=5, stokes_tables=TABLES)
        o.add_reader(_reader(g))
        if model:
            o.set_config('vertical_mixing:mixingmodel', model)
        o.seed_elements(lon=g['a_lon0'], lat=g['a_lat0'], time=T0, terminal_velocity=0.01)
        o.run(time_step=900, steps=3)
        return o.elements.z, o.elements.lon
    (za, la), (zb, lb), (zr, lr) = run(), run(), run('randomwalk')
    assert same_bits(za, zb) and same_bits(la, lb)
    assert (za <= 0).all() and 1.0 < -za.mean() < 3.5            # scale = 0.02 / 0.01 = 2 m
    assert not np.array_equal(za, zr) and (zr <= 0).all()
