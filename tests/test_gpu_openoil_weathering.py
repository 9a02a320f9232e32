"""GPU: OpenOil's NOAA oil weathering -- the launches of csrc/odr_weather.hip against the host build of the same header and against
the reference (golden C39, tools/gen_golden_openoil_weathering.py), the sizes at which indexing can go wrong, the state following
the element ID through compaction and the re-sort, the budget, and the model run.

Device against host build: density and fraction_evaporated (+ - * / only) bit for bit; what lies behind exp / pow within
weather_host.BOUNDS['all'], the distances measured against the golden and doubled (the device's expf / powf are a third
implementation next to libm's and NumPy's: the same float32 ulp on some arguments)."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from opendrift_amd import _abi, readers
from opendrift_amd._abi import OdrError

import weather_host as W

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
U, XW, YW, TEMP, HS, TP = ('x_sea_water_velocity', 'x_wind', 'y_wind', 'sea_water_temperature', 'sea_surface_wave_significant_height',
                           'sea_surface_wave_period_at_variance_spectral_density_maximum')
ENV_NAMES = dict(xwind=XW, ywind=YW, temp=TEMP, hs=HS, tp=TP)
B = W.BOUNDS['all']


@pytest.fixture(scope='module')
def G():
    return W.Golden()


def _particles(ctx, ids, z, age, env, lon=None, lat=None):
    """A particle set of the elements `ids` (ascending) with per-element ages: the oldest are appended first and aged."""
    n = len(ids)
    P = ctx.particles(n)
    age = np.asarray(age, np.float64)
    lon = np.linspace(4, 5, n) if lon is None else lon
    lat = np.full(n, 60.0) if lat is None else lat
    levels = np.unique(age)[::-1]
    for k, a in enumerate(levels):
        m = age == a
        P.append(lon[m], lat[m], z=np.asarray(z, np.float64)[m], id=np.asarray(ids)[m])
        P.increase_age(a - (levels[k + 1] if k + 1 < len(levels) else 0.0))
    order = P.ids()
    pos = {int(e): k for k, e in enumerate(ids)}
    sel = np.array([pos[int(e)] for e in order])
    assert np.array_equal(P.download_f32('age_seconds'), age[sel].astype(np.float32))
    for k in (_abi.OIL_PROPERTIES.index('density'), _abi.OIL_PROPERTIES.index('viscosity')):
        P.set_property(k, np.zeros(n, np.float32))
    _upload_env(P, env, sel)
    return P, sel


def _upload_env(P, env, sel):
    for k, v in env.items():
        if k in ('hs', 'tp') and not np.any(v):
            continue        # not sampled: the launch takes a missing array as zeros
        P.env_upload(ENV_NAMES[k], np.asarray(v, np.float32)[sel])


def _table(P, oil, rho_w, n_total, state, mc):
    """state: {name: [n_total]} (NaN where there is no element), mc [n_total, ncomp]"""
    P.weathering_setup(oil, n_total, rho_w)
    for k in W.REC:
        P.weathering_set(k, np.nan_to_num(state[k]))
    P.weathering_set('mass_components', mc)


def _compare(P, ids, host, host_mc, what, ref=None, ref_mc=None, skip=()):
    worst = {}
    for k in [q for q in W.STATE if q not in skip]:
        got = P.weathering_get(k)[ids]
        for tag, exp in (('host', host[k]), ('reference', None if ref is None else ref[k][ids])):
            if exp is None:
                continue
            u = W.ulps(got, exp)
            worst[(tag, k)] = float(u.max()) if u.size else 0.
            assert (u <= B[k]).all(), (what, tag, k, u.max())
    got = P.weathering_get('mass_components')[ids]
    for tag, exp in (('host', host_mc), ('reference', None if ref_mc is None else ref_mc[ids])):
        if exp is not None:
            u = W.ulps(got, exp)
            worst[(tag, 'mass_components')] = float(u.max()) if u.size else 0.
            assert (u <= B['mass_components']).all(), (what, tag, u.max())
    return worst


# ------------------------------------------------------------------------------------------------ the launches against C39
@pytest.mark.parametrize('case', W.Golden.CASES)
def test_replay_of_the_reference_steps(ctx, G, case):
    """Every step of C39 from the reference's state in front of it, and every process from the state in front of that process."""
    oil, rho_w, dt, procs = G.oil(case), G.rho_w(case), G.dt(case), G.processes(case)
    n_total = len(G.g(case, 'lon'))
    worst = {}
    for s in range(G.steps(case)):
        ids, env, z, age = G.inputs(case, s)
        P, sel = _particles(ctx, ids, z, age, env)
        replays = [(None, ['properties'] + procs, 'b')]
        before = None
        for pr in ['properties'] + procs:
            replays.append((before, [pr], G._stage_prefix(pr)))
            before = G._stage_prefix(pr)
        for before, which, behind in replays:
            front, mc0 = G.state(case, s, before), G.mc(case, s, before)
            _table(P, oil, rho_w, n_total, front, mc0)
            P.oil_weather(dt, which)
            host, host_mc, red, tk = W.step(oil, rho_w, which, dt, env, z, age, {k: v[ids] for k, v in front.items()}, mc0[ids])
            w = _compare(P, ids, host, host_mc, (case, s, which), G.state(case, s, behind), G.mc(case, s, behind))
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0), v)
            dev_red = P.weathering_get('reduction')
            for k in ('n_surface', 'min_age_surface', 'hs_max', 'tp_max', 'tp_min', 'tp_count'):
                assert dev_red[k] == red[k], (case, s, k)
            if oil.get('max_water_fraction'):
                assert dev_red['min_ydiff'] == red['min_ydiff']
            # rows of elements that are not there stay as they are; the emulsion's properties reach the mixing kernels as float32
            absent = np.setdiff1d(np.arange(n_total), ids)
            assert np.array_equal(P.weathering_get('mass_components')[absent], mc0[absent])
            for k, name in ((1, 'density'), (2, 'viscosity')):
                assert np.array_equal(P.get_property(k), P.weathering_get(name)[ids][sel].astype(np.float32))
        P.close()
    print(case, {k: v for k, v in sorted(worst.items()) if v})


# ------------------------------------------------------------------------------------------------ sizes
def _synthetic(n, ncomp, seed, submerged=False):
    rng = np.random.default_rng(seed)
    bp = np.linspace(350., 900., ncomp) if ncomp > 1 else np.array([480.])
    mf = rng.uniform(0.5, 1.5, ncomp)
    oil = dict(mass_fraction=(mf / mf.sum()).tolist(), boiling_point=bp.tolist(), molecular_weight=(0.4 * bp - 60).tolist(), density=870.,
               density_ref_temp=288.15, density_k=0.7, viscosity=2e-5, viscosity_ref_temp=288.15, viscosity_B=2500., bullwinkle_fraction=0.05,
               bullwinkle_time=None, emulsion_water_fraction_max=0.7, oil_water_interfacial_tension=0.025,
               max_water_fraction={'temperatures': [5., 15.], 'max_water_fraction': [0.5, 0.65]})
    n_total = n + 3                           # three elements are released later: they have rows and are not in the set
    ids = np.sort(rng.permutation(n_total)[:n])
    ws = rng.uniform(0, 16, n)
    ws[::7], ws[3::7] = 0.0, 10.0             # calm, and exactly at the change of form of the mass transport coefficient
    env = dict(xwind=ws.astype(np.float32), ywind=np.zeros(n, np.float32), temp=rng.uniform(1, 22, n).astype(np.float32),
               hs=np.zeros(n, np.float32), tp=np.zeros(n, np.float32))
    z = np.where(rng.uniform(size=n) < (1.0 if submerged else 0.3), -rng.uniform(0.1, 30, n), 0.0)
    age = 900. * rng.integers(1, 4, n)
    m0 = rng.uniform(5, 15, n_total)
    evap = rng.uniform(0, 0.3, n_total) * m0
    mc = np.asarray(oil['mass_fraction']) * (m0 - evap)[:, None]
    state = {k: np.zeros(n_total) for k in W.REC}
    state.update(mass_oil=mc.sum(axis=1), mass_evaporated=evap, interfacial_area=rng.uniform(0, 2e6, n_total),
                 oil_film_thickness=np.full(n_total, 0.001), biodegradation_half_time_droplet=np.full(n_total, 1.),
                 biodegradation_half_time_slick=np.full(n_total, 3.), mass_dispersed=rng.uniform(0, 1, n_total))
    state['water_fraction'] = state['interfacial_area'] * 1e-5 / (6 + state['interfacial_area'] * 1e-5)
    return oil, n_total, ids, env, z, age, state, mc


@pytest.mark.parametrize('ncomp', [1, 2, 7, 32])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1025])
def test_sizes(ctx, n, ncomp):
    rho_w = 1026.95
    for submerged, bio in ((False, 'half_time'), (True, 'Adcroft')):
        oil, n_total, ids, env, z, age, state, mc = _synthetic(n, ncomp, 1000 * n + ncomp, submerged)
        which = ['properties', 'evaporation', 'emulsification', 'dispersion', bio]
        P, sel = _particles(ctx, ids, z, age, env)
        _table(P, oil, rho_w, n_total, state, mc)
        P.oil_weather(900., which)
        host, host_mc, red, _ = W.step(oil, rho_w, which, 900., env, z, age, {k: v[ids] for k, v in state.items()}, mc[ids])
        _compare(P, ids, host, host_mc, (n, ncomp, submerged), skip=('mass_biodegraded',) if bio == 'Adcroft' else ())
        if bio == 'Adcroft':
            # Adcroft's fraction is the float32 1 - expf(-age0 / tau), about 1e-4 here: the device's expf and libm's may lie one float32
            # ulp of a value below 1 apart (2**-24; the subtraction is exact), and mass_biodegraded = mass_oil * fraction carries it with
            # a weight that grows with 1 / fraction -- the ulp distance of the golden's 2 .. 20 degC does not transfer to 1 .. 22 degC.
            # Two such ulps of the fraction, times the oil mass in front of the process:
            d = np.abs(P.weathering_get('mass_biodegraded')[ids] - host['mass_biodegraded'])
            assert (d <= 2 * 2.0**-24 * state['mass_oil'][ids]).all(), d.max()
        absent = np.setdiff1d(np.arange(n_total), ids)
        for k in W.REC:
            assert np.array_equal(P.weathering_get(k)[absent], state[k][absent]), k
        assert np.array_equal(P.weathering_get('mass_components')[absent], mc[absent])
        dev_red = P.weathering_get('reduction')
        assert dev_red['n_surface'] == (z == 0).sum() == red['n_surface'] and dev_red['min_ydiff'] == red['min_ydiff']
        if submerged:      # no evaporation
            assert np.array_equal(P.weathering_get('mass_evaporated'), state['mass_evaporated'])
        else:
            got, had, windy = P.weathering_get('mass_evaporated')[ids], state['mass_evaporated'][ids], (env['xwind'] > 0) & (z == 0)
            assert (got[windy] > had[windy]).all() and np.array_equal(got[~windy], had[~windy])      # (a calm has no mass transport)
        P.close()


@pytest.mark.parametrize('n', [65, 1025])
def test_sampled_peak_period_with_zeros_and_a_one_entry_max_water_fraction(ctx, n):
    """wave_period with a peak-period reader (physics_methods.py:918-943): a sampled period stands, a zero is replaced by the mean
    of the positive ones (the tp_sum / tp_count fold of the reduction); and the one-entry form of max_water_fraction on the device.
    The periods are multiples of 0.25 s, so their float64 sum is exact in every fold order and the mean is the same float32 on the
    device, in the host build and in NumPy."""
    rho_w, ncomp = 1026.95, 7
    oil, n_total, ids, env, z, age, state, mc = _synthetic(n, ncomp, 31 * n)
    oil['max_water_fraction'] = {'temperatures': [5.], 'max_water_fraction': [0.4]}
    rng = np.random.default_rng(n)
    env['tp'] = rng.choice(np.array([0., 0., 4., 5.5, 7.25, 9.], np.float32), n)
    env['tp'][:3] = (0., 4., 9.)[:min(3, n)]
    which = ['properties', 'evaporation', 'emulsification', 'dispersion', 'half_time']
    P, sel = _particles(ctx, ids, z, age, env)
    _table(P, oil, rho_w, n_total, state, mc)
    P.oil_weather(900., which)
    host, host_mc, red, _ = W.step(oil, rho_w, which, 900., env, z, age, {k: v[ids] for k, v in state.items()}, mc[ids])
    dev_red = P.weathering_get('reduction')
    pos = env['tp'][env['tp'] > 0].astype(np.float64)
    assert dev_red['tp_max'] == 9. and dev_red['tp_min'] == 0. and dev_red['tp_sum'] == pos.sum() and dev_red['tp_count'] == pos.size
    for k in _abi.WEATHER_REDUCTION:
        assert dev_red[k] == red[k], k
    assert dev_red['hs_max'] == 0
    _compare(P, ids, host, host_mc, ('tp', n))      # (the one-entry max_water_fraction: the device against the host build)
    # the period reaches the dispersion: with every period replaced by the mean, only the elements that had one of their own change
    mean = np.float32(pos.sum() / pos.size)
    P2, _ = _particles(ctx, ids, z, age, dict(env, tp=np.where(env['tp'] > 0, env['tp'], mean).astype(np.float32)))
    _table(P2, oil, rho_w, n_total, state, mc)
    P2.oil_weather(900., which)
    assert P2.weathering_get('reduction')['tp_min'] > 0
    for k in W.STATE:
        assert np.array_equal(P2.weathering_get(k), P.weathering_get(k)), k       # a zero period IS the mean, bit for bit
    P3, _ = _particles(ctx, ids, z, age, dict(env, tp=np.full(n, mean, np.float32)))
    _table(P3, oil, rho_w, n_total, state, mc)
    P3.oil_weather(900., which)
    breaking = (env['xwind'] > 5) & (env['tp'] > 0) & (env['tp'] != mean)
    got, other = P.weathering_get('mass_dispersed')[ids], P3.weathering_get('mass_dispersed')[ids]
    assert (got[breaking] != other[breaking]).sum() >= 5 and np.array_equal(got[~breaking], other[~breaking])
    for q in (P, P2, P3):
        q.close()


def test_setup_refusals(ctx):
    P = ctx.particles(4)
    P.append(np.zeros(4), np.zeros(4))
    with pytest.raises(OdrError, match='no weathering table'):
        P.oil_budget(1)
    oil, n_total, ids, env, z, age, state, mc = _synthetic(4, 3, 1)
    P.weathering_setup(oil, 3)
    for k in (1, 2):
        P.set_property(k, np.zeros(4, np.float32))
    with pytest.raises(OdrError, match='sampled'):
        P.oil_weather(900.)
    _upload_env(P, dict(env, hs=np.ones(4)), np.arange(4))
    with pytest.raises(OdrError, match='has no row'):       # four elements, IDs 0 .. 3, three rows
        P.oil_weather(900.)
    with pytest.raises(ValueError, match='rows'):
        P.weathering_seed(2, np.ones(2), oil['mass_fraction'], 870., 1e-5)
    P.close()


# ------------------------------------------------------------------------------------------------ the state follows the ID
def test_state_follows_the_id_through_compaction_and_the_sort(ctx):
    n, ncomp, rho_w = 3000, 7, 1026.95
    oil, _, _, _, _, _, state, mc = _synthetic(n - 3, ncomp, 77)
    rng = np.random.default_rng(5)
    nx, ny = 24, 16
    sid = ctx.add_grid(np.arange(nx, dtype=np.float64), 50.0 + np.arange(ny, dtype=np.float64), lon_mode=2)
    ctx.upload_block(sid, 0, 0.0, {U: np.zeros((ny, nx), np.float32)})
    lon, lat = rng.uniform(0.5, nx - 1.5, n), rng.uniform(50.5, 50 + ny - 1.5, n)
    z = np.where(rng.uniform(size=n) < 0.4, -rng.uniform(0.1, 30, n), 0.0)
    env_of = dict(xwind=rng.uniform(0, 16, n).astype(np.float32), ywind=rng.uniform(-3, 3, n).astype(np.float32),
                  temp=rng.uniform(1, 22, n).astype(np.float32), hs=np.zeros(n, np.float32), tp=np.zeros(n, np.float32))
    gone = np.zeros(n, bool)
    gone[5::11] = True
    which = ['properties', 'evaporation', 'emulsification', 'dispersion', 'half_time']

    def run(disturb):
        P, _ = _particles(ctx, np.arange(n), z, np.full(n, 900.), env_of, lon, lat)
        _table(P, oil, rho_w, n, state, mc)
        snaps = []
        for step in range(3):
            if disturb and step == 1:
                P.deactivate(gone[P.ids()], 1)
                assert P.compact() == n - gone.sum()
            if disturb and step == 2:
                P.sort_by_cell(sid, keep_environment=False)
            order = P.ids()
            _upload_env(P, env_of, order)
            P.oil_weather(900., which)
            P.increase_age(900.)
            snaps.append({k: P.weathering_get(k) for k in W.STATE + ['mass_components']})
        order, budget = P.ids(), P.oil_budget(1)
        P.close()
        return snaps, order, budget
    plain, order0, budget0 = run(False)
    moved, order1, budget1 = run(True)
    assert not np.array_equal(order1, np.sort(order1)) and len(order1) == n - gone.sum()
    for k in W.STATE + ['mass_components']:
        assert np.array_equal(moved[2][k][~gone], plain[2][k][~gone]), k          # bit for bit by ID
        assert np.array_equal(moved[2][k][gone], plain[0][k][gone]), k            # the deactivated keep the rows they left with
    assert budget1['n'] == n == budget0['n'] and budget1['mass_stranded'] > 0 and budget0['mass_stranded'] == 0
    seeded = state['mass_oil'] + state['mass_evaporated'] + state['mass_dispersed']
    for b in (budget0, budget1):
        # every process conserves an element's mass to an ulp or two: three steps of four processes stay far inside 64 ulp
        assert abs(b['mass_total'] / seeded.sum() - 1) <= 64 * 2.220446049250313e-16
        assert b['mass_total'] == b['mass_dispersed'] + b['mass_submerged'] + b['mass_surface'] + b['mass_stranded'] + b['mass_evaporated'] + \
            b['mass_biodegraded']


# ------------------------------------------------------------------------------------------------ the model run
def _reader(G, case):
    g = {k[len(case) + 3:]: G.G[k] for k in G.G.files if k.startswith(case + '_g_')}
    times = [T0 + timedelta(seconds=900. * k) for k in range(16)]
    one = np.ones((len(times), 1, 1), np.float32)
    return readers.GridReader(g['x'], g['y'], times, {k: one * v for k, v in g.items() if k not in 'xy'})


def _budget_of(mass, status, z, stranded):
    """get_oil_budget's masks (openoil.py:1282-1303) on arrays by element ID, NaN where the element is not there."""
    m = {k: np.nan_to_num(v) for k, v in mass.items()}
    st, surf = status == stranded, z == 0
    b = dict(mass_surface=m['mass_oil'][surf & ~st].sum(), mass_submerged=m['mass_oil'][~surf & ~st].sum(), mass_stranded=m['mass_oil'][st].sum(),
             mass_evaporated=m['mass_evaporated'].sum(), mass_dispersed=m['mass_dispersed'].sum(), mass_biodegraded=m['mass_biodegraded'].sum())
    b['mass_total'] = b['mass_dispersed'] + b['mass_submerged'] + b['mass_surface'] + b['mass_stranded'] + b['mass_evaporated'] + b['mass_biodegraded']
    return b


# Largest relative difference of the device run from the reference's run of case (r), measured on the MI355X (1.505e-08: the
# device's float32 powf in the mass transport coefficient lies a float32 ulp from NumPy's on some winds), doubled: see DESIGN.md
# section 7i.  The run has drift:vertical_mixing off: with it on the reference draws its mixing numbers from np.random in a
# different order than the device path (opendrift_amd/openoil.py), elements are at the surface in different steps, and neither
# statuses nor masses can agree.
RUN_TOLERANCE = 2 * 1.505e-08


def test_model_run_against_the_reference(G):
    from opendrift_amd.openoil import OpenOil
    case = 'r'
    o = OpenOil(loglevel=50, seed=0, weathering_model='noaa')
    o.add_reader(_reader(G, case))
    o.set_config('general:use_auto_landmask', False)
    o.set_config('seed:ocean_only', False)
    o.set_config('drift:vertical_mixing', False)
    o.set_config('drift:current_uncertainty', 0)
    o.set_config('drift:wind_uncertainty', 0)
    o.set_config('drift:stokes_drift', False)
    n = len(G.g(case, 'lon'))
    o.seed_elements(lon=G.g(case, 'lon'), lat=G.g(case, 'lat'), z=G.g(case, 'z_seed'), time=T0, number=n, m3_per_hour=2.0,
                    oil_film_thickness=0.001, wind_drift_factor=0.02, biodegradation_half_time_droplet=0.8,
                    biodegradation_half_time_slick=2.5, oil_type=G.oil(case))
    assert np.array_equal(o._weather_sched['mass_oil'], G.g(case, 'seeded_mass'))
    steps = G.steps_of_run(case)
    o.run(time_step=900, steps=steps)
    # statuses at every output time, by element ID
    cats = list(G.g(case, 'status_categories'))
    assert o.status_categories[:len(cats)] == cats
    status = o.result['status']
    for k in range(steps):      # (the result holds an element up to the output time it left at; the golden keeps its last status)
        got, exp = status[:, k], G.g(case, 'end_status')[k]
        there = ~np.isnan(got)
        assert np.array_equal(got[there].astype(int), exp[there]) and (exp[~there] != 0).all() and (exp[there] == 0).sum() == (exp == 0).sum(), k
    left = G.g(case, 'end_status')[steps - 1] != 0
    assert ((status[:, :steps] == cats.index('stranded')).sum(axis=1)[left] == 1).all()      # each recorded once as stranded
    # the masses behind the last step, by element ID, and the budget series
    worst = 0.0
    for k in ('mass_oil', 'mass_evaporated', 'mass_dispersed'):
        got, exp = o.P.weathering_get(k), G.g(case, 'end_' + k)[-1]
        worst = max(worst, float(np.max(np.abs(got - exp) / np.maximum(np.abs(exp), 1e-300), where=exp != 0, initial=0.0)))
    budget = o.get_oil_budget()
    assert set(budget) == set(_abi.OIL_BUDGET) | {'oil_density'} and len(budget['mass_total']) == steps + 1
    seeded = G.g(case, 'seeded_mass')
    stranded = cats.index('stranded')
    zero = {k: np.zeros(n) for k in ('mass_evaporated', 'mass_dispersed', 'mass_biodegraded')}
    z_seed = G.g(case, 'z_seed').astype(np.float32).astype(np.float64)
    for k in range(steps):
        mass = dict(zero, mass_oil=seeded) if k == 0 else {q: G.g(case, 'end_' + q)[k - 1] for q in W.STATE[:4]}
        exp = _budget_of(mass, G.g(case, 'end_status')[k], z_seed if k == 0 else G.g(case, 'end_z')[k - 1], stranded)
        for q, v in exp.items():
            if v:
                worst = max(worst, abs(budget[q][k] / v - 1))
            else:
                assert budget[q][k] == 0, (q, k)
        # mass_total equals the seeded mass at every output time: the golden's own drift is 2.2e-16 (tools/gen_golden_openoil_weathering.py
        # prints it), twice that is the bound; measured on the MI355X: 2.2e-16
        assert abs(budget['mass_total'][k] / seeded.sum() - 1) <= 2 * 2.220446049250313e-16, k
    assert budget['mass_stranded'][0] > 0 and budget['mass_stranded'][-1] > budget['mass_stranded'][0] * 0.9
    print('largest relative difference of masses and budget from the reference: %.3e; of mass_total from the seeded mass: %.3e' % (
        worst, np.abs(budget['mass_total'] / seeded.sum() - 1).max()))
    assert worst <= RUN_TOLERANCE
    o.P.close()


def test_model_run_with_vertical_mixing(G):
    """Weathering and the mixing loop together: the launch stores the emulsion's density and viscosity, rounded to float32, in the
    property slots the mixing kernels read (deviation (i)).  The reference's run cannot be the yardstick (see
    RUN_TOLERANCE); what is held here: the slots are the table's values, elements are entrained and resurface, the budget keeps the
    seeded mass, and two runs agree bit for bit."""
    from opendrift_amd.openoil import OpenOil
    case = 'r'
    n, steps = len(G.g(case, 'lon')), G.steps_of_run(case)

    def run():
        o = OpenOil(loglevel=50, seed=0, weathering_model='noaa')
        o.add_reader(_reader(G, case))
        o.set_config('general:use_auto_landmask', False)
        o.set_config('seed:ocean_only', False)
        o.set_config('vertical_mixing:timestep', 60)
        assert o.get_config('drift:vertical_mixing') is True
        o.seed_elements(lon=G.g(case, 'lon'), lat=G.g(case, 'lat'), z=0., time=T0, number=n, m3_per_hour=2.0, oil_film_thickness=0.001,
                        oil_type=G.oil(case))
        o.run(time_step=900, steps=steps)
        return o
    o = run()
    order = o.P.ids()
    assert len(order) > 0
    for k, name in ((1, 'density'), (2, 'viscosity')):
        table = o.P.weathering_get(name)[order]
        assert np.array_equal(o.P.get_property(k), table.astype(np.float32)), name       # the slots the mixing kernels read
        assert (table != o._weather_sched[name][0]).any(), name                          # the emulsion's values, not the seeded ones
    z = np.nan_to_num(np.array(o.result['z']))
    entrained = (z < 0).any(axis=1)
    print('entrained at some output time: %d of %d, of them at the surface at the end: %d' % (
        entrained.sum(), n, ((z[:, -1] == 0) & entrained).sum()))
    assert entrained.sum() >= 5                   # every element was seeded at the surface: the mixing loop ran on the stored values
    budget = o.get_oil_budget()
    seeded = o._weather_sched['mass_oil'].sum()
    # an element's mass passes through three processes per step, each conserving it to an ulp or two (<= 2 * 3 * steps ulp); the
    # reduction folds n values as a tree (log2(n) + 1 roundings)
    bound = (6 * steps + np.log2(n) + 1) * 2.220446049250313e-16
    drift = np.abs(budget['mass_total'] / seeded - 1).max()
    print('mass_total against the seeded mass with mixing on: %.3e (bound %.3e)' % (drift, bound))
    assert drift <= bound
    assert budget['mass_submerged'].max() > 0 and budget['mass_evaporated'][-1] > 0 and budget['mass_dispersed'][-1] > 0
    o2 = run()
    b2 = o2.get_oil_budget()
    for k in _abi.OIL_BUDGET:
        assert np.array_equal(budget[k], b2[k]), k
    for k in W.STATE:
        assert np.array_equal(o.P.weathering_get(k), o2.P.weathering_get(k)), k
    o.P.close()
    o2.P.close()
