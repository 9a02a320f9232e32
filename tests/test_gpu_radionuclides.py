"""GPU: RadionuclideDrift -- the three launches of csrc/odr_radio.hip.h against the host build of the same header and against the
reference (golden C30, tools/gen_golden_radionuclides.py) with the reference's draws, small shapes, the device RNG's statistics,
the species-aware sea-floor action in every kernel that honours it, and the model run.

Deviation of the device from the host build, measured on the MI355X: none -- specie, moving, counters, z,
the float32 diameter and the float32 terminal velocity come out bit for bit (every operation is an IEEE operation in the same
order; the exponentials may differ by an ulp, which no decision of the golden comes near).  Four times that is still none:
the comparisons below are for equality."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden
from opendrift_amd import _abi, readers
from opendrift_amd._abi import OdrError
from opendrift_amd.device import Context, Particles

import radio_host as R

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
U, V, DEPTH, SSH, SAL, TEMP = ('x_sea_water_velocity', 'y_sea_water_velocity', 'sea_floor_depth_below_sea_level', 'sea_surface_height',
                               'sea_water_salinity', 'sea_water_temperature')
KZ, W, XW, YW, MLD, LAND = 'ocean_vertical_diffusivity', 'upward_sea_water_velocity', 'x_wind', 'y_wind', 'ocean_mixed_layer_thickness', 'land_binary_mask'
CONC3_ID = _abi.VARIABLES['sea_surface_swell_wave_significant_height']
SHAPES = [1, 63, 64, 65, 255, 256, 257, 1000]


@pytest.fixture(scope='module')
def G():
    return R.Golden()


def _particles(ctx, n, specie, diameter, moving, z, env):
    ctx.slot_aliases['conc3'] = CONC3_ID
    P = ctx.particles(n)
    P.append(np.linspace(4, 5, n), np.full(n, 60.0), z=np.asarray(z, np.float64), moving=np.asarray(moving, np.int32))
    P.set_property(0, np.asarray(diameter, np.float32))
    P.set_property(2, np.full(n, 2650., np.float32))
    P.set_property(3, np.asarray(specie, np.float32))
    for k, v in env.items():
        P.env_upload(k, np.asarray(v, np.float32))
    return P


def _state(P):
    d = P.download()
    return dict(specie=P.get_property(3), diameter=P.get_property(0), moving=d['moving'], z=d['z'])


def _same(a, b, what):
    for k in ('specie', 'moving', 'diameter'):
        assert np.array_equal(a[k], b[k]), '%s: %s' % (what, k)
    assert np.array_equal(a['z'].view(np.uint64), np.asarray(b['z'], np.float64).view(np.uint64)), '%s: z' % what


# ------------------------------------------------------------------------------------------------ the launches against C30
@pytest.mark.parametrize('case', ['a', 'b'])
def test_launches_reproduce_the_reference_and_the_host_build(ctx, G, case):
    """Every step of C30 in ODR_RNG_HOST mode: speciation, terminal velocity, resuspension.  Integers identical to the reference's
    and the host build's; z, diameter and terminal velocity identical to the host build's (the module docstring)."""
    m, dt = G.setup(case), G.dt(case)
    S = None
    for s in range(G.steps(case)):
        inp, draws, exp = G.speciation_step(case, s)
        n = len(inp['z'])
        P = _particles(ctx, n, inp['specie'], inp['diameter'], inp['moving'], inp['z'],
                       {SAL: inp['sal'], DEPTH: inp['depth'], 'conc3': inp['conc3']})
        S = S or P.radio_setup(**m)
        S.counts(reset=True)
        P.radio_speciation(S, dt, **draws)
        got, host = _state(P), R.speciation(m, dt, **inp, **draws)
        _same(got, host, 'step %d speciation, host build' % s)
        assert np.array_equal(got['specie'], exp['specie']) and np.array_equal(got['moving'], exp['moving'])
        c = S.counts(reset=True)
        assert np.array_equal(c, exp['counts']) and np.array_equal(c, host['counts'])
        z = got['z']
        if exp['z_f32']:
            z = np.where(z != inp['z'], z.astype(np.float32).astype(np.float64), z)
        assert np.array_equal(z, exp['z']) and np.array_equal(got['diameter'], exp['diameter'])
        # terminal velocity on the state behind the speciation
        tin, tv = G.terminal_velocity_step(case, s)
        P.env_upload(TEMP, tin['temperature'])
        P.radio_terminal_velocity()
        w = P.download_f32('terminal_velocity')
        assert np.array_equal(w, R.terminal_velocity(**tin))
        nz = tv != 0
        assert (np.abs(w[nz].astype(np.float64) - tv[nz]) <= 4 * 1.192e-7 * np.abs(tv[nz])).all() and (w[~nz] == 0).all()
        P.close()
        # resuspension on the state the reference had in front of it
        inp, draws, exp = G.resuspension_step(case, s)
        P = _particles(ctx, n, inp['specie'], inp['diameter'], inp['moving'], inp['z'], {U: inp['u'], V: inp['v'], DEPTH: inp['depth']})
        P.radio_resuspend(S, **draws)
        got, host = _state(P), R.resuspend(m, **inp, **draws)
        _same(got, host, 'step %d resuspension, host build' % s)
        _same(got, exp, 'step %d resuspension, reference' % s)
        c = S.counts(reset=True)
        assert np.array_equal(c, exp['counts']) and np.array_equal(c, host['counts'])
        P.close()
    S.close()


# ------------------------------------------------------------------------------------------------ small shapes
def _population(m, n, kind, seed):
    """kind 'mixed': every species, some on the sea bed; 'none': species whose row is empty (nothing can transform); 'all': u1 = 0
    for species with a rate (salinity above 20: in that table of the Al setup every row has one)."""
    rng = np.random.default_rng(seed)
    ns = m['nspecies']
    rates = m['rates'] if np.ndim(m['rates']) == 2 else m['rates'][3]
    has = np.flatnonzero(rates.sum(axis=1) > 0)
    empty = np.flatnonzero(rates.sum(axis=1) == 0)
    depth = rng.uniform(20, 40, n).astype(np.float32)
    specie = rng.integers(0, ns, n)
    if kind == 'none':
        specie = rng.choice(empty, n)
    elif kind == 'all':
        specie = rng.choice(has, n)
    z = -rng.uniform(0, 1, n) * depth
    bed = rng.random(n) < 0.4
    z[bed] = -depth[bed].astype(np.float64)
    moving = np.where(bed & (rng.random(n) < 0.7), 0, 1).astype(np.int32)
    u1 = np.zeros(n) if kind == 'all' else rng.random(n)
    return dict(specie=specie.astype(np.float32), diameter=np.where(rng.random(n) < 0.5, 0, 4e-5).astype(np.float32), moving=moving, z=z,
                sal=rng.uniform(21 if kind == 'all' else 0, 35, n).astype(np.float32), depth=depth, conc3=rng.uniform(5e-4, 3e-3, n).astype(np.float32)), \
        dict(u1=u1, u2=rng.random(n), diameter_noise=rng.normal(0, 2e-6, n), depth_noise=rng.normal(0, 0.8, n)), \
        dict(u=rng.uniform(-0.02, 0.02, n).astype(np.float32), v=rng.uniform(-0.02, 0.02, n).astype(np.float32))


@pytest.mark.parametrize('n', SHAPES)
def test_small_shapes_equal_the_host_build(ctx, G, n):
    """One wave, a wave boundary, a workgroup boundary, a ragged tail; a population in which nothing can transform (counters
    stay 0, nothing is written), one in which every element does, a mixed one; speciation and resuspension."""
    for case, empty_ok in (('a', True), ('b', False)):      # (every species of the Al setup has a rate)
        m, dt = G.setup(case), G.dt(case)
        S = None
        for kind in ('mixed', 'none', 'all') if empty_ok else ('mixed', 'all'):
            inp, draws, cur = _population(m, n, kind, seed=n)
            P = _particles(ctx, n, inp['specie'], inp['diameter'], inp['moving'], inp['z'],
                           {SAL: inp['sal'], DEPTH: inp['depth'], 'conc3': inp['conc3'], U: cur['u'], V: cur['v']})
            S = S or P.radio_setup(**m)
            S.counts(reset=True)
            P.radio_speciation(S, dt, **draws)
            got, host = _state(P), R.speciation(m, dt, **inp, **draws)
            _same(got, host, '%s %s n=%d' % (case, kind, n))
            c = S.counts(reset=True)
            assert np.array_equal(c, host['counts'])
            if kind == 'none':
                assert c.sum() == 0 and np.array_equal(got['specie'], inp['specie']) and np.array_equal(got['z'], inp['z'])
                assert np.array_equal(got['moving'], inp['moving']) and np.array_equal(got['diameter'], inp['diameter'])
            if kind == 'all':
                assert c.sum() == n
            noise = dict(diameter_noise=draws['diameter_noise'], depth_noise=draws['depth_noise'])
            P.radio_resuspend(S, **noise)
            got2 = _state(P)
            host2 = R.resuspend(m, host['specie'], host['diameter'], host['moving'], host['z'], cur['u'], cur['v'], inp['depth'], **noise)
            _same(got2, host2, '%s %s n=%d resuspension' % (case, kind, n))
            assert np.array_equal(S.counts(reset=True), host2['counts'])
            P.close()
        S.close()


# ------------------------------------------------------------------------------------------------ the device RNG
def _rng_run(ctx, m, dt, n, specie, sal, step, seed_ctx=None):
    c = seed_ctx or ctx
    P = _particles(c, n, np.full(n, specie), np.zeros(n), np.ones(n), np.full(n, -5.0),
                   {SAL: np.full(n, sal), DEPTH: np.full(n, 100.0), 'conc3': np.full(n, 2e-3)})
    S = P.radio_setup(**m)
    P.radio_speciation(S, dt, step=step)
    out, counts = _state(P), S.counts()
    S.close()
    P.close()
    return out, counts


def test_device_rng_statistics_and_reproducibility(ctx, G):
    """A STATISTICAL check: 200 000 LMM elements under uniform conditions far from the sea bed.  The transformed count within five
    binomial sigma of N psum, the split over the targets within five sigma of p_j / psum -- both from the rates, not measured.
    (Far from the bed an LMM element has ONE target; the split is checked on 200 000 LMMcation elements of the Al setup at
    salinity 15, which have three.)  The same (seed, step) twice: identical bits; another step: different."""
    n = 200000
    m, dt = G.setup('a'), 3600.0
    k = m['rates'][0, 1] * np.float32(2e-3).astype(np.float64) / 1e-3
    psum = 1 - np.exp(-k * dt)
    out, counts = _rng_run(ctx, m, dt, n, 0, 30.0, step=3)
    sigma = np.sqrt(n * psum * (1 - psum))
    print('LMM: transformed %d, expected %.1f +- %.1f' % (counts.sum(), n * psum, sigma))
    assert abs(counts.sum() - n * psum) < 5 * sigma
    assert counts[0, 1] == counts.sum() == (out['specie'] == 1).sum()      # the one target
    again, counts2 = _rng_run(ctx, m, dt, n, 0, 30.0, step=3)
    _same(out, again, 'same seed and step')
    assert np.array_equal(counts, counts2)
    other, _ = _rng_run(ctx, m, dt, n, 0, 30.0, step=4)
    assert (other['specie'] != out['specie']).sum() > n * psum * (1 - psum)
    # the new particles got a diameter around the mean with the configured spread (normal noise from the second block)
    d = out['diameter'][out['specie'] == 1].astype(np.float64)
    assert abs(d.mean() - m['particle_diameter']) < 5 * m['diameter_uncertainty'] / np.sqrt(len(d))
    assert abs(d.std() / m['diameter_uncertainty'] - 1) < 0.05
    # the split: LMMcation at salinity 15 (the table of (10, 20])
    mb, dtb = G.setup('b'), 3600.0
    p = 1 - np.exp(-mb['rates'][2, 0] * dtb)
    psum = p.sum()
    assert (p > 0).sum() == 3 and 0.3 < psum < 0.6
    out, counts = _rng_run(ctx, mb, dtb, n, 0, 15.0, step=1)
    nt = counts.sum()
    assert abs(nt - n * psum) < 5 * np.sqrt(n * psum * (1 - psum))
    for j in np.flatnonzero(p > 0):
        q = p[j] / psum
        print('LMMcation -> %d: %d, expected %.1f +- %.1f' % (j, counts[0, j], nt * q, np.sqrt(nt * q * (1 - q))))
        assert abs(counts[0, j] - nt * q) < 5 * np.sqrt(nt * q * (1 - q))
    assert counts[0][p == 0].sum() == 0 and counts[1:].sum() == 0


# ------------------------------------------------------------------------------------------------ the species-aware sea-floor action
def _flat_world(kz):
    c = Context(seed=1)
    for nm, fb in ((DEPTH, 5.0), (SSH, 0.0), (KZ, kz), (W, 0.0), (XW, 0.0), (YW, 0.0), (MLD, 50.0), (U, 0.0), (V, 0.0)):
        c.bind(nm, [], fb)
    return c


def _mix(make_ctx, lane, action, lon, lat, z0, tv, moving, specie, uni, dt=600.0, dt_mix=60.0):
    c = make_ctx()
    n = len(lon)
    P = c.particles(n)
    P.append(lon, lat, z=np.full(n, -1.0), terminal_velocity=tv)
    P.env_sample([U, V, W, DEPTH, SSH, XW, YW, MLD], 0.0)
    Zmin = -1. * (P.env_download(DEPTH) + P.env_download(SSH))
    P.upload(z=Zmin + z0 if np.ndim(z0) else z0, moving=moving)
    P.set_property(3, specie)
    P.store_previous()
    if action == 'species':
        c.set_seafloor_settle_species(3, [1, 3])
    elif action == 'empty':
        c.set_seafloor_settle_species(3, [])
    else:
        c.set_seafloor_action(action)
    if lane == 'buoyancy':
        P.vertical_buoyancy(dt)
    elif lane == 'windspeed_Large1994':
        P.vmix_analytic(lane, 1e-2, dt, dt_mix, uniforms=uni)
    else:
        P.vmix(0.0, dt, dt_mix, uniforms=uni)
    d = P.download()
    d['Zmin'] = Zmin
    P.close()
    c.close()
    return d


@pytest.mark.parametrize('lane', ['flat5', 'column', 'window', 'generic', 'windspeed_Large1994', 'buoyancy'])
def test_species_action_in_the_mixing_kernels_and_vertical_buoyancy(monkeypatch, lane):
    """ODR_SEAFLOOR_SETTLE_SPECIES: particle species (1, 3) and dissolved / sediment ones (0, 2, 4) driven below the sea floor
    -- a flat floor of 5 m under a constant diffusivity ('flat5'), the sloping floor of the SedimentDrift golden in every other
    kernel that honours the action.  An element of a species in the mask ends exactly as under ODR_SEAFLOOR_SETTLE, any other
    exactly as under ODR_SEAFLOOR_LIFT, bit for bit; an empty mask is the lift action."""
    from test_gpu_sedimentdrift import KLEV, _device_world, _settle_case
    g = golden('c26_sedimentdrift.npz')
    lon, lat, above, tv, moving, uni = _settle_case(g, n=3001, seed=8)
    n = len(lon)
    specie = (np.arange(n) % 5).astype(np.float32)
    moving = np.ones(n, np.int32)
    if lane == 'flat5':
        make, z0 = (lambda: _flat_world(0.02)), above * 0.6
    else:
        make, z0 = (lambda: _device_world(g, KLEV)), above
        monkeypatch.setenv('ODR_VMIX_WINDOW', '1' if lane == 'window' else '0')
        if lane == 'generic':
            monkeypatch.setenv('ODR_NO_FAST_PATH', '1')
    run = lambda action: _mix(make, lane, action, lon, lat, z0, tv, moving, specie, uni)      # noqa: E731
    settle, lift, got, empty = run('settle'), run('lift_to_seafloor'), run('species'), run('empty')
    particle = np.isin(specie, (1, 3))
    for k in ('z', 'moving', 'status', 'lon', 'lat'):
        assert np.array_equal(got[k], np.where(particle, settle[k], lift[k])), k
        assert np.array_equal(empty[k], lift[k]), k
    Zmin = got['Zmin'].astype(np.float64)
    hit = settle['moving'] == 0                     # the elements that went below the floor
    assert (hit & particle).sum() > n // 20 and (hit & ~particle).sum() > n // 20
    assert (got['moving'][hit & particle] == 0).all() and np.array_equal(got['z'][hit & particle], Zmin[hit & particle])
    assert (got['moving'][~particle] == 1).all() and (got['z'][~particle] >= Zmin[~particle]).all()
    assert (got['status'] == 0).all()


def test_species_action_needs_its_slot(ctx):
    P = ctx.particles(8)
    P.append(np.linspace(4, 5, 8), np.full(8, 60.0), z=np.full(8, -1.0))
    for nm, fb in ((DEPTH, 5.0), (SSH, 0.0)):
        ctx.bind(nm, [], fb)
    P.env_sample([DEPTH, SSH], 0.0)
    ctx.set_seafloor_settle_species(3, [1])
    with pytest.raises(OdrError, match='property slot 3') as e:
        P.vertical_buoyancy(600.0)
    assert e.value.code == -4
    import ctypes
    nb = ctypes.c_int64()
    with pytest.raises(ValueError, match='unknown seafloor action'):      # accepted by odr_set_seafloor_action only
        _abi.check(ctx.lib.odr_seafloor_action(ctx.h, P.h, 5, 0, ctypes.byref(nb)))
    ctx.set_seafloor_action('lift_to_seafloor')
    P.close()


# ------------------------------------------------------------------------------------------------ entry points report missing state
def test_entry_points_report_missing_state(ctx, G):
    m = G.setup('a')
    n = 300
    ctx.slot_aliases['conc3'] = CONC3_ID
    P = ctx.particles(n)
    P.append(np.linspace(4, 5, n), np.full(n, 60.0), z=np.full(n, -5.0))
    S = P.radio_setup(**m)

    def state_error(call, match):
        with pytest.raises(OdrError, match=match) as e:
            call()
        assert e.value.code == -4      # ODR_ERR_STATE

    state_error(lambda: P.radio_speciation(S, 3600.), 'property slot')
    state_error(lambda: P.radio_terminal_velocity(), 'property slot')
    state_error(lambda: P.radio_resuspend(S), 'property slot')
    P.set_property(0, np.full(n, 4e-5, np.float32))
    P.set_property(2, np.full(n, 2650., np.float32))
    P.set_property(3, np.zeros(n, np.float32))
    state_error(lambda: P.radio_speciation(S, 3600.), 'sea_floor_depth_below_sea_level')
    state_error(lambda: P.radio_terminal_velocity(), 'sea_water_temperature')
    state_error(lambda: P.radio_resuspend(S), 'x_sea_water_velocity')
    P.env_upload(DEPTH, np.full(n, 30., np.float32))
    state_error(lambda: P.radio_speciation(S, 3600.), 'conc3')
    P.env_upload(U, np.zeros(n, np.float32))
    state_error(lambda: P.radio_resuspend(S), 'y_sea_water_velocity')
    P.env_upload(TEMP, np.full(n, 8., np.float32))
    state_error(lambda: P.radio_terminal_velocity(), 'sea_water_salinity')
    Sb = P.radio_setup(**G.setup('b'))
    state_error(lambda: P.radio_speciation(Sb, 3600.), 'sea_water_salinity')
    Sb.close()
    with pytest.raises(ValueError):      # host draws of the wrong length
        P.radio_speciation(S, 3600., u1=np.zeros(3), u2=np.zeros(3), diameter_noise=np.zeros(3), depth_noise=np.zeros(3))
    # a species number outside the table: reported by name when the counters are read, the element untouched, nothing faults
    P.env_upload('conc3', np.full(n, 2e-3, np.float32))
    P.env_upload(V, np.zeros(n, np.float32))
    sp = np.zeros(n, np.float32)
    sp[7], sp[299] = 7, -2
    P.set_property(3, sp)
    P.radio_speciation(S, 3600., u1=np.ones(n), u2=np.zeros(n), diameter_noise=np.zeros(n), depth_noise=np.zeros(n))
    with pytest.raises(OdrError, match='outside the table') as e:
        S.counts(reset=True)
    assert e.value.code == -4
    assert np.array_equal(P.get_property(3), sp)
    P.radio_resuspend(S)
    with pytest.raises(OdrError, match='outside the table'):
        S.counts(reset=True)
    assert not S.counts().any()
    with pytest.raises(ValueError):
        P.radio_setup(**dict(m, nspecies=8))
    with pytest.raises(ValueError):
        P.radio_setup(**dict(m, sediment_rev=9))
    S.close()
    P.close()


# ------------------------------------------------------------------------------------------------ the model
def _model(G, case, rng, seed=0, n=None, sort_every=None, steps=None, cls=None, config=(), at_edge=0):
    from opendrift_amd import RadionuclideDrift
    g, c = G.G, case + '_'
    steps = steps or G.steps(case)
    times = [T0 + timedelta(seconds=float(t)) for t in np.arange(steps + 2) * G.dt(case)]
    fields = {k[len(c) + 2:]: np.repeat(g[k][None], len(times), axis=0) for k in g.files if k.startswith(c + 'g_') and k[len(c) + 2:] not in 'xy'}
    o = (cls or RadionuclideDrift)(loglevel=50, seed=seed, rng=rng)
    o.add_reader(readers.GridReader(g[c + 'g_x'], g[c + 'g_y'], times, fields))
    o.set_config('environment:constant:horizontal_diffusivity', 0.0)
    o.set_config('radionuclide:isotope', '241Am' if case == 'a' else 'Al')
    o.set_config('radionuclide:specie_setup', 'LMM + Rev + Slow rev + Irrev' if case == 'a' else 'LMM + Colloid + Rev')
    o.set_config('vertical_mixing:timestep', float(g[c + 'dt_mix']))
    for k, v in zip(g[c + 'config_keys'].tolist(), g[c + 'config_values'].tolist()):
        o.set_config(k, v)
    for k, v in config:
        o.set_config(k, v)
    tiles = 1 if n is None else -(-n // len(g[c + 'seed_lon']))
    pop = {k: np.tile(g[c + 'seed_' + k], tiles)[:n] for k in ('lon', 'lat', 'z')}
    if at_edge:      # every at_edge-th element within 0.01 degrees of the reader's eastern edge, where the current takes it out of the domain
        pop['lon'] = pop['lon'].copy()
        pop['lon'][::at_edge] = g[c + 'g_x'][-1] - np.linspace(0.0005, 0.0095, len(pop['lon'][::at_edge]))
    o.seed_elements(time=T0, number=len(pop['lon']), specie=np.tile(g[c + 'seed_specie'], tiles)[:n].astype(int),
                    diameter_rng=np.random.default_rng(3), **pop)
    if sort_every is not None:
        o.sort_every = sort_every
    return o, steps


def test_run_device_rng_species_census(G):
    """A STATISTICAL check: the run of C30's case (a) with the device RNG against the reference's census of species after the
    last step.  The two runs share nothing but the model, so each species fraction f carries the binomial sigma sqrt(f (1 - f) / N)
    in BOTH; the difference of two independent estimates has sqrt(2) times that, and the bound is five of those."""
    o, steps = _model(G, 'a', 'device', seed=2)
    o.run(time_step=G.dt('a'), steps=steps)
    e = o.elements
    n = len(e.ID)
    ref = G.G['a_specie3'][-1]
    assert n == len(ref)
    for k in range(o.nspecies):
        f = (ref == k).mean()
        sigma = np.sqrt(2 * max(f * (1 - f), 1.0 / n) / n)
        got = (e.specie == k).mean()
        print('%-28s reference %.4f, device %.4f (%.2f sigma)' % (o.name_species[k], f, got, abs(got - f) / sigma))
        assert abs(got - f) < 5 * sigma
    nt = o.ntransformations
    assert nt.shape == (7, 7) and nt.sum() > n and (nt[G.G['a_transfer_rates'] == 0].sum() == nt[1, 2] + nt[3, 4] + nt[5, 6] + nt[2, 1] + nt[4, 3] + nt[6, 5])
    assert (e.moving == 0).sum() > n // 20 and set(np.unique(e.moving)) <= {0, 1}
    sediment = np.isin(e.specie, (2, 4, 6))
    assert (e.moving[sediment] == 0).all() and (e.moving[~sediment] == 1).all()


def test_run_numpy_rng_equals_the_sequence_issued_by_hand(G):
    """rng='numpy': update() with np.random seeded equals the same launches issued through device.py with the same draws, bit for
    bit.  In every step, on the state and environment the run has in front of update(), the whole sequence -- speciation,
    terminal velocity, mixing with the species-aware sea-floor action, resuspension, current advection, vertical advection -- is
    issued by hand on a second particle set of the run's own context (whose readers the advection samples); np.random is then put
    back and the run's own update() follows."""
    from opendrift_amd import RadionuclideDrift
    from opendrift_amd.oceandrift import _epoch

    class Recording(RadionuclideDrift):
        def by_hand(self):
            P, n = self.P, self.num_elements_active()
            d, m = P.download(), self.setup_members()
            dt, dt_mix = self.time_step.total_seconds(), self.get_config('vertical_mixing:timestep')
            H = self.ctx.particles(n)
            H.append(d['lon'], d['lat'], z=d['z'], moving=d['moving'], id=d['ID'])
            for slot in (0, 1, 2, 3):
                H.set_property(slot, P.get_property(slot))
            for k in self._sampled:
                H.env_upload(k, P.env_download(k))
            S = H.radio_setup(**m)
            un = m['diameter_uncertainty']
            H.radio_speciation(S, dt, u1=np.random.random(n), u2=np.random.random(n), diameter_noise=np.random.normal(0., un, n),
                               depth_noise=np.random.normal(0, m['desorption_depth_uncert'], n))
            H.radio_terminal_velocity()
            uni = np.stack([np.random.random(n) for _ in range(int(dt / dt_mix))])
            self.ctx.set_seafloor_settle_species(3, self.particle_species())
            H.vmix_analytic('windspeed_Large1994', self.get_config('vertical_mixing:background_diffusivity'), dt, dt_mix, mix_at_surface=True,
                            uniforms=uni)
            H.radio_resuspend(S, diameter_noise=np.random.normal(0., un, n), depth_noise=np.random.normal(0, m['resuspension_depth_uncert'], n))
            H.advect(self.get_config('drift:advection_scheme'), _epoch(self.time), dt)
            H.vertical_advection(dt, self.get_config('drift:vertical_advection_at_surface'))
            out = dict(H.download(), specie=H.get_property(3), diameter=H.get_property(0), tv=H.download_f32('terminal_velocity'),
                       counts=S.counts(), specie_before=P.get_property(3))
            S.close()
            H.close()
            return out

        def update(self):
            state = np.random.get_state()
            hand = self.by_hand()
            np.random.set_state(state)
            before = self.ntransformations.copy()
            super().update()
            P = self.P
            got = dict(P.download(), specie=P.get_property(3), diameter=P.get_property(0), tv=P.download_f32('terminal_velocity'),
                       counts=self.ntransformations - before)
            self.records.append((hand, got))

    o, steps = _model(G, 'a', 'numpy', n=600, steps=3, cls=Recording)
    assert o.get_config('drift:vertical_advection') is True
    o.records = []
    np.random.seed(5)
    o.run(time_step=G.dt('a'), steps=steps)
    assert len(o.records) == steps
    changed = moved = 0
    for hand, got in o.records:
        for k in ('ID', 'lon', 'lat', 'z', 'moving', 'specie', 'diameter', 'tv', 'status', 'counts'):
            assert np.array_equal(got[k], hand[k]), k
        changed += int((got['specie'] != hand['specie_before']).sum())
        moved += int(got['counts'].sum())
    assert changed > 100 and moved >= changed


def test_properties_survive_compaction_and_the_periodic_sort(G, monkeypatch):
    """More elements than the re-sort threshold of run(), a re-sort in EVERY step, and every 25th element seeded at the reader's
    eastern edge, where the current takes it out of the domain (missing data: deactivated and compacted away, the survivors moved
    into the holes): the device order is no longer the seeding order, and specie, diameter, density, moving, z by element ID are
    those of the same run without any re-sort (the draws are keyed by element ID); so are the counters."""
    n = 70000

    def run(sort_every):
        sorts, sort_by_cell = [], Particles.sort_by_cell
        monkeypatch.setattr(Particles, 'sort_by_cell', lambda P, *a, **k: (sorts.append(len(P)), sort_by_cell(P, *a, **k))[1])
        o, steps = _model(G, 'a', 'device', seed=4, n=n, sort_every=sort_every, steps=3, at_edge=25)
        o.run(time_step=G.dt('a'), steps=steps)
        monkeypatch.setattr(Particles, 'sort_by_cell', sort_by_cell)
        return o, sorts
    a, sorts = run(1)
    b, none = run(0)
    assert len(sorts) == 3 and not none
    ea, eb = a.elements, b.elements
    gone = a.num_elements_deactivated()
    print('deactivated', gone, 'of', n, '| elements present at the re-sorts', sorts)
    assert 1000 < gone <= n // 25 and len(ea.ID) + gone == n and gone == b.num_elements_deactivated()
    assert len(ea.ID) > 65536 and sorts[-1] < n                # (a re-sort ran on a compacted set)
    assert not (np.diff(a.P.ids()) > 0).all()      # the device order is no longer the seeding order
    ia, ib = np.argsort(ea.ID), np.argsort(eb.ID)
    assert np.array_equal(ea.ID[ia], eb.ID[ib])
    for q in ('specie', 'diameter', 'density', 'neutral_buoyancy_salinity', 'moving', 'z', 'lon', 'lat', 'terminal_velocity'):
        assert np.array_equal(getattr(ea, q)[ia], getattr(eb, q)[ib]), q
    # an element that never was a particle keeps the diameter 0 it was seeded with; density is the seeded one for everybody
    assert (ea.density == np.float32(2650)).all() and len(np.unique(ea.specie)) == 7
    seeded = np.tile(G.G['a_seed_specie'], -(-n // len(G.G['a_seed_specie'])))[:n]
    untouched = (seeded[ea.ID] == 0) & (ea.specie == 0) & (ea.diameter == 0)
    assert untouched.sum() > 100
    assert np.array_equal(a.ntransformations, b.ntransformations) and a.ntransformations.sum() > n
