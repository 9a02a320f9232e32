"""CPU: the per-element code of the NOAA oil weathering launch (opendrift_amd/csrc/odr_weather.hip.h, compiled for the host by
tests/weather_host.cpp) replays every step of the golden C39 -- the reference's own OpenOil, tools/gen_golden_openoil_weathering.py
-- from the reference's state in front of the step and in front of each process, and is compared with the state behind it.

Masks and counts are compared exactly, density and fraction_evaporated (+ - * / only) bit for bit, the values behind exp / pow to
weather_host.BOUNDS, which says where its figures come from; the measured distances are printed (pytest -s)."""
import numpy as np
import pytest

import weather_host as W

G = W.Golden()


def _sub(d, ids):
    return {k: v[ids] for k, v in d.items()}


def _same_f32(case, s, ids, env, dt):
    """Elements on which the host build's float32 pow / exp chains give the values NumPy gave the reference (stored with the golden):
    (mass transport, Adcroft's fraction)."""
    ws = np.sqrt(env['xwind']**2 + env['ywind']**2)
    same_K = G.g(case, 'e_K')[s][ids] == W.mass_transport(ws)
    if case + '_b_fraction' not in G.G.files:
        return same_K, np.ones(len(ids), bool)
    return same_K, G.g(case, 'b_fraction')[s][ids] == W.adcroft_fraction(G.g(case, 'p_temp')[s][ids], dt)


def _check(worst, tag, out, mc, exp, mc_exp, sel=slice(None), regime='all'):
    for k in W.STATE:
        u = W.ulps(out[k][sel], exp[k][sel])
        worst[(tag, k)] = max(worst.get((tag, k), 0), float(u.max()) if u.size else 0.)
        assert (u <= W.BOUNDS[regime][k]).all(), (tag, k, u.max())
    u = W.ulps(mc[sel], mc_exp[sel])
    worst[(tag, 'mass_components')] = max(worst.get((tag, 'mass_components'), 0), float(u.max()) if u.size else 0.)
    assert (u <= W.BOUNDS[regime]['mass_components']).all(), (tag, u.max())


@pytest.mark.parametrize('case', W.Golden.CASES)
def test_whole_step_replay(case):
    oil, rho_w, dt, procs = G.oil(case), G.rho_w(case), G.dt(case), G.processes(case)
    worst = {}
    for s in range(G.steps(case)):
        ids, env, z, age = G.inputs(case, s)
        front, behind = _sub(G.state(case, s, None), ids), _sub(G.state(case, s, 'b'), ids)
        out, mc, red, tk = W.step(oil, rho_w, ['properties'] + procs, dt, env, z, age, front, G.mc(case, s, None)[ids])
        assert np.array_equal(tk, G.g(case, 'p_temp')[s][ids])                  # the Kelvin conversion, float32
        assert red['n_surface'] == (z == 0).sum()
        surf_age = age[z == 0]
        assert red['min_age_surface'] == (surf_age.min() if surf_age.size else np.inf)
        # masks: who evaporated, who emulsified
        for k in ('mass_evaporated', 'water_fraction', 'interfacial_area', 'mass_dispersed', 'mass_biodegraded'):
            assert np.array_equal(out[k] != front[k], behind[k] != front[k]), (s, k)
        assert np.array_equal(out['water_fraction'] == oil['emulsion_water_fraction_max'],
                              behind['water_fraction'] == oil['emulsion_water_fraction_max'])
        _check(worst, 'step', out, mc, behind, G.mc(case, s, 'b')[ids], regime=case)
        # with no sampled wave height the launch derives it from the wind: the float32 value the reference had stored.  Case (d)
        # has a wave-height reader: its heights are the reader's and there is nothing to derive.
        derived = np.array_equal(G.g(case, 's0_env_hs')[s][ids], np.float32(0.0246) * (env['xwind']**2 + env['ywind']**2))
        assert derived == (case != 'd'), (case, s)
        if not derived:
            continue
        out0, mc0, red0, _ = W.step(oil, rho_w, ['properties'] + procs, dt, dict(env, hs=np.zeros_like(env['hs'])), z, age, front,
                                    G.mc(case, s, None)[ids])
        assert red0['hs_max'] == 0 and red['hs_max'] > 0
        assert all(np.array_equal(out0[k], out[k]) for k in W.STATE) and np.array_equal(mc0, mc)
    print(case, {k: v for k, v in sorted(worst.items()) if v})


@pytest.mark.parametrize('case', W.Golden.CASES)
def test_each_process_from_the_state_in_front_of_it(case):
    oil, rho_w, dt, procs = G.oil(case), G.rho_w(case), G.dt(case), G.processes(case)
    worst = {}
    for s in range(G.steps(case)):
        ids, env, z, age = G.inputs(case, s)
        same_K, same_fr = _same_f32(case, s, ids, env, dt)
        before = None
        for pr in ['properties'] + procs:
            q = G._stage_prefix(pr)
            front, behind = _sub(G.state(case, s, before), ids), _sub(G.state(case, s, q), ids)
            out, mc, red, _ = W.step(oil, rho_w, [pr], dt, env, z, age, front, G.mc(case, s, before)[ids])
            _check(worst, pr, out, mc, behind, G.mc(case, s, q)[ids], regime=case)
            sel = same_K if pr == 'evaporation' else same_fr if pr == 'Adcroft' else slice(None)
            _check(worst, pr + ' (float32 functions agree)', out, mc, behind, G.mc(case, s, q)[ids], sel, 'same')
            for k in W.STATE:       # a process leaves alone what the reference's leaves alone
                untouched = behind[k] == front[k]
                assert np.array_equal(out[k][untouched], front[k][untouched]), (pr, k)
            before = q
    print(case, {k: v for k, v in sorted(worst.items()) if v})


def test_the_one_bound_of_all_cases_is_their_maximum():
    """The GPU tests hold the device to BOUNDS['all'] (the device's powf / expf are a third implementation: which elements carry the
    float32 ulp differs, so a case's own figure does not transfer); here the host build is held to each case's own."""
    for k, v in W.BOUNDS['all'].items():
        assert v == max(W.BOUNDS[c][k] for c in W.Golden.CASES), k


def test_golden_covers_what_it_is_for():
    a = 'a'
    ws = np.hypot(G.g(a, 's0_env_xwind')[0], G.g(a, 's0_env_ywind')[0])
    assert (ws >= 10).sum() >= 5 and (ws < 10).sum() >= 5 and (ws <= 5).sum() >= 5
    wf = G.g(a, 'm_water_fraction')[-1]
    Y = float(G.g(a, 'oil_emulsion_water_fraction_max'))
    assert (wf == Y).sum() >= 5 and ((wf < Y) & (wf > 0)).sum() >= 5
    assert np.nanmax(G.g(a, 'p_viscosity')[-1] / G.g(a, 'p_viscosity')[0]) > 100
    assert (G.g('d', 'e_mass_evaporated') == 0).all() and (G.g('d', 's0_z') == 0).any()        # older than 24 h: no evaporation
    assert float(np.nanmax(G.g('c', 'm_water_fraction'))) < float(G.g('c', 'oil_emulsion_water_fraction_max'))     # SINTEF override
    assert G.g('b', 's0_present')[0].sum() < G.g('b', 's0_present')[-1].sum()                # continuous release
    for c in W.Golden.CASES:
        for k in W.REC:
            assert str(G.g(c, 'dtype_' + k)) == 'float64'


def test_row_sum_is_numpys():
    rng = np.random.default_rng(5)
    for m in (1, 2, 7, 8, 9, 15, 16, 17, 31, 32):
        a = rng.uniform(0, 1, (50, m)) * 10.0**rng.integers(-8, 8, (50, m))
        assert np.array_equal(W.row_sums(a), a.sum(axis=1)), m


def test_one_entry_max_water_fraction_is_its_value():
    """The reference stops on this form (it subtracts two lists, openoil.py:879-883); the table takes the single value, which is what
    its two masks would leave."""
    case, s = 'c', G.steps('c') - 1
    oil = dict(G.oil(case), max_water_fraction={'temperatures': [5.0], 'max_water_fraction': [0.4]})
    ids, env, z, age = G.inputs(case, s)
    front = _sub(G.state(case, s, 'e'), ids)
    out, _, red, _ = W.step(oil, G.rho_w(case), ['emulsification'], G.dt(case), env, z, age, front, G.mc(case, s, 'e')[ids])
    assert red['min_ydiff'] == oil['emulsion_water_fraction_max'] - float(np.float32(0.4))
    assert out['water_fraction'].max() == np.float32(0.4) and (out['water_fraction'] == np.float32(0.4)).sum() >= 5
