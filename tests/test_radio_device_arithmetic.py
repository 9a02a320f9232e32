"""CPU: the per-element code of csrc/odr_radio.hip.h, compiled for the host (tests/radio_host.cpp), replays every step of the golden
C30 (tools/gen_golden_radionuclides.py: the reference's own RadionuclideDrift) with the reference's recorded draws scattered to
their elements.  specie, moving and the transformation counters must be identical for every element and step, z of the teleported
elements and the float32 diameter too.  A species decision that flips because u1 lies within an ulp of psum would be reported by
element (the generator refuses a golden in which one is closer than 4 ulp).

terminal_velocity: the reference's W is float64 in its last product (the default `density` seeds a float64 array; DESIGN.md section
7g), the device's chain is float32 throughout.  The host build's largest relative deviation from the reference's value rounded to
float32, measured on C30, is 1.192e-7 (one float32 ulp); the bound is four times that."""
import numpy as np
import pytest

import radio_host as R

TV_MEASURED = 1.192e-7
TV_BOUND = 4 * TV_MEASURED


@pytest.fixture(scope='module')
def golden():
    return R.Golden()


def _report(name, got, exp, inp):
    bad = np.where(got != exp)[0]
    return '%s differs for %d elements, first: %s' % (name, len(bad), [
        (int(i), 'specie in %d' % inp['specie'][i], 'got %r' % got[i], 'expected %r' % exp[i]) for i in bad[:5]])


@pytest.mark.parametrize('case', ['a', 'b'])
def test_speciation_replays_the_reference(golden, case):
    m, dt = golden.setup(case), golden.dt(case)
    total = 0
    for s in range(golden.steps(case)):
        inp, draws, exp = golden.speciation_step(case, s)
        out = R.speciation(m, dt, **inp, **draws)
        assert out['bad'] == 0
        for k in ('specie', 'moving'):
            assert np.array_equal(out[k], exp[k]), 'step %d: %s (|u1 - psum| of those elements: %s)' % (
                s, _report(k, out[k], exp[k], inp), np.abs(draws['u1'] - exp['psum'])[out[k] != exp[k]][:5])
        assert np.array_equal(out['counts'], exp['counts']), 'step %d' % s
        assert out['diameter'].dtype == np.float32 and np.array_equal(out['diameter'], exp['diameter']), _report('diameter', out['diameter'], exp['diameter'], inp)
        z = out['z']
        if exp['z_f32']:      # the reference's z array is still the float32 one of the seeding: what it stores is rounded to it
            z = np.where(z != inp['z'], z.astype(np.float32).astype(np.float64), z)
        assert np.array_equal(z, exp['z']), 'step %d: %s' % (s, _report('z', z, exp['z'], inp))
        total += int(out['counts'].sum())
    assert total > 1000


@pytest.mark.parametrize('case', ['a', 'b'])
def test_probabilities_agree_to_the_exponential(golden, case):
    # psum differs from NumPy's only through exp (libm's here): a few ulp of the exponential, i.e. of 1, relative to psum
    m, dt = golden.setup(case), golden.dt(case)
    for s in range(golden.steps(case)):
        inp, draws, exp = golden.speciation_step(case, s)
        p, psum = R.probabilities(m, dt, inp['specie'], inp['z'], inp['sal'], inp['depth'], inp['conc3'])
        assert np.all(np.abs(psum - exp['psum']) <= 4 * np.finfo(np.float64).eps)
        assert np.all(p[:, m['nspecies']:] == 0)


@pytest.mark.parametrize('case', ['a', 'b'])
def test_resuspension_replays_the_reference(golden, case):
    m = golden.setup(case)
    resuspended = settled = 0
    for s in range(golden.steps(case)):
        inp, draws, exp = golden.resuspension_step(case, s)
        out = R.resuspend(m, **inp, **draws)
        assert out['bad'] == 0
        for k in ('specie', 'moving', 'diameter', 'z'):
            assert np.array_equal(out[k], exp[k]), 'step %d: %s' % (s, _report(k, out[k], exp[k], inp))
        assert np.array_equal(out['counts'], exp['counts']), 'step %d' % s
        resuspended += int(((inp['moving'] == 0) & (out['moving'] == 1)).sum())
        settled += int((out['moving'] == 0).sum())
    assert resuspended > 100 and settled > 100


@pytest.mark.parametrize('case', ['a', 'b'])
def test_terminal_velocity_within_four_times_the_measured_deviation(golden, case):
    worst = 0.0
    for s in range(golden.steps(case)):
        inp, tv = golden.terminal_velocity_step(case, s)
        w = R.terminal_velocity(**inp)
        still = inp['moving'] == 0
        assert (w[still] == 0).all() and (tv[still] == 0).all()
        dissolved = inp['diameter'] == 0
        assert (w[dissolved] == 0).all() and (tv[dissolved] == 0).all()
        nz = tv != 0
        rel = np.abs(w[nz].astype(np.float64) - tv[nz]) / np.abs(tv[nz])
        worst = max(worst, float(rel.max()))
    print('largest relative deviation of the terminal velocity, case %s: %.4g' % (case, worst))
    assert worst <= TV_BOUND


def test_target_is_clamped_to_the_last_species_with_a_probability():
    # u2 above every cumulative value (the reference stores the species number nspecies and fails on it a step later): the last
    # species with p > 0.  One LMM element of the three-species setup far above the sea bed: only LMM -> particle has a rate
    m = dict(R.golden_setup(np.load(R.GOLDEN), 'a'))
    out = R.speciation(m, 21600., specie=[0.], diameter=[0.], moving=[1], z=[-5.], sal=[30.], depth=[30.], conc3=[2e-3],
                       u1=[0.], u2=[np.nextafter(1., 2.)], diameter_noise=[0.], depth_noise=[0.])
    assert out['specie'][0] == 1 and out['counts'][0, 1] == 1 and out['counts'].sum() == 1


def test_species_outside_the_table_is_counted_and_left_alone():
    m = dict(R.golden_setup(np.load(R.GOLDEN), 'a'))
    kw = dict(diameter=[1e-5, 1e-5], moving=[1, 1], z=[-5., -5.], depth=[30., 30.])
    out = R.speciation(m, 21600., specie=[7., -1.], sal=[30., 30.], conc3=[2e-3, 2e-3], u1=[0., 0.], u2=[.5, .5], diameter_noise=[0., 0.],
                       depth_noise=[0., 0.], **kw)
    assert out['bad'] == 2 and out['counts'].sum() == 0 and list(out['specie']) == [7., -1.] and list(out['z']) == [-5., -5.]
    out = R.resuspend(m, specie=[9., -3.], u=[1., 1.], v=[0., 0.], diameter_noise=[0., 0.], depth_noise=[0., 0.], **kw)
    assert out['bad'] == 2 and out['counts'].sum() == 0 and list(out['moving']) == [1, 1]


def test_salinity_intervals_follow_searchsorted():
    # np.searchsorted([0, 1, 10, 20], S) - 1 with the index -1 of S <= 0 taken from the end, as the reference's fancy index does
    m = dict(R.golden_setup(np.load(R.GOLDEN), 'b'))
    S = np.array([-1., 0., 1e-6, 1., np.nextafter(np.float32(1), np.float32(2)), 10., 10.5, 20., 20.5, 35., np.nan], np.float32)
    sali = np.searchsorted([0, 1, 10, 20], S) - 1
    n = len(S)
    cat = 0      # LMMcation
    p, psum = R.probabilities(m, 43200., np.full(n, cat, np.float32), np.full(n, -5.), S, np.full(n, 30., np.float32), np.full(n, 1e-3, np.float32))
    for k in range(n):
        row = m['rates'][sali[k], cat]
        assert np.allclose(p[k, :len(row)], 1 - np.exp(-row * 43200.), rtol=1e-14, atol=0), (S[k], sali[k])
