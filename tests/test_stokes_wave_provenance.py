"""CPU: where the Stokes profile takes its wave height and period from (OceanDrift._stokes_wave_provenance,
physics_methods.py:893-943, :809-814) -- decided on the host from the movers' reduction.  The reduction's wind maximum is
advect_wind's, over the elements within wind_drift_depth of the surface, and -inf when there is none; the reference forms height
and period from the wind of EVERY element.  The decision is the same for one process and for a sharded run, whose ranks combine
the all-element maximum."""
import numpy as np
import pytest

NINF = -np.inf


class StubParticles:
    """The reductions of one rank: `local_all` is this rank's wind maximum over all of its elements"""

    def __init__(self, local_all):
        self.local_all, self.calls = local_all, []

    def _raw(self, wdd):
        raw = np.full(16, NINF)
        raw[0], raw[11], raw[9] = 4, 4 if wdd >= 1e30 else 0, self.local_all if wdd >= 1e30 else NINF
        return raw

    def reduce_scalars(self, wdd=0.1):
        from opendrift_amd.device import Particles
        self.calls.append(('reduce_scalars', wdd))
        return Particles.reduction_dict(self._raw(wdd))

    def reduce_local(self, wdd=0.1, relative_wind=False):
        self.calls.append(('reduce_local', wdd))
        return self._raw(wdd)

    def reduce_install(self, g):
        self.calls.append(('reduce_install', np.array(g, copy=True)))

    def reduce_global(self, combine, wdd=0.1, relative_wind=False):
        self.calls.append(('reduce_global', wdd))
        return combine(self._raw(wdd))

    @staticmethod
    def reduction_dict(raw):
        from opendrift_amd.device import Particles
        return Particles.reduction_dict(raw)


def model(world, local_all, other_rank_all=NINF, step_red=None, wind=True):
    from opendrift_amd.oceandrift import OceanDrift
    o = OceanDrift(loglevel=50)
    if not wind:
        o.required_variables.pop('x_wind'), o.required_variables.pop('y_wind')
    o._world, o._timing_collectives, o._step_red = world, 0, step_red
    o.P = StubParticles(local_all)

    def combine(raw):      # (the maxima of two ranks)
        g = np.array(raw, copy=True)
        g[9] = max(g[9], other_rank_all)
        return g
    o._combine = lambda: combine
    return o


def reduction(hs_max=NINF, wind_surface=NINF, n_surface=0):
    return dict(hs_max=hs_max, wind_speed_max=wind_surface, n_surface=n_surface, stokes_sum_max=0.04)


@pytest.mark.parametrize('world', [1, 2])
def test_surface_elements_decide_as_before(world):
    o = model(world, 6.0)
    assert o._stokes_wave_provenance(reduction(hs_max=1.2, wind_surface=6.0, n_surface=3)) == (0, 1)
    assert o._stokes_wave_provenance(reduction(hs_max=0.0, wind_surface=6.0, n_surface=3)) == (1, 1)
    assert o._stokes_wave_provenance(reduction(hs_max=0.0, wind_surface=0.0, n_surface=3)) == (2, 1)      # calm: Hs = 1, omega = 5
    assert o.P.calls == []                                                   # no further reduction


@pytest.mark.parametrize('world', [1, 2])
def test_submerged_population_with_a_given_wave_height_needs_no_further_reduction(world):
    o = model(world, 6.0)
    assert o._stokes_wave_provenance(reduction(hs_max=1.2)) == (0, 1)        # Tp from the wind, not 8 s
    assert o.P.calls == []


def test_submerged_population_takes_the_wave_height_from_the_wind_of_every_element():
    o = model(1, 6.0)
    assert o._stokes_wave_provenance(reduction(hs_max=0.0)) == (1, 1)
    assert o.P.calls == [('reduce_scalars', 1e30)]
    assert model(1, 0.0)._stokes_wave_provenance(reduction(hs_max=0.0)) == (2, 1)      # calm everywhere: Hs = 1 m


@pytest.mark.parametrize('local_all,other', [(6.0, NINF), (0.0, 6.0), (NINF, 6.0)])
def test_sharded_run_decides_like_one_process(local_all, other):
    """Whichever rank holds the windy elements (or any element at all): every rank gets the mode one process would get, and the
    step's installed reduction is put back."""
    step_red = np.arange(16.0)
    o = model(2, local_all, other, step_red=step_red)
    assert o._stokes_wave_provenance(reduction(hs_max=0.0)) == (1, 1)
    assert [c[0] for c in o.P.calls] == ['reduce_local', 'reduce_install'] and np.array_equal(o.P.calls[1][1], step_red)
    o = model(2, local_all, other)                                           # no step collective: the mover's reduction again
    assert o._stokes_wave_provenance(reduction(hs_max=0.0)) == (1, 1)
    assert [c[0] for c in o.P.calls] == ['reduce_local', 'reduce_global']
    assert model(2, 0.0, 0.0, step_red=step_red)._stokes_wave_provenance(reduction(hs_max=0.0)) == (2, 1)


def test_wind_that_is_not_sampled_gives_the_default_period():
    o = model(1, NINF, wind=False)
    assert o._stokes_wave_provenance(reduction(hs_max=1.2)) == (0, 2)        # Tp = 8 s
    assert o._stokes_wave_provenance(reduction(hs_max=0.0)) == (2, 2) and o.P.calls == []
