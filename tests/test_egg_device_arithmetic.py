"""CPU: the device arithmetic of PelagicEggDrift.update_terminal_velocity (opendrift_amd/csrc/odr_egg.hip.h, compiled for the
host by tests/egg_host.py) against the values the reference itself computed (golden c25, tools/gen_golden_pelagicegg.py):
(T, S, diameter, neutral_buoyancy_salinity) -> terminal_velocity of every element in every step of both cases.

The choice of the branch is identical for every element and the Stokes branch is bit for bit (it uses + - * / sqrt only).
The high-Reynolds branch goes through an exp and three fractional powers that NumPy evaluates with float32 routines that are
not correctly rounded (measured against the float64 value rounded once: np.exp 2 ulp, np.power 1 ulp), where the device
evaluates them in float64 and rounds once.  MEASURED largest distance to the golden: 5 ulp (2738 values, 1697 of them in the
high-Reynolds branch; 0 ulp for 67 % of those).  Bound: 5 + 2 = 7 ulp -- one each for a libm whose exp and pow differ from
this one in the last place."""
import numpy as np
import pytest

from conftest import golden

import egg_host

HIGH_RE_MAX_ULP = 5 + 2


def ulp_distance(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (np.signbit(a) == np.signbit(b)).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def golden_inputs(g, prefix):
    """every (step, element) the reference evaluated: T, S, diameter, salinity, terminal velocity, regime"""
    tv = g[prefix + 'terminal_velocity']
    m = np.isfinite(tv)
    d = np.broadcast_to(g[prefix + 'diameter'], tv.shape)[m]
    s = np.broadcast_to(g[prefix + 'neutral_buoyancy_salinity'], tv.shape)[m]
    return g[prefix + 'env_T'][m], g[prefix + 'env_S'][m], d, s, tv[m], g[prefix + 'high_re'][m]


@pytest.mark.parametrize('prefix', ['', 'k_'], ids=['celsius', 'kelvin_reader'])
def test_host_build_of_the_device_function_reproduces_the_reference(prefix):
    T, S, d, s, want, want_high = golden_inputs(golden('c25_pelagicegg.npz'), prefix)
    assert T.dtype == np.float32 and want.dtype == np.float32 and len(want) > 300
    assert 0.1 <= want_high.mean() <= 0.9          # both branches are covered by the input
    got, high = egg_host.terminal_velocity(T, S, d, s)
    assert np.array_equal(high, want_high)
    stokes = ~high
    assert np.array_equal(got[stokes].view(np.uint32), want[stokes].view(np.uint32))
    dist = ulp_distance(got[high], want[high])
    print('high-Reynolds branch: %d values, largest distance %d ulp, histogram %s' % (high.sum(), dist.max(), np.bincount(dist)))
    assert dist.max() <= HIGH_RE_MAX_ULP
    assert (got[stokes & (want < 0)] < 0).any() and (got[high] > 0).all()     # sinking eggs exist and take Stokes' law


def test_only_the_selected_branch_is_stored():
    """An egg heavier than the water: the reference's unused high-Reynolds value is NaN (a negative base under a fractional
    power), the stored value is the finite Stokes velocity.  Neutral buoyancy: exactly 0."""
    w, high = egg_host.terminal_velocity([8.0, 8.0], [30.0, 33.0], [0.004, 0.004], [35.0, 33.0])
    assert not high.any() and np.isfinite(w).all() and w[0] < 0 and w[1] == 0
