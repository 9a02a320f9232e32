"""CPU: the device arithmetic of LarvalFish.update_fish_larvae and LarvalFish.larvae_vertical_migration
(opendrift_amd/csrc/odr_larval.hip.h, compiled for the host by tests/larval_host.py) against the values the reference itself
computed (golden c27, tools/gen_golden_larvalfish.py): every stored step, one step at a time, from the golden's "before"
arrays to its "after" arrays.

The set of elements that hatch is identical; an egg's weight and length, a larva's stage_fraction and an egg's z are bit for bit
(nothing is stored there).  Everything else goes through exp, log, log10 and power, which NumPy evaluates with float32
routines that are not correctly rounded (measured against the float64 value rounded once: log 3 ulp, log10 2, exp 2, power 1)
where the device evaluates them in float64 and rounds once.  MEASURED largest distances to the golden over its nine steps
(about 1 000 eggs and 1 600 larvae): stage_fraction 0 ulp, weight 2 ulp, length 5 ulp, the swimming displacement 7 ulp (in ulp of
the float32 displacement: the sum with z is a float64 one).  Bounds: measured + 2 ulp -- one each for a libm whose exp / log
and pow differ from this one in the last place."""
import numpy as np
import pytest

from conftest import golden

import larval_host

STAGE_MEASURED_ULP, WEIGHT_MEASURED_ULP, LENGTH_MEASURED_ULP, DISPLACEMENT_MEASURED_ULP = 0, 2, 5, 7
STAGE_MAX_ULP = STAGE_MEASURED_ULP + 2
WEIGHT_MAX_ULP = WEIGHT_MEASURED_ULP + 2
LENGTH_MAX_ULP = LENGTH_MEASURED_ULP + 2
DISPLACEMENT_MAX_ULP = DISPLACEMENT_MEASURED_ULP + 2
# z and the displacement are summed in float64, once by the reference and once here: two roundings of at most half a float64 ulp of
# |z| < 64 m (2 x 2**-48 m) against the float32 ulp of a displacement of at least 0.02 m (2**-29 m): at most 2**-18 of such an ulp
DISPLACEMENT_SUM_SLACK_ULP = 2.0 ** -17
STEPS = 9


def ulp_distance(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (np.signbit(a) == np.signbit(b)).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def golden_step(g, k):
    """The elements present in step k: the inputs and the reference's outputs of both methods"""
    m = g['hatched_before'][k] >= 0
    d = {name: g[name][k][m] for name in ('env_T', 'stage_fraction_before', 'stage_fraction_after', 'hatched_before', 'hatched_after',
                                          'weight_before', 'weight_after', 'length_before', 'length_after', 'mig_z_before',
                                          'mig_z_after', 'mig_length', 'mig_hatched')}
    d['direction'], d['f'], d['dt'] = int(g['direction'][k]), float(g['fraction_of_timestep_swimming']), float(g['dt'])
    return d


def check_update(d, s, h, w, L):
    """(stage_fraction, hatched, weight, length) after update_fish_larvae against the reference; returns the largest distances"""
    assert np.array_equal(h, d['hatched_after'].astype(np.float32))                    # the same elements hatch
    egg, was_larva = h == 0, d['hatched_before'] == 1
    assert np.array_equal(bits(w[egg]), bits(d['weight_after'][egg])) and np.array_equal(bits(w[egg]), bits(d['weight_before'][egg]))
    assert np.array_equal(bits(L[egg]), bits(d['length_after'][egg])) and np.array_equal(bits(L[egg]), bits(d['length_before'][egg]))
    assert np.array_equal(bits(s[was_larva]), bits(d['stage_fraction_before'][was_larva]))
    assert np.isfinite(s).all() and np.isfinite(w).all() and np.isfinite(L).all()
    return (ulp_distance(s[~was_larva], d['stage_fraction_after'][~was_larva]).max(initial=0),
            ulp_distance(w[~egg], d['weight_after'][~egg]).max(initial=0), ulp_distance(L[~egg], d['length_after'][~egg]).max(initial=0))


def check_migration(d, z, displacement):
    """z after larvae_vertical_migration against the reference; `displacement`: the float32 value the code under test added
    (its ulp is the unit).  Returns the largest distance in those ulp"""
    want, larva = d['mig_z_after'], d['mig_hatched'] == 1
    assert np.array_equal(z[~larva], want[~larva]) and np.array_equal(z[~larva], d['mig_z_before'][~larva])     # eggs: untouched
    assert np.array_equal(z == 0, want == 0) and (z <= 0).all()                                                  # the same larvae are clamped
    free = larva & (want != 0)
    assert (np.abs(displacement[free]) >= 0.02).all() and (np.abs(want) <= 64).all()      # (what DISPLACEMENT_SUM_SLACK_ULP assumes)
    return (np.abs(z[free] - want[free]) / np.spacing(np.abs(displacement[free])).astype(np.float64)).max(initial=0)


def test_golden_covers_what_the_tests_rely_on():
    g = golden('c27_larvalfish.npz')
    d = g['direction']
    assert len(d) == STEPS and (d == -1).sum() >= 2 and (d == 1).sum() >= 2
    egg0 = g['seed_hatched'] == 0
    hatches = egg0 & (g['hatched_after'] == 1).any(axis=0)
    assert 0.2 <= hatches.sum() / egg0.sum() <= 0.8
    assert g['env_T'].dtype == np.float32 and g['weight_after'].dtype == np.float32 and g['mig_z_after'].dtype == np.float64
    assert float(g['fraction_of_timestep_swimming']) != 0.15      # (the configured value has to reach the kernel)


@pytest.mark.parametrize('k', range(STEPS))
def test_host_build_of_the_device_functions_reproduces_the_reference(k):
    d = golden_step(golden('c27_larvalfish.npz'), k)
    s, h, w, L, written = larval_host.update(d['env_T'], d['dt'], d['stage_fraction_before'], d['hatched_before'], d['weight_before'],
                                             d['length_before'])
    ds, dw, dl = check_update(d, s, h, w, L)
    # what was stored: stage_fraction of every egg, hatched of those that hatch, weight and length of every larva -- nothing else
    assert np.array_equal(written & 1 != 0, d['hatched_before'] == 0) and np.array_equal(written & 4 != 0, h == 1)
    assert np.array_equal(written & 2 != 0, (d['hatched_before'] == 0) & (h == 1))
    z, disp = larval_host.migrate(d['mig_hatched'], d['mig_length'], d['f'], d['dt'], d['direction'], d['mig_z_before'])
    dz = check_migration(d, z, disp)
    print('step %d (direction %+d): stage_fraction %d ulp, weight %d ulp, length %d ulp, displacement %.2f ulp; %d eggs, %d hatch, '
          '%d larvae, %d clamped at 0' % (k, d['direction'], ds, dw, dl, dz, (d['hatched_before'] == 0).sum(),
                                         ((d['hatched_before'] == 0) & (h == 1)).sum(), (h == 1).sum(), (z[d['mig_hatched'] == 1] == 0).sum()))
    assert ds <= STAGE_MAX_ULP and dw <= WEIGHT_MAX_ULP and dl <= LENGTH_MAX_ULP
    assert dz <= DISPLACEMENT_MAX_ULP + DISPLACEMENT_SUM_SLACK_ULP


def test_an_egg_goes_through_no_larval_formula():
    """An egg with weight 0, length 0 (5.289 / 0, log(0)) and a NaN in both: nothing but stage_fraction is stored, and z stays."""
    T = np.float32([8.0, 8.0, 8.0])
    s, h, w, L, written = larval_host.update(T, 600.0, [0.5, 0.5, 0.5], [0, 0, 0], [0.0, np.nan, 0.08], [0.0, np.nan, 0.0])
    assert (written == 1).all() and (h == 0).all() and (s > 0.5).all() and np.isfinite(s).all()
    assert w[0] == 0 and L[0] == 0 and np.isnan(w[1]) and np.isnan(L[1])
    z, disp = larval_host.migrate(h, L, 0.15, 600.0, 1, [-3.0, -3.0, -3.0])
    assert (z == -3.0).all() and (disp == 0).all()


def test_hatching_threshold_and_same_call_growth():
    """stage_fraction reaching exactly 1 hatches (>=); the new larva grows and gets its length in the same call."""
    days = np.float32(600.0 / 86400.0)
    duration = np.float32(np.exp(np.float64(np.float32(3.65) - np.float32(0.145) * np.float32(8.0))))
    step = days / duration
    below = np.float32(1.0) - step                      # float32 sum with `step` is exactly 1 or within an ulp of it
    s, h, w, L, written = larval_host.update(np.float32([8.0, 8.0]), 600.0, [below, 0.2], [0, 0], [0.08, 0.08], [0.0, 0.0])
    assert (s[0] >= 1) == (h[0] == 1) and h[1] == 0
    s, h, w, L, written = larval_host.update(np.float32([8.0]), 600.0, [1.0], [0], [0.08], [0.0])
    assert h[0] == 1 and written[0] == 7 and w[0] > np.float32(0.08) and 4.5 < L[0] < 5.5


def test_surface_clamp_and_direction():
    z, disp = larval_host.migrate([1, 1, 1], [10.0, 10.0, 10.0], 0.15, 600.0, 1, [-0.01, -5.0, 0.0])
    assert z[0] == 0 and z[2] == 0 and -5.0 < z[1] < -4.0 and (disp > 0).all()
    zd, dd = larval_host.migrate([1, 1, 1], [10.0, 10.0, 10.0], 0.15, 600.0, -1, [-0.01, -5.0, 0.0])
    assert np.array_equal(dd, -disp) and (zd < [-0.01, -5.0, 0.0]).all()
