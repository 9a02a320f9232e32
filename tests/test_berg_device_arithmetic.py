"""CPU: the device arithmetic of OpenBerg.roll_over and OpenBerg.advect_iceberg (opendrift_amd/csrc/odr_berg.hip.h, compiled for
the host by tests/berg_host.py: the per-element functions, the fixed-order sums and the control flow of the RK45 solve) against
the values the reference itself computed (golden c28, tools/gen_golden_openberg.py): every stored step, from the golden's
recorded inputs.

Bit for bit: sail, draft, length and width after roll_over, the grounded flags, `moving` after grounding and degrounding, and V0
(no sum over elements enters it).  Equal: attempts and rejected attempts of every step (198 - 208 attempts, 37 - 45 of them
rejected).  The solved velocities differ from SciPy's only through the order of the sums (the error norm here, np.dot through BLAS
in rk_step and the norm there) and the dense-output value SciPy returns at the end point: MEASURED max |host - golden| over the
eight steps 8.43e-12 m/s (V0: 0).  Bound: 4 x the measured maximum.  A correct restatement stays under 1e-9 m/s: beyond that the
bound is not to be widened, the restatement is wrong.

Positions: every step's move replayed from the golden's own start positions with the host velocities through the host build of the
device geodesic (tests/geod_host.cpp): MEASURED max |host - golden| over the eight steps 8.99e-13 deg (longitude; latitude
2.42e-13 deg).  The bound of one step is 4 x that; a run of STEPS steps is held to STEPS times the bound of one step
(tests/test_gpu_openberg.py)."""
import numpy as np
import pytest

from conftest import golden

import berg_host

STEPS = 8
VELOCITY_MEASURED = 8.43e-12          # m/s
VELOCITY_BOUND = 4 * VELOCITY_MEASURED
assert VELOCITY_BOUND < 1e-9
POSITION_MEASURED_DEG = 8.99e-13      # one step
POSITION_STEP_BOUND_DEG = 4 * POSITION_MEASURED_DEG
DIMS = ('sail', 'draft', 'length', 'width')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def golden_step(g, k):
    """The elements present in step k: the recorded inputs and the reference's outputs"""
    m = g['grounded'][k] >= 0
    d = {name: g[name][k][m] for name in g.files if g[name].shape == g['grounded'].shape}
    d['env'] = {name: d['env_' + name] for name in berg_host.ENV}
    d['kw'] = dict(wave_from_direction=float(g['c_sea_surface_wave_from_direction']), sea_ice_thickness=float(g['c_sea_ice_thickness']),
                   lat_is_float32=k == 0)       # (elements.lat is a float32 array until the first update_positions)
    d['dt'] = float(g['dt'])
    norms = g['error_norms'][k]
    d['attempts'], d['rejected'] = int(np.isfinite(norms).sum()), int((norms >= 1).sum())
    return d


def records(g, n, first_step=1):
    """n element records of the steps from `first_step` on, one after the other (float64 latitudes from step 1 on): inputs of
    roll_over and advect_iceberg as arrays of length n"""
    parts = [golden_step(g, k) for k in range(first_step, STEPS)]
    cat = lambda name: np.concatenate([p[name] for p in parts])[:n]      # noqa: E731
    d = {name: cat(name) for name in [x + '_before' for x in DIMS] + ['adv_lat', 'moving_before']}
    d['env'] = {name: cat('env_' + name) for name in berg_host.ENV}
    assert len(d['adv_lat']) == n
    return d


def test_golden_covers_what_the_tests_rely_on():
    g = golden('c28_openberg.npz')
    norms = g['error_norms']
    assert norms.shape[0] == STEPS and ((norms >= 1).sum(axis=1) > 0).sum() >= 2
    assert not (np.abs(norms[np.isfinite(norms)] - 1) < 1e-6).any()
    assert np.array_equal(np.isfinite(norms).sum(axis=1), (g['nfev'] - 2) // 6)
    present = g['grounded'] >= 0
    n = present.shape[1]
    assert (g['grounded'] == 1).any(axis=0).sum() >= 0.05 * n
    assert ((g['moving_before'] == 0) & (g['moving_after'] == 1)).any(axis=0).sum() >= 5
    rolled = present & (g['width_after'] != np.minimum(g['length_before'], g['width_before']))
    assert rolled[0].sum() >= 0.1 * n and (~rolled.any(axis=0)).sum() >= 0.1 * n
    a = g['env_sea_ice_area_fraction']
    for cls in (a <= np.float32(0.15), (a > np.float32(0.15)) & (a < np.float32(0.9)), a >= np.float32(0.9)):
        assert (cls & present).sum(axis=1).max() >= 0.1 * n
    assert g['Vx'].dtype == np.float64 and g['sail_after'].dtype == np.float32 and g['env_x_wind'].dtype == np.float32


@pytest.mark.parametrize('k', range(STEPS))
def test_host_build_of_the_device_functions_reproduces_the_reference(k):
    d = golden_step(golden('c28_openberg.npz'), k)
    dims = berg_host.roll_over(*(d[n + '_before'] for n in DIMS))
    for a, n in zip(dims, DIMS):
        assert np.array_equal(bits(a), bits(d[n + '_after'])), n
    r = berg_host.advect(d['env'], d['adv_lat'], *dims, d['moving_before'], d['dt'], **d['kw'])
    assert r['status'] == 0, berg_host.SOLVE[r['status']]
    assert np.array_equal(r['grounded'], d['grounded']) and np.array_equal(r['moving'], d['moving_after'])
    assert np.array_equal(r['V0x'], d['V0x']) and np.array_equal(r['V0y'], d['V0y'])
    grounded = d['grounded'] == 1
    dv = max(np.abs(r['Vx'] - np.where(grounded, 0, d['Vx'])).max(), np.abs(r['Vy'] - np.where(grounded, 0, d['Vy'])).max())
    print('step %d: %d attempts, %d rejected (reference %d, %d); max |V - reference| %.3g m/s; %d grounded'
          % (k, r['attempts'], r['rejected'], d['attempts'], d['rejected'], dv, grounded.sum()))
    assert (r['attempts'], r['rejected']) == (d['attempts'], d['rejected'])
    assert dv <= VELOCITY_BOUND
    assert (r['Vx'][grounded] == 0).all() and (r['Vy'][grounded] == 0).all()
    assert np.array_equal(r['iceb_x_velocity'], r['Vx'].astype(np.float32)) and np.array_equal(r['iceb_y_velocity'], r['Vy'].astype(np.float32))


@pytest.mark.parametrize('k', range(STEPS))
def test_positions_of_one_step_from_the_host_velocities(k):
    """update_positions of step k replayed on the CPU: the golden's start positions moved by the host build's velocities along
    the host build of the device geodesic, against the reference's positions after the step."""
    g = golden('c28_openberg.npz')
    d = golden_step(g, k)
    m = g['grounded'][k] >= 0
    dims = berg_host.roll_over(*(d[n + '_before'] for n in DIMS))
    r = berg_host.advect(d['env'], d['adv_lat'], *dims, d['moving_before'], d['dt'], **d['kw'])
    assert r['status'] == 0 and np.array_equal(g['lat'][k][m], d['adv_lat'])
    hd = r['moving'] * d['dt']
    lat, lon = berg_host.geod_move(d['adv_lat'], g['lon'][k][m], r['Vx'] * hd, r['Vy'] * hd)
    dlon, dlat = np.abs(lon - g['lon'][k + 1][m]).max(), np.abs(lat - g['lat'][k + 1][m]).max()
    print('step %d: max |position - reference| lon %.3g lat %.3g deg' % (k, dlon, dlat))
    assert dlon <= POSITION_STEP_BOUND_DEG and dlat <= POSITION_STEP_BOUND_DEG
    still = r['moving'] == 0
    assert still.any() == (d['grounded'] == 1).any() and np.array_equal(lon[still], g['lon'][k][m][still])


def test_numpy_float32_sine_and_cosine_are_restated_bit_for_bit():
    """The reference's wave direction and the Coriolis parameter of a run's first step go through np.sin / np.cos of float32
    arrays, which are not correctly rounded: berg_sincosf_numpy restates NumPy's routine, on two million arguments.  The routine
    restated is the one NumPy dispatches to on a CPU with fused multiply-add (x86 AVX2 + FMA3 or AVX-512), where the golden was
    made; without FMA NumPy's float32 sine takes another route, the reference itself gives other bits, and this test and the
    golden's first step do not hold."""
    x = np.random.default_rng(1).uniform(-7, 7, 2000000).astype(np.float32)
    s, c = berg_host.sincosf(x)
    assert np.array_equal(bits(s), bits(np.sin(x))) and np.array_equal(bits(c), bits(np.cos(x)))


def test_float64_sine_of_the_latitude_is_within_an_ulp():
    x = np.linspace(-np.pi / 2, np.pi / 2, 4001)
    s = np.array([berg_host.sin(v) for v in x])
    assert (np.abs(s - np.sin(x)) <= np.spacing(np.abs(np.sin(x)))).all()


def test_sums_do_not_depend_on_how_often_they_are_formed_but_on_the_workgroup_size():
    """The same input twice: the same bits.  Another workgroup size orders the sums differently: the attempt counts stay, the
    velocities move by rounding only -- the sum really is what orders the bits."""
    d = records(golden('c28_openberg.npz'), 513)
    dims = berg_host.roll_over(*(d[n + '_before'] for n in DIMS))
    run = lambda **kw: berg_host.advect(d['env'], d['adv_lat'], *dims, d['moving_before'], 3600.0, wave_from_direction=200.0,      # noqa: E731
                                        sea_ice_thickness=1.0, **kw)
    a, b, c = run(), run(), run(block=64)
    assert a['status'] == 0 and a['attempts'] > 50 and a['rejected'] > 0
    assert np.array_equal(a['Vx'], b['Vx']) and np.array_equal(a['Vy'], b['Vy']) and a['attempts'] == b['attempts']
    assert c['attempts'] == a['attempts'] and np.abs(c['Vx'] - a['Vx']).max() < 1e-9


def test_roll_over_orders_and_splits_every_element():
    """A stable berg given with width > length: the two are swapped and the thickness is split again, without a roll."""
    s, d, L, W = berg_host.roll_over([10.0], [90.0], [100.0], [150.0])
    assert L[0] == 150 and W[0] == 100
    assert d[0] == np.float32(100.0) * np.float32(900 / 1027) and s[0] == np.float32(100.0) - d[0]
    s, d, L, W = berg_host.roll_over([10.0], [90.0], [100.0], [30.0])       # W / H = 0.3 < 0.807: rolls
    assert L[0] == 100 and W[0] == 100 and np.float32(s[0] + d[0]) == 30


def test_solver_failures_are_reported_and_the_solve_ends():
    n = 4
    env = {k: np.zeros(n, np.float32) for k in berg_host.ENV}
    env['x_wind'][:] = np.nan
    r = berg_host.advect(env, np.full(n, 75.0), [10.0] * n, [90.0] * n, [100.0] * n, [30.0] * n, np.ones(n, np.int32), 3600.0)
    assert berg_host.SOLVE[r['status']] == 'error norm not finite' and r['attempts'] <= 1
