"""The sixteen global reductions over the active elements (k_reduce<EXT>, k_red_finish over the per-wave records of the step
launch, odr_reduce_install) and the cache that serves them (odr_i_reduce) against NumPy (tests/reduction_ref.py, written
from the reference project's lines and checked by hand in tests/test_reduction_reference.py).

Values are compared with `==` (so -inf equals -inf and -0.0 equals 0.0; no bit patterns: the sign of a zero maximum is not
defined) and the tolerance is NONE: maxima and counts are exact, every per-element expression is one chain of correctly
rounded IEEE operations that NumPy reproduces, the counts are far below 2^53.

  a  every slot at the wave and workgroup edges, both dictionaries
  b  the extreme at the indices where k_reduce's launch geometry branches (second trip, `u = 1` half, tail lanes)
  c  what must not count: deactivated elements, NaN, signed zeros, absent variables, the wind drift depth edges
  d  every entry point that changes what the reductions read must void the cache (one case each)
  e  a reduction formed by the step launch holds signs, not maxima: whoever needs values reduces again
  f  k_red_finish beyond one trip of its grid
  g  rows of two particle sets combine to the row of their union; installed rows stay until unpinned

k_reduce<true> is read through reduce_local / reduce_scalars; k_reduce<false> (the movers' own pass, without the lon / lat /
z extremes) through reduce_cached right after a mover."""
import numpy as np
import pytest

import reduction_ref as R
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context, Particles
from reduction_ref import HD, HS, MLD, SX, SY, TP, U, V, XW, YW

pytestmark = pytest.mark.gpu

INF = np.inf
f32 = np.float32
LAND, DEPTH, W = 'land_binary_mask', 'sea_floor_depth_below_sea_level', 'upward_sea_water_velocity'
WDDS = (0.1, 2.0, 0.0, -0.1, 1e30)
STOKES = dict(profile=0, hs_mode=2, tp_mode=2)      # monochromatic, scalar wave height and period: needs no Hs / Tp / wind


# ------------------------------------------------------------------------------------------------ helpers
def _random_state(n, seed, names=R.ENV_NAMES):
    rng = np.random.default_rng(seed)
    z = np.where(rng.random(n) < 0.4, 0.0, -rng.uniform(0, 4, n))      # plenty within 0.1 m and within 2 m, some below both
    z = np.where(rng.random(n) < 0.05, rng.uniform(0, 1, n), z)        # and a few in the air
    env = {}
    for nm in names:
        a = rng.uniform(0, 30, n) if nm in (HD, HS, TP, MLD) else rng.normal(0, 3, n)
        env[nm] = a.astype(f32)
    return dict(lon=rng.uniform(-10, 20, n), lat=rng.uniform(55, 70, n), z=z, wdf=rng.uniform(0, 0.05, n).astype(f32),
                status=np.zeros(n, np.int32), env=env)


def _make(ctx, s, cap=None):
    n = len(s['lon'])
    P = ctx.particles(max(cap or n, 1))
    if n:
        P.append(s['lon'], s['lat'], z=s['z'], wind_drift_factor=s['wdf'], id=s.get('ID'), moving=s.get('moving'),
                 terminal_velocity=s.get('tv'))
        for nm, a in s['env'].items():
            P.env_upload(nm, a)
        for code in np.unique(s['status'][s['status'] != 0]):
            P.deactivate(s['status'] == code, int(code))
    return P


def _ref(s, wdd, rel):
    return R.raw16(s['lon'], s['lat'], s['z'], s['status'], s['wdf'], s['env'], wdd, rel)


def _assert_raw(got, want, what):
    bad = [(R.KEYS[k], got[k], want[k]) for k in range(16) if not got[k] == want[k]]
    assert not bad, (what, bad)


def _assert_dict(got, want, what):
    assert list(got) == R.KEYS, (what, list(got))
    bad = [(k, got[k], want[k]) for k in R.KEYS if not got[k] == want[k]]
    assert not bad, (what, bad)


def _check_extents_pass(P, s, wdd, rels=(False, True), refs=None):
    """k_reduce<true>: reduce_local for both relative_wind settings, reduce_scalars, and the two dictionaries.
    refs: {relative_wind: reference row} where the caller has them already (the large sets)."""
    refs = refs or {}
    for rel in rels:
        want = refs[rel] if rel in refs else _ref(s, wdd, rel)
        got = P.reduce_local(wdd, rel)
        _assert_raw(got, want, ('reduce_local', wdd, rel))
        _assert_dict(Particles.reduction_dict(got), R.as_dict(want), ('reduction_dict', wdd, rel))
    sc = P.reduce_scalars(wdd)
    _assert_dict(sc, R.as_dict(refs[False] if False in refs else _ref(s, wdd, False)), ('reduce_scalars', wdd))
    _assert_dict(Particles.reduction_dict(P.reduce_local(wdd, False)), sc, ('reduction_dict(reduce_local) against reduce_scalars', wdd))


def _check_movers_pass(P, s, wdd, rel, refresh=True, ref=None):
    """k_reduce<false>: what a mover reduced for itself, read back as it stands on the device.  The mover moves the
    elements: the host copy of the positions is refreshed."""
    env = s['env']
    P.reduce_unpin()           # (forget whatever reduce_local left: the mover must make its own pass)
    if XW in env and YW in env and (not rel or (U in env and V in env)):
        P.advect_wind(600.0, wind_drift_depth=wdd, relative_wind=rel)
        want = _ref(s, wdd, rel) if ref is None else ref.copy()
    elif HD in env:
        P.hdiffusion(600.0, step=0)
        want = _ref(s, 0.0, False)      # a mover without wind arguments reduces with (0, False)
    elif SX in env and SY in env:
        P.stokes_drift(600.0, **STOKES)
        want = _ref(s, 0.0, False)
    else:
        return
    got, st = P.reduce_cached()
    assert st == dict(valid=True, extents=False, partial=False, pinned=False), st
    want[1:7] = -INF                    # the movers' pass leaves the extremes out
    _assert_raw(got, want, ('mover pass', wdd, rel))
    if refresh:
        d = P.download()
        s['lon'], s['lat'] = d['lon'], d['lat']


def _check(P, s, wdds=WDDS):
    for wdd in wdds:
        _check_extents_pass(P, s, wdd)
        for rel in (False, True):
            _check_movers_pass(P, s, wdd, rel)


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 511, 513])
def test_every_slot_at_the_wave_and_workgroup_edges(n):
    ctx = Context(seed=1)
    s = _random_state(n, seed=n)
    P = _make(ctx, s)
    _check(P, s)
    P.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize('which', ['maxima', 'minima'])
def test_the_extreme_at_every_branch_of_the_launch_geometry(which):
    """k_reduce is grid-stride over at most 2048 workgroups of 256 and takes two elements per trip, the second at
    i0 + stride: with n = 2*2048*256 + 2*256 + 37 there is a second trip whose `u = 1` half runs past n for most lanes.  One
    element holds the extreme of every slot at once (for the minima: the least lon, lat and z, and values BELOW the
    constant in every other slot, so that every maximum comes from the rest); it visits each branch in turn."""
    G = 2048 * 256
    n = 2 * G + 2 * 256 + 37
    spots = [0, G - 1, G, 2 * G, 2 * G + 256, n - 1]
    ctx = Context(seed=1)
    s = dict(lon=np.full(n, 5.0), lat=np.full(n, 60.0), z=np.full(n, -1.0), wdf=np.full(n, 0.02, f32),
             status=np.zeros(n, np.int32), env={nm: np.full(n, 0.5 if nm in (U, V) else 1.0, f32) for nm in R.ENV_NAMES})
    P = _make(ctx, s)
    if which == 'maxima':
        one = dict(lon=6.0, lat=61.0, z=-0.5, wdf=0.04, env={nm: (-1.0 if nm in (U, V) else 2.0) for nm in R.ENV_NAMES})
    else:
        one = dict(lon=4.0, lat=59.0, z=-1.5, wdf=0.01, env={nm: (0.75 if nm in (U, V) else 0.5) for nm in R.ENV_NAMES})
    const = R.as_dict(_ref(s, 2.0, True))
    for i in spots:
        keep = dict(lon=s['lon'][i], lat=s['lat'][i], z=s['z'][i], wdf=s['wdf'][i], env={nm: a[i] for nm, a in s['env'].items()})
        for src in (one, keep):          # put the element in, check; put the constant back
            for q in ('lon', 'lat', 'z', 'wdf'):
                s[q][i] = src[q]
            for nm in R.ENV_NAMES:
                s['env'][nm][i] = src['env'][nm]
            P.upload(lon=s['lon'], lat=s['lat'], z=s['z'], wind_drift_factor=s['wdf'])
            for nm in R.ENV_NAMES:
                P.env_upload(nm, s['env'][nm])
            if src is keep:
                break
            refs = {rel: _ref(s, 2.0, rel) for rel in (False, True)}
            want = R.as_dict(refs[True])
            # the element does hold the extremes the case is about (a check of the test's own set-up)
            if which == 'maxima':
                assert all(want[k] > const[k] for k in R.KEYS if k not in ('n_active', 'n_surface', 'lon_min', 'lat_min', 'z_min')), i
            else:
                assert all(want[k] < const[k] for k in ('lon_min', 'lat_min', 'z_min')), i
                assert all(want[k] == const[k] for k in R.KEYS if k not in ('lon_min', 'lat_min', 'z_min')), i
            _check_extents_pass(P, s, 2.0, refs=refs)
            for rel in (False, True):
                _check_movers_pass(P, s, 2.0, rel, refresh=False, ref=refs[rel])      # (the positions are uploaded again for the next spot)
    P.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ c
def _with_outlier(n, i, seed):
    """a random set whose element i holds the extreme of every slot"""
    s = _random_state(n, seed)
    s['lon'][i], s['lat'][i], s['z'][i], s['wdf'][i] = 170.0, 89.0, 1.5, 0.9
    for nm in R.ENV_NAMES:
        s['env'][nm][i] = -500.0 if nm in (U, V) else 400.0
    return s


def test_a_deactivated_element_that_holds_every_extreme_does_not_count():
    ctx = Context(seed=1)
    n, i = 300, 137
    s = _with_outlier(n, i, seed=5)
    live = R.as_dict(_ref(s, 2.0, True))
    s['status'][i] = 7
    dead = R.as_dict(_ref(s, 2.0, True))
    assert all(live[k] > dead[k] for k in R.KEYS if not k.endswith('_min') and k != 'n_surface')   # (the set-up: it did hold them)
    P = _make(ctx, s)
    _check(P, s)                                  # deactivated, still in the arrays
    assert P.compact() == n - 1
    d = P.download()
    o = d['ID']                                   # the survivors in their new order (IDs are the original indices)
    assert i not in o and len(o) == n - 1
    s2 = dict(lon=d['lon'], lat=d['lat'], z=s['z'][o], wdf=s['wdf'][o], status=np.zeros(n - 1, np.int32),
              env={nm: a[o] for nm, a in s['env'].items()})
    assert np.array_equal(d['z'], s2['z'])
    _check(P, s2)                                 # and after the compaction
    P.close()
    ctx.close()


def test_nothing_active_and_nothing_at_all():
    """n_active 0, minima +inf, maxima -inf -- for a set whose elements are all deactivated and for an empty one"""
    ctx = Context(seed=1)
    s = _random_state(70, seed=2)
    s['status'][:] = 3
    P = _make(ctx, s)
    E = ctx.particles(16)
    want = np.array([0.0] + [-INF] * 10 + [0.0] + [-INF] * 4)
    for X, st in ((P, s), (E, None)):
        for wdd in (0.1, 0.0, 1e30):
            for rel in (False, True):
                _assert_raw(X.reduce_local(wdd, rel), want, (st is None, wdd, rel))
            sc = X.reduce_scalars(wdd)
            _assert_dict(sc, R.as_dict(want), (st is None, wdd))
            assert sc['n_active'] == 0 and sc['lon_min'] == sc['lat_min'] == sc['z_min'] == INF and sc['z_max'] == -INF
    _check(P, s, wdds=(0.1,))                      # (and the movers' own pass over the deactivated set)
    P.close()
    E.close()
    ctx.close()


def test_nan_is_ignored():
    """NaN in z and in every sampled variable, amid finite values: the device's maxima are those of the finite values (fmax),
    where ndarray.max() would hand NaN on -- pinned, not changed (tests/reduction_ref.py)."""
    ctx = Context(seed=1)
    n = 300
    s = _random_state(n, seed=9)
    rng = np.random.default_rng(10)
    for a in [s['z']] + list(s['env'].values()):
        a[rng.choice(n, 7, replace=False)] = np.nan
    s['z'][int(np.nanargmax(s['env'][XW]))] = np.nan          # the element with the strongest x_wind is nowhere
    s['env'][MLD][int(np.nanargmax(s['env'][MLD]))] = np.nan  # and the largest of a variable is the one that is missing
    P = _make(ctx, s)
    for wdd in (0.1, 2.0, 1e30):
        _check_extents_pass(P, s, wdd)
    for wdd in (0.1, 2.0):
        for rel in (False, True):
            _check_movers_pass(P, s, wdd, rel)
    P.close()
    ctx.close()


def test_signed_zeros_negative_maxima_and_a_stokes_sum_of_zero():
    ctx = Context(seed=1)
    n = 200
    rng = np.random.default_rng(3)
    pm0 = lambda dt: np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(dt)
    # -0.0 against 0.0 in every array: every maximum is a zero of either sign, every element is at the surface
    s = dict(lon=pm0(np.float64), lat=pm0(np.float64), z=pm0(np.float64), wdf=pm0(f32), status=np.zeros(n, np.int32),
             env={nm: pm0(f32) for nm in R.ENV_NAMES})
    P = _make(ctx, s)
    _check(P, s, wdds=(0.1, 0.0))
    got = P.reduce_local(0.1, True)
    assert got[0] == n and got[11] == n and all(got[k] == 0 for k in range(16) if k not in (0, 11))
    P.close()
    # all-negative D (the maximum is negative, the early-out `== 0` does not hold); sx = 1, sy = -1 everywhere (it does)
    s = _random_state(n, seed=4)
    s['env'][HD] = (-rng.uniform(0.5, 3, n)).astype(f32)
    s['env'][SX][:] = 1.0
    s['env'][SY][:] = -1.0
    P = _make(ctx, s)
    _check(P, s, wdds=(0.1,))
    got = P.reduce_local(0.1, False)
    assert got[7] == float(s['env'][HD].max()) < 0 and got[8] == 0
    P.close()
    ctx.close()


@pytest.mark.parametrize('wdd', [0.1, 2.0, -0.1])
def test_z_exactly_at_the_wind_drift_depth_and_z_in_the_air(wdd):
    """z == -|wdd| is at the surface with a factor of exactly 0; the next float64 below is not.  z > 0 keeps its own factor.
    The elements AT the depth carry the strongest wind, those a hair below a stronger one still, those in the air the
    largest factor: each slot tells which side its element fell on."""
    ctx = Context(seed=1)
    n = 260
    s = _random_state(n, seed=6)
    a = abs(wdd)
    s['z'][:] = -0.5 * a
    s['z'][0:40] = -a
    s['z'][40:80] = np.nextafter(-a, -INF)
    s['z'][80:120] = np.linspace(0.01, 3.0, 40)
    s['env'][XW][:] = 1.0
    s['env'][XW][0:40] = 20.0
    s['env'][XW][40:80] = 40.0
    s['wdf'][:] = 0.02
    s['wdf'][80:120] = 0.5
    want = R.as_dict(_ref(s, wdd, False))
    assert want['n_surface'] == n - 40 and want['wdf_surface_max'] == float(f32(0.5))
    assert f32(20.0) <= want['wind_speed_max'] < 40.0
    P = _make(ctx, s)
    _check(P, s, wdds=(wdd,))
    P.close()
    ctx.close()


ABSENT = {'no_wind': (XW, YW), 'only_x_wind': (YW,), 'only_y_wind': (XW,), 'wind_without_current': (U, V),
          'wind_with_one_current_component': (V,), 'only_stokes_x': (SY,), 'only_stokes_y': (SX,), 'no_hs': (HS,),
          'no_tp': (TP,), 'no_mld': (MLD,), 'no_hs_tp_mld': (HS, TP, MLD), 'no_diffusivity': (HD,),
          'only_diffusivity': tuple(nm for nm in R.ENV_NAMES if nm != HD), 'only_stokes': tuple(nm for nm in R.ENV_NAMES if nm not in (SX, SY)),
          'nothing_sampled': R.ENV_NAMES}


@pytest.mark.parametrize('case', sorted(ABSENT))
def test_absent_variables_leave_their_slots_empty(case):
    ctx = Context(seed=1)
    s = _random_state(300, seed=8, names=[nm for nm in R.ENV_NAMES if nm not in ABSENT[case]])
    want = _ref(s, 2.0, True)
    empty = {'no_wind': (9, 10, 14), 'only_x_wind': (9, 10, 14), 'only_y_wind': (9, 10, 14), 'only_stokes_x': (8,),
             'only_stokes_y': (8,), 'no_hs': (12,), 'no_tp': (13,), 'no_mld': (15,), 'no_hs_tp_mld': (12, 13, 15),
             'no_diffusivity': (7,), 'nothing_sampled': tuple(range(7, 11)) + (12, 13, 14, 15)}.get(case, ())
    assert all(want[k] == -INF for k in empty) and (not empty or 9 not in empty or want[11] == 0)    # (the reference agrees with the title)
    P = _make(ctx, s)
    _check(P, s, wdds=(0.1, 2.0))
    P.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ d
N_D = 300


def _calm(surface=100, z_deep=-5.0, wind=(0.0, 0.0), cur=None, wdf=0.02, n=N_D, **more):
    """calm wind, no Stokes drift, zero D, the first `surface` elements at z = 0: every mover returns early"""
    rng = np.random.default_rng(21)
    z = np.full(n, z_deep)
    z[:surface] = 0.0
    env = {XW: np.full(n, wind[0], f32), YW: np.full(n, wind[1], f32), SX: np.zeros(n, f32), SY: np.zeros(n, f32), HD: np.zeros(n, f32)}
    if cur is not None:
        env[U], env[V] = np.full(n, cur[0], f32), np.full(n, cur[1], f32)
    for nm, v in more.items():
        env[{'w': W, 'depth': DEPTH}[nm]] = np.full(n, v, f32)
    return dict(lon=rng.uniform(4, 6, n), lat=rng.uniform(59, 61, n), z=z, wdf=np.full(n, wdf, f32), status=np.zeros(n, np.int32), env=env)


def _mv(wdd=0.1, rel=False):
    return dict(wind=dict(wind_drift_depth=wdd, relative_wind=rel), stokes=dict(STOKES), hdiffusion=dict(step=0))


def _snapshot(P, names):
    d = P.download()
    d['wdf'], d['tv'] = P.download_f32('wind_drift_factor'), P.download_f32('terminal_velocity')
    d['env'] = {nm: P.env_download(nm) for nm in names}
    return d


def _same_bits(a, b, what):
    for q in ('lon', 'lat', 'z', 'ID', 'status'):
        assert np.array_equal(a[q], b[q]), (what, q, int((a[q] != b[q]).sum()))
    assert np.isfinite(a['lon']).all() and np.isfinite(a['lat']).all(), what


def _moved(a, b):
    return bool(((a['lon'] != b['lon']) | (a['lat'] != b['lat'])).any())


def _second_call_against_a_fresh_set(ctx, P, names, mv, what):
    """P.movers(**mv) against a fresh particle set put into P's present state and moved once: same bits.  Returns whether
    something moved."""
    snap = _snapshot(P, names)
    P.movers(600.0, **mv)
    after = P.download()
    Q = _make(ctx, snap, cap=len(snap['lon']) + 8)
    assert np.array_equal(Q.download()['status'], snap['status'])
    Q.movers(600.0, **mv)
    _same_bits(after, Q.download(), what)
    Q.close()
    return _moved(after, snap)


def _one(i, v, base=0.0, n=N_D):
    a = np.full(n, base, f32)
    a[i] = v
    return a


def _deactivate_one(P, i, code, compact=False):
    m = np.zeros(len(P), np.uint8)
    m[i] = 1
    P.deactivate(m, code)
    if compact:
        P.compact()


def _append_at_surface(P):
    n = len(P)
    P.append(5.0, 60.0, z=0.0, wind_drift_factor=0.02)
    # (the set-up of this case: the new element sits where the compacted one was, whose sampled wind is still there)
    assert len(P) == n + 1 and P.env_download(XW)[n] == 3.0 and P.env_download(YW)[n] == 4.0


# case: (state, prepare, change, movers of the first call, movers of the second call, first call moves, second call moves)
INVALIDATION = {
    'env_upload_wind': (_calm(), None, lambda P: P.env_upload(XW, _one(7, 3.0)), _mv(), _mv(), False, True),
    'env_upload_stokes': (_calm(), None, lambda P: P.env_upload(SX, _one(7, 1.0)), _mv(), _mv(), False, True),
    'env_upload_D': (_calm(), None, lambda P: P.env_upload(HD, _one(150, 10.0)), _mv(), _mv(), False, True),
    'env_add_noise_wind': (_calm(), None, lambda P: P.env_add_noise(XW, YW, 1.0, step=0), _mv(), _mv(), False, True),
    'upload_z': (_calm(surface=0, wind=(3.0, 4.0)), None, lambda P: P.upload(z=np.where(np.arange(N_D) < 50, 0.0, -5.0)), _mv(), _mv(), False, True),
    'upload_wind_drift_factor': (_calm(wind=(3.0, 4.0), wdf=0.0), None, lambda P: P.upload(wind_drift_factor=np.full(N_D, 0.02, f32)),
                                 _mv(), _mv(), False, True),
    'vertical_advection': (_calm(surface=0, z_deep=-1.0, wind=(3.0, 4.0), w=0.002), None, lambda P: P.vertical_advection(600.0),
                           _mv(), _mv(), False, True),
    'vertical_buoyancy': (dict(_calm(surface=0, z_deep=-1.0, wind=(3.0, 4.0), depth=100.0), tv=np.full(N_D, 0.002, f32)), None,
                          lambda P: P.vertical_buoyancy(600.0), _mv(), _mv(), False, True),
    'seafloor': (_calm(surface=0, wind=(3.0, 4.0), depth=0.05), None, lambda P: P.seafloor('lift_to_seafloor'), _mv(), _mv(), False, True),
    'truncate_z': (_calm(surface=0, wind=(3.0, 4.0)), None, lambda P: P.truncate_z(0.05), _mv(), _mv(), False, True),
    'restore_z': (_calm(surface=0, wind=(3.0, 4.0)), lambda P: P.truncate_z(0.05), lambda P: P.restore_z(), _mv(), _mv(), True, False),
    'append': (_calm(surface=0, wind=(3.0, 4.0), n=N_D + 1), lambda P: _deactivate_one(P, N_D, 9, compact=True), _append_at_surface,
               _mv(), _mv(), False, True),
    'deactivate_and_compact': (dict(_calm(), env=dict(_calm()['env'], **{XW: _one(7, 3.0), YW: _one(7, 4.0)})), None,
                               lambda P: _deactivate_one(P, 7, 4, compact=True), _mv(), _mv(), True, False),
    # (deactivate() also stops the element: moving = 0 survives the renumbering.  So the case is built on the Stokes drift,
    # whose test is on the SUM: sx = 1, sy = -1 on every active element, sy = +1 on the deactivated one -- once that one
    # counts again, every element drifts)
    'remap_status_to_active': (dict(_calm(), env=dict(_calm()['env'], **{SX: _one(7, 1.0, base=1.0), SY: _one(7, 1.0, base=-1.0)})),
                               lambda P: _deactivate_one(P, 7, 5), lambda P: P.remap_status(5, 0), _mv(), _mv(), False, True),
    'another_wind_drift_depth': (_calm(surface=0, z_deep=-1.0, wind=(3.0, 4.0)), None, lambda P: None, _mv(0.1), _mv(2.0), False, True),
    'relative_wind_off': (_calm(wind=(3.0, 4.0), cur=(3.0, 4.0)), None, lambda P: None, _mv(rel=True), _mv(rel=False), False, True),
    'relative_wind_on': (_calm(wind=(3.0, 4.0), cur=(3.0, 4.0)), None, lambda P: None, _mv(rel=False), _mv(rel=True), True, False),
}


@pytest.mark.parametrize('case', sorted(INVALIDATION))
def test_every_entry_point_voids_the_cached_reductions(case):
    """movers() fills the cache; ONE change that voids (or, for deactivate_and_compact / restore_z / relative_wind_on, brings
    back) an early-out; movers() again must decide on the new state: the positions equal, bit for bit, those of a fresh
    particle set put into the same state and moved once, and something moved (or nothing did).  remap_status(code, 0)
    re-activates an element and the ABI accepts it, so the case is here; it was the one that failed when these tests were
    written (99 of 300 longitudes differed from the fresh set's: the second call kept the early-out of the first) until
    odr_particles_remap_status bumped the epochs for a renumbering to or from 0."""
    s, prepare, change, mv1, mv2, first_moves, second_moves = INVALIDATION[case]
    ctx = Context(seed=11)
    P = _make(ctx, s, cap=len(s['lon']) + 8)
    if prepare:
        prepare(P)
    before = P.download()
    P.movers(600.0, **mv1)
    assert _moved(P.download(), before) == first_moves, case
    raw, st = P.reduce_cached()
    assert st == dict(valid=True, extents=False, partial=False, pinned=False), (case, st)    # the cache is filled
    change(P)
    assert _second_call_against_a_fresh_set(ctx, P, list(s['env']), mv2, case) == second_moves, case
    P.close()
    ctx.close()


def test_a_compaction_carries_a_valid_cache_over_and_only_a_valid_one():
    """odr_compact_apply keeps the movers' cached reduction (it runs over the active elements, which a compaction neither
    changes nor removes) -- unless something changed since it was formed: deactivate() bumps the epoch, so the cache that
    held the deactivated element's wind must not survive the compaction that follows."""
    ctx = Context(seed=11)
    s = _calm()
    s['env'][XW], s['env'][YW] = _one(7, 3.0), _one(7, 4.0)
    P = _make(ctx, s, cap=N_D + 8)
    P.movers(600.0, **_mv())
    P.compact()                                    # nothing to remove: the cache stays, and stays right
    raw, st = P.reduce_cached()
    want = _ref(s, 0.1, False)
    want[1:7] = -INF
    assert st['valid'] and not st['extents']
    _assert_raw(raw, want, 'carried over')
    _deactivate_one(P, 7, 4)
    assert not P.reduce_cached()[1]['valid']
    P.compact()
    assert not P.reduce_cached()[1]['valid']       # not revived by the compaction
    P.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ e, f: the step launch
def _stere_ctx(g, names, hd=None, seed=3):
    ctx = Context(seed=seed)
    sid = ctx.add_grid(g['x'], g['y'], proj=synth.NORKYST_PROJ)
    for k in range(len(g['t'])):
        ctx.upload_block(sid, k, float(g['t'][k]), {nm: g[nm][k] for nm in names})
    for nm in names:
        ctx.bind(nm, [sid], np.nan if nm == LAND else 0.0)
    if hd is not None:
        ctx.bind(HD, [ctx.add_constant({HD: hd})], 0.0)
    return ctx


def _small_stere(n, seed=4):
    """the polar-stereographic reader of test_gpu_movers._setup on the smallest grid that holds the elements for a step"""
    from opendrift_amd.projection import stere_polar_inverse
    g = synth.grid_stere(nx=48, ny=32, nt=2, seed=0)
    rng = np.random.default_rng(seed)
    x = rng.uniform(g['x'][4], g['x'][36], n)        # (west of the land band, a step of ~1 cell away from every edge)
    y = rng.uniform(g['y'][4], g['y'][-5], n)
    lon, lat = stere_polar_inverse(x, y, **synth.NORKYST_PROJ)
    z = np.where(rng.random(n) < 0.5, 0.0, -rng.uniform(0, 3, n))
    return g, [U, V, XW, YW, SX, SY, LAND], lon, lat, z, rng.uniform(0, 0.05, n).astype(f32)


def _sign(m):
    return 1.0 if m > 0 else (0.0 if m == 0 else -INF)


@pytest.mark.parametrize('rel', [False, True])
def test_values_after_a_step_launch_that_formed_the_movers_tests(rel):
    """With set_step_reduce(True) the launch of env_coast_advect leaves SIGNS in red[] (+1 / 0 / -inf) and marks them partial:
    enough for the movers' `== 0` tests, not for anyone who needs values.  reduce_local and reduce_scalars must hand out the
    true maxima of the state the launch left, and n_surface as a count."""
    n = 1500
    g, names, lon, lat, z, wdf = _small_stere(n)
    ctx = _stere_ctx(g, names, hd=10.0)
    ctx.set_step_reduce(True, wind_drift_depth=0.1, relative_wind=rel)
    P = ctx.particles(n)
    P.append(lon, lat, z=z, wind_drift_factor=wdf)
    P.env_coast_advect(names + [HD], 0.0, 'euler', 900.0, coastline='none', store_previous=False)
    raw, st = P.reduce_cached()
    assert st == dict(valid=True, extents=False, partial=True, pinned=False), st       # the launch did form them
    d = P.download()
    s = dict(lon=d['lon'], lat=d['lat'], z=d['z'], status=d['status'], wdf=P.download_f32('wind_drift_factor'),
             env={nm: P.env_download(nm) for nm in (U, V, XW, YW, SX, SY, HD)})
    assert (s['status'] == 0).all() and np.array_equal(s['z'], z)
    want = _ref(s, 0.1, rel)
    assert want[11] == (z >= -0.1).sum() > 1 and want[14] > 1 and want[7] == 10      # (values a sign cannot be taken for)
    for k in (7, 8, 10, 14):
        assert raw[k] == _sign(want[k]), (R.KEYS[k], raw[k], want[k])
    assert raw[11] == want[11]
    _check_extents_pass(P, s, 0.1, rels=(rel, not rel))
    assert not P.reduce_cached()[1]['partial']
    P.close()
    ctx.set_step_reduce(False)
    ctx.close()


def test_wind_profile_mixing_right_after_such_a_launch_reads_the_true_mld_maximum():
    """vmix_analytic sizes its profile by MLD.max() (oceandrift.py:430): right behind a step launch that left signs in red[]
    it must reduce again -- same z as without the setting."""
    n = 1200
    g, names, lon, lat, z, wdf = _small_stere(n)
    z = -np.random.default_rng(5).uniform(0.5, 30, n)
    mld = np.full(n, 20.0, f32)
    mld[n - 3] = 50.0
    res = []
    for on in (False, True):
        ctx = _stere_ctx(g, names, hd=10.0)
        ctx.set_step_reduce(on, wind_drift_depth=0.1)
        P = ctx.particles(n)
        P.append(lon, lat, z=z, wind_drift_factor=wdf)
        P.env_upload(DEPTH, np.full(n, 100.0, f32))
        P.env_upload(MLD, mld)
        P.env_coast_advect(names + [HD], 0.0, 'euler', 900.0, coastline='none', store_previous=False)
        assert P.reduce_cached()[1]['partial'] == on
        P.vmix_analytic('windspeed_Large1994', 1.2e-5, 900.0, 60.0, step=0)
        raw, st = P.reduce_cached()
        assert raw[15] == 50.0 and not st['partial']        # what the mixing launch read
        res.append(P.download())
        P.close()
        ctx.set_step_reduce(False)
        ctx.close()
    _same_bits(res[0], res[1], 'vmix_analytic')
    assert (res[1]['z'] != z).mean() > 0.9


def test_the_records_of_a_step_launch_beyond_one_trip_of_their_fold():
    """k_red_finish is grid-stride over at most 128 workgroups of 256: wave records 32 768 and later (elements 2 097 152 and
    later) are folded in a second trip.  Everything is calm and at the surface; ONE element in such a wave has wind and one,
    in the launch's last and partial wave, Stokes drift (each on a node of its own, as in test_gpu_movers.py::
    test_one_nonzero_element_in_any_lane_keeps_the_mover_alive; lane 3 only: that test sweeps the lanes).  The movers must
    stay alive with the tests formed by the launch exactly as with the pass over the arrays."""
    from opendrift_amd.projection import stere_polar_inverse
    n = 64 * (128 * 256) + 64 * 300 + 5
    i_wind, i_stokes = 64 * (128 * 256 + 5) + 3, 64 * (128 * 256 + 300) + 3
    assert i_wind // 64 >= 32768 and i_stokes // 64 == (n - 1) // 64 and i_stokes < n
    g = synth.grid_stere(nx=48, ny=32, nt=2, seed=0)
    names = [U, V, XW, YW, SX, SY, LAND]
    for nm in names:
        g[nm][:] = 0
    nodes = {'calm': (10, 10), 'wind': (10, 20), 'stokes': (20, 20)}         # (row, column): far apart, nothing interpolates across
    g[XW][:, 10, 20] = g[YW][:, 10, 20] = 4.0
    g[SX][:, 20, 20] = g[SY][:, 20, 20] = 4.0
    kinds = sorted(nodes)
    nlon, nlat = stere_polar_inverse(np.array([g['x'][nodes[k][1]] for k in kinds], dtype=np.float64),
                                     np.array([g['y'][nodes[k][0]] for k in kinds], dtype=np.float64), **synth.NORKYST_PROJ)
    lon, lat = np.full(n, nlon[kinds.index('calm')]), np.full(n, nlat[kinds.index('calm')])
    for k, i in (('wind', i_wind), ('stokes', i_stokes)):
        lon[i], lat[i] = nlon[kinds.index(k)], nlat[kinds.index(k)]
    res = []
    for on in (False, True):
        ctx = _stere_ctx(g, names)
        ctx.set_step_reduce(on, wind_drift_depth=0.1)
        P = ctx.particles(n)
        P.append(lon, lat, z=np.zeros(n))
        P.env_coast_advect(names, 0.0, 'euler', 600.0, coastline='none', store_previous=False)
        raw, st = P.reduce_cached()
        assert st['partial'] == on and (not on or (st['valid'] and raw[8] == 1 and raw[14] == 1 and raw[11] == n)), (on, st, raw)
        P.movers(600.0, wind=dict(wind_drift_depth=0.1), stokes=dict(STOKES))
        if on:
            assert P.reduce_cached()[1]['partial']          # the movers did take the launch's tests
        res.append(P.download())
        P.close()
        ctx.set_step_reduce(False)
        ctx.close()
    _same_bits(res[0], res[1], 'on against off')
    moved = np.flatnonzero((res[1]['lon'] != lon) | (res[1]['lat'] != lat))
    assert i_wind in moved and i_stokes in moved, moved[:5]


# ------------------------------------------------------------------------------------------------ g
def test_rows_of_two_particle_sets_combine_to_the_row_of_their_union():
    ctx = Context(seed=1)
    s = _random_state(700, seed=12)
    s['status'][[5, 310, 650]] = 2
    part = lambda a, b: dict({q: s[q][a:b] for q in ('lon', 'lat', 'z', 'wdf', 'status')}, env={nm: v[a:b] for nm, v in s['env'].items()})
    PA, PB, PW = _make(ctx, part(0, 300)), _make(ctx, part(300, 700)), _make(ctx, s)
    for wdd, rel in ((0.1, False), (2.0, True)):
        rows = [PA.reduce_local(wdd, rel).copy(), PB.reduce_local(wdd, rel).copy()]
        whole = PW.reduce_local(wdd, rel)
        _assert_raw(R.combine(rows), whole, ('combined', wdd, rel))
        _assert_raw(whole, _ref(s, wdd, rel), ('whole', wdd, rel))
    for X in (PA, PB, PW):
        X.close()
    ctx.close()


def _diffusive(ctx, n=300, d=10.0):
    s = _random_state(n, seed=13, names=[HD])
    s['env'][HD][:] = d
    return s, _make(ctx, s)


def test_an_installed_row_rules_until_it_is_unpinned():
    ctx = Context(seed=1)
    s, P = _diffusive(ctx)
    row = P.reduce_local()
    assert row[7] == 10
    row[7] = 0.0                                   # "D is 0 on every rank"
    P.reduce_install(row)
    start = P.download()
    P.hdiffusion(600.0, step=0)
    assert not _moved(P.download(), start)
    P.env_upload(HD, np.full(len(start['lon']), 10.0, f32))      # a state change in between does not reduce again while pinned
    P.hdiffusion(600.0, step=1)
    assert not _moved(P.download(), start)
    raw, st = P.reduce_cached()
    assert st['pinned'] and st['valid'] and raw[7] == 0
    P.reduce_unpin()
    P.hdiffusion(600.0, step=2)
    assert _moved(P.download(), start)
    raw, st = P.reduce_cached()
    assert raw[7] == 10 and st == dict(valid=True, extents=False, partial=False, pinned=False)
    P.close()
    ctx.close()


@pytest.mark.parametrize('reader', ['reduce_local', 'reduce_scalars'])
def test_reading_the_reductions_releases_an_installed_row(reader):
    """reduce_local (and reduce_scalars) overwrite red[] with THIS set's values: they clear the pin, and the next mover
    decides on the present state, not on the row installed before."""
    ctx = Context(seed=1)
    s, P = _diffusive(ctx)
    row = P.reduce_local()
    row[7] = 0.0
    P.reduce_install(row)
    assert P.reduce_cached()[1]['pinned']
    got = P.reduce_local() if reader == 'reduce_local' else P.reduce_scalars()
    assert (got[7] if reader == 'reduce_local' else got['D_max']) == 10
    assert not P.reduce_cached()[1]['pinned']
    start = P.download()
    P.hdiffusion(600.0, step=0)
    assert _moved(P.download(), start)             # the installed D_max = 0 is gone
    P.env_upload(HD, np.zeros(len(start['lon']), f32))
    mid = P.download()
    P.hdiffusion(600.0, step=1)                    # and the next mover reduces afresh: D is 0 now
    raw, st = P.reduce_cached()
    assert raw[7] == 0 and st['valid'] and not st['pinned']
    assert not _moved(P.download(), mid)
    P.close()
    ctx.close()
