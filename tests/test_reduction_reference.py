"""CPU: tests/reduction_ref.py (the NumPy reference tests/test_gpu_reductions.py holds the device against) on sets of three
to six elements whose sixteen slots are worked out by hand in the comments -- so that the reference cannot be wrong
together with the kernel.  Every number below is exact in float32 (and hence in float64) unless its comment says how it
rounds."""
import numpy as np

import reduction_ref as R

INF = np.inf
f32 = np.float32


def _env(**kw):
    short = dict(u=R.U, v=R.V, xw=R.XW, yw=R.YW, sx=R.SX, sy=R.SY, hd=R.HD, hs=R.HS, tp=R.TP, mld=R.MLD)
    return {short[k]: np.asarray(v, dtype=np.float32) for k, v in kw.items()}


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == (16,)
    bad = [(k, R.KEYS[k], got[k], want[k]) for k in range(16) if not got[k] == want[k]]
    assert not bad, bad


# five elements, one of them deactivated and holding what would be the extreme of every slot
LON = [4.0, 5.5, -3.25, 100.0, 4.5]
LAT = [60.0, 61.5, 59.75, -80.0, 60.5]
Z = [0.0, -1.0, -4.0, 7.0, -0.5]
ST = [0, 0, 0, 3, 0]
WDF = [0.5, 0.25, 1.0, 9.0, 0.125]
ENV = dict(u=[1, 0, 0, 50, -1], v=[0, 2, 0, 50, 0], xw=[3, 0, 30, 90, -6], yw=[4, -5, 40, 90, 8],
           sx=[0.5, -1, 2, 70, 0], sy=[0.25, 3, -2.5, 70, 0], hd=[1, 7, 3, 99, 2], hs=[0.5, 0.75, 2.5, 40, 1],
           tp=[8, 6, 4, 44, 9.5], mld=[20, 55, 30, 400, 10])


def test_every_slot_with_every_variable_present():
    # active: 0, 1, 2, 4.  wind_drift_depth 2: surface = z >= -2 -> elements 0 (z 0), 1 (z -1), 4 (z -0.5); 2 (z -4) is below
    #   wdf: 0.5*(2+0)/2 = 0.5;  0.25*(2-1)/2 = 0.125;  0.125*(2-0.5)/2 = 0.09375          -> max 0.5
    #   wind speed: (3,4) -> 5;  (0,-5) -> 5;  (-6,8) -> 10                                  -> max 10  (element 2's 50 is below)
    #   relative:   (3-1, 4-0) = (2,4) -> sqrt(20);  (0-0, -5-2) -> 7;  (-6+1, 8-0) = (-5,8) -> sqrt(89)
    #   stokes sums: 0.75, 2, -0.5, 0 -> 2;   D 7;  Hs 2.5;  Tp 9.5;  MLD 55
    raw = R.raw16(LON, LAT, Z, ST, WDF, _env(**ENV), 2.0, False)
    _same(raw, [4, 3.25, 5.5, -59.75, 61.5, 4.0, 0.0, 7, 2, 10, 0.5, 3, 2.5, 9.5, 10, 55])
    rel = R.raw16(LON, LAT, Z, ST, WDF, _env(**ENV), 2.0, True)
    assert rel[14] == float(np.sqrt(f32(89)))      # float32 square root, then widened
    assert rel[14] != np.sqrt(89.0)
    rel[14] = raw[14]
    _same(rel, raw)                                 # nothing else depends on relative_wind
    # the sign of wind_drift_depth does not matter (np.abs, :737)
    _same(R.raw16(LON, LAT, Z, ST, WDF, _env(**ENV), -2.0, False), raw)


def test_as_dict_names_every_slot_and_restores_the_minima():
    raw = R.raw16(LON, LAT, Z, ST, WDF, _env(**ENV), 2.0, False)
    d = R.as_dict(raw)
    assert list(d) == R.KEYS and len(d) == 16
    assert (d['lon_min'], d['lat_min'], d['z_min']) == (-3.25, 59.75, -4.0)
    assert (d['lon_max'], d['lat_max'], d['z_max']) == (5.5, 61.5, 0.0)
    assert (d['n_active'], d['n_surface'], d['rel_wind_speed_max'], d['mld_max']) == (4, 3, 10, 55)
    # what the package's own dictionary makes of the same row
    from opendrift_amd.device import Particles
    assert Particles.reduction_dict(raw) == d


def test_wind_drift_depth_edges():
    env = _env(xw=[3, 0, 30, 6], yw=[4, -5, 40, 8])
    z = [0.0, -0.1, -0.1000001, 2.0]
    wdf = [0.5, 0.25, 1.0, 0.125]
    st = [0, 0, 0, 0]
    ll = [0.0] * 4
    # wdd 0.1: z == -wdd exactly IS at the surface and its factor is 0.25*(0.1 - 0.1)/0.1 = 0; the element a hair below is not;
    # z > 0 keeps its own factor (0.125, not 0.125*2.1/0.1 = 2.625); element 0: 0.5*(0.1+0)/0.1 = 0.5 (x*y/y, |error| <= 1 ulp:
    # computed, not assumed)
    raw = R.raw16(ll, ll, z, st, wdf, env, 0.1, False)
    assert raw[11] == 3 and raw[10] == 0.5 * (0.1 + 0.0) / 0.1 and raw[9] == 10 and raw[14] == 10
    assert raw[10] < 2.0
    # wdd 0 ("surface only"): z >= 0 -> elements 0 and 3, factors untouched -> 0.5; speeds 5 and 10
    raw = R.raw16(ll, ll, z, st, wdf, env, 0.0, False)
    assert raw[11] == 2 and raw[10] == 0.5 and raw[9] == 10
    # wdd 1e30 (every element is "at the surface"): factors ~ their own value for z <= 0 -> max 1.0*(1e30 - 0.1000001)/1e30 == 1.0;
    # the fastest wind is the deep element's 50
    raw = R.raw16(ll, ll, z, st, wdf, env, 1e30, False)
    assert raw[11] == 4 and raw[10] == 1.0 and raw[9] == 50
    # negative depth == its absolute value
    _same(R.raw16(ll, ll, z, st, wdf, env, -0.1, True), R.raw16(ll, ll, z, st, wdf, env, 0.1, False))
    # every element below: the surface slots stay empty, the counts are counts
    raw = R.raw16(ll, ll, [-5.0, -6.0, -7.0, -8.0], st, wdf, env, 0.1, False)
    assert raw[11] == 0 and raw[10] == -INF and raw[9] == -INF and raw[14] == -INF and raw[0] == 4


def test_wdf_is_scaled_in_float64_from_the_float32_factor():
    # 0.1f is 0.100000001490116...; (0.1f * (3 + -1)) / 3 in float64 -- not float32 arithmetic, not 0.1 (double)
    env = _env(xw=[1, 1, 1], yw=[0, 0, 0])
    raw = R.raw16([0] * 3, [0] * 3, [-1.0, -2.0, -2.5], [0] * 3, [0.1, 0.1, 0.1], env, 3.0, False)
    want = float(f32(0.1)) * (3.0 + -1.0) / 3.0
    assert raw[10] == want and want != 0.1 * 2.0 / 3.0 and want != float(f32(0.1) * f32(2.0) / f32(3.0))


def test_absent_variables_leave_their_slots_empty():
    full = R.raw16(LON, LAT, Z, ST, WDF, _env(**ENV), 2.0, True)

    def without(*names):
        return R.raw16(LON, LAT, Z, ST, WDF, _env(**{k: v for k, v in ENV.items() if k not in names}), 2.0, True)

    def differs(raw, slots):
        assert sorted(k for k in range(16) if not raw[k] == full[k]) == sorted(slots)

    r = without('xw', 'yw')                       # no wind: no surface bookkeeping at all
    differs(r, [9, 10, 11, 14])
    assert r[11] == 0 and r[9] == r[10] == r[14] == -INF
    differs(without('yw'), [9, 10, 11, 14])       # one component is no wind either
    r = without('u', 'v')                         # wind, no current, relative wind asked for: the plain wind speed
    differs(r, [14])
    assert r[14] == r[9] == 10
    assert without('v')[14] == 10                 # both current components or none (:762-768 raise and pass otherwise)
    for one in ('sx', 'sy'):                      # one Stokes component: no sum
        r = without(one)
        differs(r, [8])
        assert r[8] == -INF
    for name, slot in (('hd', 7), ('hs', 12), ('tp', 13), ('mld', 15)):
        r = without(name)
        differs(r, [slot])
        assert r[slot] == -INF
    r = R.raw16(LON, LAT, Z, ST, WDF, {}, 2.0, False)      # nothing sampled: counts and extents only
    _same(r, [4, 3.25, 5.5, -59.75, 61.5, 4.0, 0.0] + [-INF] * 4 + [0] + [-INF] * 4)


def test_nothing_active_and_nothing_at_all():
    want = [0] + [-INF] * 10 + [0] + [-INF] * 4
    _same(R.raw16(LON, LAT, Z, [1, 2, 3, 4, 5], WDF, _env(**ENV), 2.0, True), want)
    _same(R.raw16([], [], [], [], [], _env(**{k: [] for k in ENV}), 2.0, True), want)
    d = R.as_dict(np.array(want, dtype=np.float64))
    assert d['n_active'] == 0 and d['lon_min'] == d['lat_min'] == d['z_min'] == INF and d['z_max'] == d['D_max'] == -INF


def test_nan_is_ignored_and_zero_signs_compare_equal():
    nan = np.nan
    # NaN in z: that element is neither an extreme nor at the surface (so its wind of 50 and its factor 9 do not count)
    env = _env(xw=[3, 50, 0], yw=[4, 0, 0], hd=[nan, 2, 1], sx=[1, nan, -1], sy=[1, 5, 1], hs=[nan, nan, nan], mld=[5, nan, 7],
               tp=[nan, 3, nan])
    raw = R.raw16([1, nan, 3], [nan, 2, 3], [-1.0, nan, 0.0], [0, 0, 0], [0.5, 9.0, 0.25], env, 2.0, False)
    _same(raw, [3, -1, 3, -2, 3, 1.0, 0.0, 2, 2, 5, 0.25, 2, -INF, 3, 5, 7])
    # -0.0 against 0.0: equal under ==, whichever the maximum returns
    env = _env(xw=[-0.0, 0.0, -0.0], yw=[0.0, -0.0, -0.0], hd=[-0.0, 0.0, -0.0], sx=[1, 1, 1], sy=[-1, -1, -1])
    raw = R.raw16([0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [0, 0, 0], [0.0, -0.0, 0.0], env, 0.1, False)
    _same(raw, [3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, -INF, -INF, 0, -INF])
    # all-negative D: the maximum is negative, not 0
    raw = R.raw16([0] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3, _env(hd=[-3, -0.5, -2]), 0.1, False)
    assert raw[7] == -0.5


def test_stokes_sum_is_a_float32_sum():
    # 1 + 2^-24 rounds to 1 in float32 (ties to even); in float64 it would not
    raw = R.raw16([0] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3, _env(sx=[1, 0, 0], sy=[2.0 ** -24, 0, 0]), 0.1, False)
    assert raw[8] == 1.0


def test_combine_sums_the_counts_and_maximises_the_rest():
    env = _env(**ENV)
    whole = R.raw16(LON, LAT, Z, ST, WDF, env, 2.0, True)
    parts = [R.raw16(LON[a:b], LAT[a:b], Z[a:b], ST[a:b], WDF[a:b], {k: v[a:b] for k, v in env.items()}, 2.0, True)
             for a, b in ((0, 2), (2, 5))]
    _same(R.combine(parts), whole)
