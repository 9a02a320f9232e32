"""Device result buffer (odr_history_*) at its edges, bit for bit against oracle/history.py: every record width
(k_hist_record<1> .. <10>), every source kind, the float32 casts at their limits, the trajectory window of a sharded
run (id_base), previous positions and property snapshots, partial / repeated / chunked flushes, a record behind a flush
in flight, and k_hist_minmax off the easy path.  No tolerance anywhere."""
import numpy as np
import pytest

from opendrift_amd._abi import VARIABLES
from oracle.history import HistoryOracle

pytestmark = pytest.mark.gpu

ENV = [name for name, _ in sorted(VARIABLES.items(), key=lambda kv: kv[1])][:22]
# the 40 variables of the widest record: float64, int32 and float32 element properties, the nine property slots, 22
# environment variables
NAMES = (['lon', 'lat', 'z', 'status', 'moving', 'age_seconds', 'wind_drift_factor', 'current_drift_factor',
          'terminal_velocity'] + [('property', s) for s in range(9)] + ENV)
assert len(NAMES) == 40
K = {name: k for k, name in enumerate(NAMES)}
FLT_MAX = float(np.finfo(np.float32).max)
I32_MAX = 2 ** 31 - 1


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _same_scalar(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def _check(H, O, names, t0=0, nt=None):
    """every variable of the last flush (time slots [t0, t0 + nt)) against the oracle"""
    nt = O.buf[names[0]].shape[1] - t0 if nt is None else nt
    for v in names:
        a = H.array(v)
        assert a.dtype == np.float32 and a.shape == (O.n_trajectories, nt), (v, a.shape)
        want = O.buf[v][:, t0:t0 + nt]
        assert _same(a, want), (v, int((~((a == want) | (np.isnan(a) & np.isnan(want)))).sum()))


def _check_minmax(H, O, names):
    for v in names:
        lo, hi = H.minmax(v)
        olo, ohi = O.minmax(v)
        assert _same_scalar(lo, olo) and _same_scalar(hi, ohi), (v, lo, olo, hi, ohi)


# ------------------------------------------------------------------ 1. every record width
def _fill(P, ids, shift):
    """Variable k of NAMES (status and age_seconds apart) := 2000 * (k + 1) + ID + shift at every element: exact in
    float32, and no two variables share a value, so that a swap of lanes, variables or elements cannot cancel."""
    val = {name: 2000.0 * (k + 1) + ids + shift for name, k in K.items()}
    P.upload(lon=val['lon'], lat=val['lat'], z=val['z'], moving=val['moving'].astype(np.int32),
             wind_drift_factor=val['wind_drift_factor'].astype(np.float32),
             current_drift_factor=val['current_drift_factor'].astype(np.float32),
             terminal_velocity=val['terminal_velocity'].astype(np.float32))
    for s in range(9):
        P.set_property(s, val[('property', s)].astype(np.float32))
    for name in ENV:
        P.env_upload(name, val[name].astype(np.float32))
    val['moving'] = val['moving'].astype(np.int32)
    return val


WIDTHS = [1, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 36, 37, 39, 40]
WIDTH_CASES = [(w, 1025) for w in WIDTHS] + [(w, n) for w in (1, 5, 40) for n in (1, 63, 64, 65, 257)]


@pytest.mark.parametrize('nvars,n', [pytest.param(w, n, id='NQ%d-nvars%d-n%d' % ((w + 3) // 4, w, n)) for w, n in WIDTH_CASES])
def test_every_record_width_and_source_kind(ctx, nvars, n):
    """The first nvars of the 40 variables (stride / 4 = NQ of the id): one record of every element into slot 0, one of
    the deactivated elements only into slot 2 with other values, slot 1 left alone.  Device order is a permutation
    against ID and some rows of the buffer belong to no element."""
    rng = np.random.default_rng(1000 * nvars + n)
    names = NAMES[:nvars]
    ntraj, nt = n + 5, 3
    ids = rng.permutation(ntraj)[:n].astype(np.int32)
    dead = rng.uniform(size=n) < 0.3
    dead[0] = True
    if n > 1:
        dead[1] = False
    P = ctx.particles(n + 3)
    n1 = n // 2                                     # two releases: two ages
    z = np.zeros(n)
    if n1:
        P.append(z[:n1], z[:n1], id=ids[:n1])
        P.increase_age(512.5)
    P.append(z[n1:], z[n1:], id=ids[n1:])
    P.increase_age(12000.25)
    age = np.zeros(n, np.float32)
    age[:n1] += np.float32(512.5)
    age += np.float32(12000.25)
    status = np.where(dead, 8001 + ids % 3, 0).astype(np.int32)
    for code in (8001, 8002, 8003):
        P.deactivate(status == code, code)
    H = ctx.history(ntraj, nt, names)
    O = HistoryOracle(ntraj, nt, names)
    for slot, shift, only_deactivated in ((0, 0.0, False), (2, 100000.0, True)):
        val = _fill(P, ids.astype(np.float64), shift)       # (after deactivate: it clears `moving`)
        if shift:
            P.increase_age(shift)
            age = age + np.float32(shift)
        val['status'], val['age_seconds'] = status, age
        got = P.download()
        assert np.array_equal(got['ID'], ids) and np.array_equal(got['status'], status) and np.array_equal(got['moving'], val['moving'])
        H.record(P, slot, only_deactivated)
        O.record(slot, ids, status, val, only_deactivated)
    H.flush()
    H.wait()
    _check(H, O, names)
    absent = np.setdiff1d(np.arange(ntraj), ids)
    for v in names:
        a = H.array(v)
        assert np.isnan(a[:, 1]).all() and np.isnan(a[absent]).all(), v
        assert np.isfinite(a[ids, 0]).all() and np.isfinite(a[ids[dead], 2]).all() and np.isnan(a[ids[~dead], 2]).all(), v
    _check_minmax(H, O, names)
    H.close()


# ------------------------------------------------------------------ 2. casts
def test_float32_casts_at_their_edges(ctx):
    """float64 -> float32 at round-to-even ties of both parities, beyond FLT_MAX, at subnormals and signed zeros;
    int32 -> float32 above 2^24: NumPy's assignment cast, compared as bit patterns."""
    f = np.array([1.0, 4.2, 1e10, 1e-30, 3.0e38, 1.5e-40], np.float32)          # (the last one is subnormal)
    lo = np.concatenate([f, np.nextafter(f, np.float32(np.inf))])               # both parities of the last mantissa bit
    ties = (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) / 2
    assert (np.unique(lo.view(np.uint32) & 1) == [0, 1]).all() and (ties.astype(np.float32).astype(np.float64) != ties).all()
    lon = np.concatenate([ties, np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf)])
    lat = -lon
    zed = np.array([3.5e38, -3.5e38, 1e-45, -1e-45, 1e-39, -1e-39, 0.0, -0.0, np.nan, np.inf, -np.inf,
                    FLT_MAX, -FLT_MAX, (FLT_MAX + 2.0 ** 128) / 2, np.nextafter((FLT_MAX + 2.0 ** 128) / 2, 0.0),
                    2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 3 * 2.0 ** -150, -3 * 2.0 ** -150, 2.0 ** -126])
    n = len(lon)
    z = np.resize(zed, n)
    assert n >= len(zed)
    moving = np.resize(np.array([2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, I32_MAX, -2 ** 31, 2 ** 25 + 2, 2 ** 25 + 6,
                                 I32_MAX - 64, I32_MAX - 63, 16777217 * 3, 0, -1], np.int32), n)
    codes = (1, 2 ** 24 + 1, I32_MAX)
    status = np.resize(np.array((0,) + codes, np.int32), n)
    prop = np.resize(np.array([0.0, -0.0, 1e-45, -1e-39, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan, 1.17549435e-38],
                              np.float32), n)
    names = ['lon', 'lat', 'z', 'status', 'moving', ('property', 0)]
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    for code in codes:
        P.deactivate(status == code, code)
    P.upload(moving=moving)
    P.set_property(0, prop)
    got = P.download()
    assert np.array_equal(got['status'], status) and np.array_equal(got['moving'], moving)
    H = ctx.history(n, 2, names)
    O = HistoryOracle(n, 2, names)
    val = {'lon': lon, 'lat': lat, 'z': z, 'status': status, 'moving': moving, ('property', 0): prop}
    with np.errstate(over='ignore', invalid='ignore'):
        O.record(0, np.arange(n), status, val)
        O.record(1, np.arange(n), status, val, only_deactivated=True)
    H.record(P, 0)
    H.record(P, 1, only_deactivated=True)
    H.flush()
    H.wait()
    for v in names:
        a, want = H.array(v), O.buf[v]
        bad = np.flatnonzero((a.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert bad.size == 0, (v, bad[:5], a[bad[:5], 0], want[bad[:5], 0], np.asarray(val[v])[bad[:5]])
    assert np.isinf(O.buf['z']).any() and (O.buf['status'] == 2.0 ** 31).any() and (O.buf['lon'] == np.float32(1.0)).any()
    assert (O.buf['z'].view(np.uint32) == 0x80000000).any()          # -0.0 is in the expectation
    _check_minmax(H, O, names)
    H.close()


# ------------------------------------------------------------------ 3. trajectory window
@pytest.mark.parametrize('id_base,ntraj', [(37, 100), (150, 100), (0, 100), (500, 100), (199, 3)])
def test_id_base_window(ctx, id_base, ntraj):
    """The buffer of one rank of a sharded run: elements with the IDs 0..199 in shuffled order, a buffer of the rows
    [id_base, id_base + ntraj).  (37, 100): rows 0..99 hold the IDs 37..136; (150, 100): the IDs end at row 49, the
    rest stays NaN; (0, 100): IDs at or above ntraj are dropped; (500, 100): nothing is written."""
    rng = np.random.default_rng(id_base)
    n = 200
    ids = rng.permutation(n).astype(np.int32)
    lon = 1000.0 + ids + 1e-7
    prop = (5000 + ids).astype(np.float32)
    status = np.where(ids % 3 == 0, 7, 0).astype(np.int32)
    P = ctx.particles(n)
    P.append(lon, np.zeros(n), id=ids)
    P.set_property(4, prop)
    P.deactivate(status == 7, 7)
    names = ['lon', 'status', ('property', 4)]
    H = ctx.history(ntraj, 3, names, id_base=id_base)
    O = HistoryOracle(ntraj, 3, names, id_base=id_base)
    val = {'lon': lon, 'status': status, ('property', 4): prop}
    for slot, only_deactivated in ((1, False), (2, True)):
        H.record(P, slot, only_deactivated)
        O.record(slot, ids, status, val, only_deactivated)
    H.flush()
    H.wait()
    _check(H, O, names)
    _check_minmax(H, O, names)
    a = H.array(('property', 4))
    rows = np.arange(ntraj)
    held = id_base + rows < n                                 # rows whose ID exists
    assert np.array_equal(a[held, 1], (5000 + id_base + rows[held]).astype(np.float32)) and np.isnan(a[~held]).all()
    assert np.isnan(a[:, 0]).all()
    H.close()


# ------------------------------------------------------------------ 4. previous position, snapshots
def test_position_from_previous_and_property_snapshots(ctx):
    rng = np.random.default_rng(4)
    n, extra = 300, 50
    names = ['lon', 'lat', 'z', ('property', 0), ('property', 1)]
    P = ctx.particles(n + extra + 50)                          # room left after the append: the capacity is not the count
    lon0, lat0 = rng.uniform(3, 5, n), rng.uniform(60, 62, n)
    P.append(lon0, lat0, z=-rng.uniform(0, 10, n))
    a0, b0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    P.set_property(0, a0)
    P.set_property(1, b0)
    P.store_previous()
    P.update_positions(rng.standard_normal(n), rng.standard_normal(n), 600.0)
    z1 = -rng.uniform(20, 30, n)
    P.upload(z=z1)
    d = P.download()
    lon1, lat1 = d['lon'], d['lat']
    assert (lon1 != lon0).all() and (lat1 != lat0).all()
    ntraj = n + extra
    H = ctx.history(ntraj, 6, names)
    O = HistoryOracle(ntraj, 6, names)
    ids, st = np.arange(n), np.zeros(n, np.int32)

    def vals(lon, lat, z, a, b):
        return {'lon': lon, 'lat': lat, 'z': z, ('property', 0): a, ('property', 1): b}
    H.record(P, 0, position_from_previous=1)                  # stored lon / lat, current z
    O.record(0, ids, st, vals(lon0, lat0, z1, a0, b0))
    H.record(P, 1, position_from_previous=0)
    O.record(1, ids, st, vals(lon1, lat1, z1, a0, b0))
    P.snapshot_property(1)
    a1, b1 = a0 + np.float32(10), b0 + np.float32(20)
    P.set_property(0, a1)
    P.set_property(1, b1)
    H.record(P, 2, position_from_previous=2)                  # slot 0 has no snapshot: live; slot 1: the copy
    O.record(2, ids, st, vals(lon1, lat1, z1, a1, b0))
    H.record(P, 3, position_from_previous=3)
    O.record(3, ids, st, vals(lon0, lat0, z1, a1, b0))
    H.record(P, 4, position_from_previous=0)
    O.record(4, ids, st, vals(lon1, lat1, z1, a1, b1))
    # the set grows (within its capacity): the copy holds fewer elements than the record writes and is no longer valid
    # (include/odrift.h); the record reads the live slot of every element
    lonx, latx, zx = rng.uniform(3, 5, extra), rng.uniform(60, 62, extra), -rng.uniform(0, 10, extra)
    P.append(lonx, latx, z=zx)
    a2, b2 = rng.standard_normal(ntraj).astype(np.float32), rng.standard_normal(ntraj).astype(np.float32)
    P.set_property(0, a2)
    P.set_property(1, b2)
    H.record(P, 5, position_from_previous=2)
    O.record(5, np.arange(ntraj), np.zeros(ntraj, np.int32),
             vals(np.concatenate([lon1, lonx]), np.concatenate([lat1, latx]), np.concatenate([z1, zx]), a2, b2))
    H.flush()
    H.wait()
    _check(H, O, names)
    _check_minmax(H, O, names)
    H.close()


# ------------------------------------------------------------------ 5. flush paths
def test_partial_and_repeated_flushes(ctx):
    """flush(), flush(2, 1), flush(4, 2), flush(): the pinned buffer is reused with another row length each time"""
    rng = np.random.default_rng(5)
    n, nt = 700, 6
    U = 'x_sea_water_velocity'
    names = ['lon', 'status', U]
    ids = rng.permutation(n + 9)[:n].astype(np.int32)
    P = ctx.particles(n)
    P.append(np.zeros(n), np.zeros(n), id=ids)
    status = np.where(rng.uniform(size=n) < 0.4, 3, 0).astype(np.int32)
    P.deactivate(status == 3, 3)
    H = ctx.history(n + 9, nt, names)
    O = HistoryOracle(n + 9, nt, names)
    for slot in range(nt):
        lon, u = 100.0 * slot + rng.uniform(0, 1, n), (50 * slot + rng.standard_normal(n)).astype(np.float32)
        P.upload(lon=lon)
        P.env_upload(U, u)
        H.record(P, slot, only_deactivated=bool(slot % 2))
        O.record(slot, ids, status, {'lon': lon, 'status': status, U: u}, only_deactivated=bool(slot % 2))
    for t0, m in ((0, None), (2, 1), (4, 2), (0, None), (5, 1), (1, 5)):
        H.flush(t0, m)
        H.wait()
        _check(H, O, names, t0, m)
    _check_minmax(H, O, names)
    H.close()


def test_record_and_reset_behind_a_flush_in_flight(ctx):
    """A record into a slot that a flush is still reading, and a reset directly behind a flush, wait for the flush on
    the device: the host arrays hold what the buffer held when the flush was issued."""
    n = 1 << 19
    names = ['lon', 'status', 'z']
    ids, st = np.arange(n), np.zeros(n, np.int32)
    old = {'lon': np.arange(n) * 1e-3, 'status': st, 'z': -np.arange(n) * 0.5}
    new = {'lon': 700.0 + np.arange(n) * 1e-3, 'status': st, 'z': 9.0 + np.arange(n)}
    P, P2 = ctx.particles(n), ctx.particles(n)
    P.append(old['lon'], np.zeros(n), z=old['z'])
    P2.append(new['lon'], np.zeros(n), z=new['z'])
    H = ctx.history(n, 2, names)
    O = HistoryOracle(n, 2, names)
    for slot in (0, 1):
        H.record(P, slot)
        O.record(slot, ids, st, old)
    H.flush(0, 2)
    H.record(P2, 0)                                           # before wait(): must not reach the flush
    H.wait()
    _check(H, O, names)
    O.record(0, ids, st, new)
    H.flush()
    H.wait()
    _check(H, O, names)
    assert H.array('lon')[5, 0] == np.float32(700.005) and H.array('lon')[5, 1] == np.float32(0.005)
    H.flush()
    H.reset()                                                 # no wait in between
    H.wait()
    _check(H, O, names)
    H.flush()
    H.wait()
    assert all(np.isnan(H.array(v)).all() for v in names) and np.isnan(H.minmax('z')).all()
    H.close()


def test_chunked_flush_at_its_smallest_size(ctx):
    """ntraj * nt > 2^27 splits a variable of the flush into chunks of 2^27 / nt trajectories: nt = 2048 gives chunks of
    65536 rows, ntraj = 65536 + 3 a second chunk of 3 rows, and two variables use both halves of the staging buffer in
    turn.  Rows on both sides of the chunk boundary are written, in the first, a middle and the last time slot."""
    rng = np.random.default_rng(6)
    nt, ntraj = 2048, 65536 + 3
    names = ['z', 'status']                                   # one float64 and one int32 source
    ids = np.unique(np.concatenate([[0, 1, 65535, 65536, 65538], rng.integers(0, ntraj, 1000)]))
    ids = rng.permutation(ids).astype(np.int32)
    n = len(ids)
    P = ctx.particles(n)
    P.append(np.zeros(n), np.zeros(n), id=ids)
    H = ctx.history(ntraj, nt, names)
    O = HistoryOracle(ntraj, nt, names)
    status = np.zeros(n, np.int32)
    for slot, only_deactivated, code in ((0, False, 0), (1, False, 11), (1023, True, 0), (2047, False, 12)):
        if code:
            hit = (rng.uniform(size=n) < 0.3) & (status == 0)
            hit[ids == 65536] |= code == 11                   # a row of the second chunk is in the deactivated-only record
            hit &= status == 0
            P.deactivate(hit, code)
            status = np.where(hit, code, status).astype(np.int32)
        z = -(ids + 1e5 * (slot + 1)) - 1e-7
        P.upload(z=z)
        H.record(P, slot, only_deactivated)
        O.record(slot, ids, status, {'z': z, 'status': status}, only_deactivated)
    assert np.isfinite(O.buf['z'][65536, 1023]) and np.isfinite(O.buf['z'][65538, 2047]) and np.isfinite(O.buf['z'][65535, 0])
    H.flush()
    H.wait()
    for v in names:
        a = H.array(v)
        assert a.shape == (ntraj, nt)
        if not _same_bits(a, O.buf[v]):                       # (the bit patterns first: 134 M entries per variable)
            assert _same(a, O.buf[v]), v
    _check_minmax(H, O, names)
    H.close()


# ------------------------------------------------------------------ 6. minmax
_NAN, _INF = np.float32(np.nan), np.float32(np.inf)
MINMAX_CASES = {
    'only_negative': lambda n, rng: -rng.uniform(1, 50, n).astype(np.float32),
    'signed_zeros': lambda n, rng: np.where(rng.uniform(size=n) < 0.5, np.float32(-0.0), np.float32(0.0)),
    'minus_zero_only': lambda n, rng: np.full(n, -0.0, np.float32),
    'finite_and_both_inf': lambda n, rng: np.concatenate([[_INF, -_INF], rng.standard_normal(n - 2).astype(np.float32)]),
    'only_plus_inf': lambda n, rng: np.where(rng.uniform(size=n) < 0.5, _INF, _NAN),
    'only_minus_inf': lambda n, rng: np.where(rng.uniform(size=n) < 0.5, -_INF, _NAN),
    'one_plus_inf': lambda n, rng: np.concatenate([np.full(n - 1, _NAN), [_INF]]),
    'nothing_written': lambda n, rng: np.full(n, _NAN),
}


@pytest.mark.parametrize('case', sorted(MINMAX_CASES))
def test_minmax_edges(ctx, case):
    """One variable of a 5-variable record (two quads, three padding lanes) holds the case, its neighbours are finite:
    nanmin / nanmax of the oracle's float32 array; NaN, NaN when the variable holds no number."""
    rng = np.random.default_rng(7)
    n = 600
    x = rng.permutation(MINMAX_CASES[case](n, rng)).astype(np.float32)
    names = ['lon', 'lat', ('property', 0), 'z', 'status']
    lon, lat, z = rng.uniform(1, 2, n), rng.uniform(60, 61, n), -rng.uniform(1, 2, n)
    P = ctx.particles(n)
    P.append(lon, lat, z=z)
    P.set_property(0, x)
    st = np.zeros(n, np.int32)
    H = ctx.history(n + 4, 2, names)
    O = HistoryOracle(n + 4, 2, names)
    assert all(np.isnan(H.minmax(v)).all() for v in names)    # nothing recorded yet
    H.record(P, 1)
    O.record(1, np.arange(n), st, {'lon': lon, 'lat': lat, ('property', 0): x, 'z': z, 'status': st})
    with np.errstate(invalid='ignore'):
        olo, ohi = O.minmax(('property', 0))
    want = {'only_plus_inf': (np.inf, np.inf), 'only_minus_inf': (-np.inf, -np.inf), 'one_plus_inf': (np.inf, np.inf),
            'nothing_written': (np.nan, np.nan), 'signed_zeros': (0.0, 0.0), 'minus_zero_only': (0.0, 0.0)}.get(case)
    if want:
        assert _same_scalar(olo, want[0]) and _same_scalar(ohi, want[1]), (olo, ohi)
    lo, hi = H.minmax(('property', 0))
    assert _same_scalar(lo, olo) and _same_scalar(hi, ohi), (case, lo, olo, hi, ohi)
    _check_minmax(H, O, names)
    H.flush()
    H.wait()
    _check(H, O, names)
    H.close()
