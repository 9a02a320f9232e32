"""GPU: the bookkeeping kernels every step of every model goes through, at the sizes where their loops, ballots and scans
change shape, against the NumPy reference of tests/bookkeeping_model.py.

  status scan   k_cmp_count, k_cmp_total, k_cmp_scan
  compaction    k_cmp_lists, k_cmp_move (in place), k_cmp_scatter (ODR_ORDERED_COMPACT)
  ID ranks      k_rank_mark, k_rank_count, k_scan_local, k_scan_add, k_rank_assign
  re-sort       k_sort_hist, k_sort_perm, k_gather_perm with key_run

Everything is compared exactly: integers as they are, floats by their bits.  A compaction is compared slot by slot with
`original[model_src]`; only the re-sort, whose order inside a bin is decided by atomics, is compared through the IDs.  W is
the wave size and B the default ODR_BLOCK: 4B is one pass of k_cmp_count, 1024B the row boundary of k_cmp_scan, 8192B its
8-row batch boundary and the grid-stride wrap of k_cmp_count's 2048 workgroups.  The sequential fallback of k_cmp_scan
(more than 256 x 1024 chunks) needs more than 67 M elements: out of reach of a test that takes seconds, and not built here.

plon / plat have no download of their own: _previous() reads them through the product (coastline action 'previous' puts an
element on land back there), as the last thing a test does with a particle set."""
import numpy as np
import pytest

import bookkeeping_model as bm
from opendrift_amd import _abi
from opendrift_amd import synthetic as synth
from opendrift_amd._abi import OdrError
from scenarios import Scenario

pytestmark = pytest.mark.gpu

W, B = 64, 256
U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
WVEL, KZ = 'upward_sea_water_velocity', 'ocean_vertical_diffusivity'
DEPTH, SSH, LAND = 'sea_floor_depth_below_sea_level', 'sea_surface_height', 'land_binary_mask'
F32 = ('wind_drift_factor', 'current_drift_factor', 'terminal_velocity', 'age_seconds')
ENV2 = ('sea_water_temperature', 'sea_water_salinity')     # two uploaded environment variables
SLOTS2 = (2, 6)                                            # two property slots
NVAR = len(_abi.VARIABLES)
MODES = ['in_place', 'ordered']


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _set_mode(monkeypatch, mode):
    if mode == 'ordered':
        monkeypatch.setenv('ODR_ORDERED_COMPACT', '1')     # (the library reads it on every call)
    else:
        monkeypatch.delenv('ODR_ORDERED_COMPACT', raising=False)


# ------------------------------------------------------------------ the carried state
def _lon0(ids):
    return 2.0 + np.asarray(ids, dtype=np.float64) * 1e-6


def _lat0(ids):
    return 55.0 + np.asarray(ids, dtype=np.float64) * 5e-7


def _env_value(ids, v):
    """what environment variable / property slot number v holds for an ID: float32(ID) or a fixed function of it"""
    f = np.asarray(ids).astype(np.float32)
    return f if v == 0 else (f * np.float32(0.5) + np.float32(v)).astype(np.float32)


def _append(P, ids, explicit=True):
    """The elements `ids` in three batches that age between them: lon, lat, z, the drift factors and the terminal velocity are
    distinct per ID, age_seconds differs from batch to batch.  plon / plat are the appended lon / lat."""
    n = len(ids)
    f = np.asarray(ids).astype(np.float32)
    cuts = [0, n // 3, 2 * n // 3, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b == a:
            continue
        s = slice(a, b)
        P.append(_lon0(ids[s]), _lat0(ids[s]), z=-0.5 * ids[s], id=ids[s].astype(np.int32) if explicit else None,
                 wind_drift_factor=f[s] * np.float32(0.25), current_drift_factor=f[s] + np.float32(0.5),
                 terminal_velocity=-f[s])
        P.increase_age(100.0)


def _dress(P, env, slots):
    """positions moved away from the previous ones, moving, the environment variables and the property slots of every element"""
    ids = P.ids()
    n = len(ids)
    P.update_positions(0.1 + 0.01 * (ids % 7), np.full(n, -0.2), 600.0)
    P.upload(moving=(ids % 3 != 0).astype(np.int32))
    for k, v in enumerate(env):
        P.env_upload(v, _env_value(ids, k))
    for k, s in enumerate(slots):
        P.set_property(s, _env_value(ids, k + len(env)))


def _snapshot(P, env, slots):
    d = P.download()
    for k in F32:
        d[k] = P.download_f32(k)
    for v in env:
        d['env:%s' % v] = P.env_download(v)
    for s in slots:
        d['slot:%d' % s] = P.get_property(s)
    return d


def _previous(P):
    """(plon, plat) of every slot.  Overwrites lon, lat and the sampled land mask."""
    P.env_upload(LAND, np.ones(len(P), np.float32))
    P.coastline('previous')
    d = P.download()
    return d['lon'], d['lat']


def _deactivate(P, remove, codes=(11, 12)):
    """two status codes, by the parity of the index: the deactivated store has a status column worth comparing"""
    idx = np.arange(len(remove))
    for k, code in enumerate(codes):
        m = remove & (idx % len(codes) == k)
        if m.any():
            P.deactivate(m, code)


STORE_KEYS = ('ID', 'lon', 'lat', 'z', 'status')


def _empty_store():
    return dict(ID=np.empty(0, np.int32), lon=np.empty(0), lat=np.empty(0), z=np.empty(0), status=np.empty(0, np.int32))


def _check_compaction(P, env, slots, mode, store, what, apply=False):
    """One compaction against the model: the count, len(P), every array slot by slot, the deactivated store (the model's
    accumulated `store` + this round's), and a second compaction that changes nothing.  Returns (after, store)."""
    before = _snapshot(P, env, slots)
    src, dead_src = (bm.compact_ordered if mode == 'ordered' else bm.compact_in_place)(before['status'])
    store = {k: np.concatenate([store[k], before[k][dead_src]]) for k in STORE_KEYS}
    kept = P.compact_apply() if apply else P.compact()
    assert kept == len(src), what
    assert len(P) == len(src) and P.count() == (len(src), len(store['ID'])), what
    after = _snapshot(P, env, slots)
    assert after.keys() == before.keys()
    for k in before:
        assert _same_bits(after[k], before[k][src]), (what, k)
    dead = P.download_deactivated()
    for k in STORE_KEYS:
        assert _same_bits(dead[k], store[k]), (what, 'deactivated', k)
    assert P.compact() == kept, what
    again, dead2 = _snapshot(P, env, slots), P.download_deactivated()
    for k in after:
        assert _same_bits(again[k], after[k]), (what, 'second compaction', k)
    for k in STORE_KEYS:
        assert _same_bits(dead2[k], store[k]), (what, 'second compaction, deactivated', k)
    return after, store


def _check_previous(P, what):
    ids = P.ids()
    plon, plat = _previous(P)
    assert _same_bits(plon, _lon0(ids)) and _same_bits(plat, _lat0(ids)), (what, 'plon / plat')


# ------------------------------------------------------------------ a. compaction
PATTERNS = ['nobody', 'everybody', 'first', 'last', 'all_but_last', 'first_half', 'second_half', 'alternating', 'one_wave',
            'one_chunk', 'ragged_wave', 'random_1', 'random_50', 'random_99']
LARGE_PATTERNS = ['first_half', 'second_half', 'alternating', 'random_50']
SMALL_SIZES = [1, 2, W - 1, W, W + 1, B - 1, B, B + 1, 4 * B - 1, 4 * B, 4 * B + 1]
LARGE_SIZES = [1024 * B - 1, 1024 * B, 1024 * B + 1, 8192 * B - 1, 8192 * B, 8192 * B + 1]


def _removal(pattern, n, rng):
    r = np.zeros(n, bool)
    if pattern == 'everybody':
        r[:] = True
    elif pattern == 'first':
        r[0] = True
    elif pattern == 'last':
        r[-1] = True
    elif pattern == 'all_but_last':
        r[:-1] = True
    elif pattern == 'first_half':        # every head slot a hole, every tail element a fill
        r[:n // 2] = True
    elif pattern == 'second_half':       # nothing moves
        r[n - n // 2:] = True
    elif pattern == 'alternating':
        r[::2] = True
    elif pattern == 'one_wave':          # exactly one whole wave, in the middle
        lo = (n // W // 2) * W
        r[lo:lo + W] = True
    elif pattern == 'one_chunk':
        lo = (n // B // 2) * B
        r[lo:lo + B] = True
    elif pattern == 'ragged_wave':       # the last wave, ragged unless n is a multiple of W
        r[(n - 1) // W * W:] = True
    elif pattern.startswith('random_'):
        r = rng.uniform(size=n) < int(pattern[7:]) / 100.0
    else:
        assert pattern == 'nobody'
    return r


def _compaction_case(ctx, mode, n, pattern, rng):
    what = (mode, n, pattern)
    ids = np.arange(n)
    P = ctx.particles(n)
    _append(P, ids)
    P.store_previous()
    _dress(P, ENV2, SLOTS2)
    remove = _removal(pattern, n, rng)
    _deactivate(P, remove)
    after, _ = _check_compaction(P, ENV2, SLOTS2, mode, _empty_store(), what)
    assert len(after['ID']) == n - int(remove.sum()), what
    assert (after['status'] == 0).all(), what
    assert not _same_bits(after['lon'], _lon0(after['ID'])) or len(after['ID']) == 0    # (the positions did move)
    assert _same_bits(after['env:' + ENV2[0]], after['ID'].astype(np.float32)), what
    _check_previous(P, what)
    P.close()


@pytest.mark.parametrize('n', SMALL_SIZES)
@pytest.mark.parametrize('mode', MODES)
def test_compaction_every_pattern(ctx, monkeypatch, mode, n):
    _set_mode(monkeypatch, mode)
    rng = np.random.default_rng(n)
    for pattern in PATTERNS:
        _compaction_case(ctx, mode, n, pattern, rng)


@pytest.mark.parametrize('n', LARGE_SIZES)
@pytest.mark.parametrize('mode', MODES)
def test_compaction_at_the_scan_rows(ctx, monkeypatch, mode, n):
    _set_mode(monkeypatch, mode)
    rng = np.random.default_rng(n)
    for pattern in LARGE_PATTERNS:
        _compaction_case(ctx, mode, n, pattern, rng)


# ------------------------------------------------------------------ b. a sequence
@pytest.mark.parametrize('mode', MODES)
def test_compaction_sequence(ctx, monkeypatch, mode):
    """compact, append without IDs, deactivate with another code, compact, and a third round: dead_base > 0 and an arbitrary
    starting order"""
    _set_mode(monkeypatch, mode)
    rng = np.random.default_rng(17)
    P = ctx.particles(4000)
    store = _empty_store()
    next_id = 0
    rounds = ((4 * B + 1, 'random_50', (11, 12)), (700, 'random_50', (13, )), (300, 'alternating', (14, 15)), (W + 1, 'first_half', (16, )))
    for k, (more, pattern, codes) in enumerate(rounds):
        n0 = len(P)
        _append(P, np.arange(next_id, next_id + more), explicit=False)
        got = P.ids()
        assert np.array_equal(got[n0:], np.arange(next_id, next_id + more)), k      # new IDs continue at active + deactivated
        next_id += more
        _dress(P, ENV2, SLOTS2)
        _deactivate(P, _removal(pattern, len(P), rng), codes)
        after, store = _check_compaction(P, ENV2, SLOTS2, mode, store, (mode, 'round', k))
        assert len(after['ID']) + len(store['ID']) == next_id
        assert _same_bits(after['env:' + ENV2[1]], _env_value(after['ID'], 1)), k
    assert np.array_equal(np.sort(np.concatenate([after['ID'], store['ID']])), np.arange(next_id))
    if mode == 'in_place':
        assert (np.diff(after['ID']) < 0).any()          # (the later rounds did start from a permuted order)
    _check_previous(P, (mode, 'sequence'))
    P.close()


# ------------------------------------------------------------------ g. re-sort (its helpers are used by c.)
def _sort_grid(ctx, ny, nx):
    x, y = np.arange(nx, dtype=np.float64), 50.0 + np.arange(ny, dtype=np.float64)
    sid = ctx.add_grid(x, y, lon_mode=2)
    ctx.upload_block(sid, 0, 0.0, {U: np.zeros((ny, nx), np.float32)})
    return dict(sid=sid, x=x, y=y, ny=ny, nx=nx)


def _check_sort(P, g, env, slots, keep_environment, what):
    """keys non-decreasing, the IDs a permutation of the input, every carried array follows its ID bit for bit"""
    before = _snapshot(P, env, slots)
    P.sort_by_cell(g['sid'], keep_environment=keep_environment)
    after = _snapshot(P, env if keep_environment else (), slots)
    assert len(P) == len(before['ID']), what
    keys = bm.cell_keys(g['x'], g['y'], after['lon'], after['lat'])
    assert (np.diff(keys) >= 0).all(), (what, int((np.diff(keys) < 0).sum()))
    ob = np.argsort(before['ID'], kind='stable')
    assert np.array_equal(before['ID'][ob], np.sort(after['ID'])), what
    came_from = ob[np.searchsorted(before['ID'][ob], after['ID'])]      # the slot the element of slot j sat in
    for k in after:
        assert _same_bits(after[k], before[k][came_from]), (what, k)
    return after, keys


SORT_INPUTS = ['sorted', 'one_cell', 'two_cells', 'runs_of_3', 'all_outside', 'half_outside', 'last_row_and_column']
SORT_SIZES = [2, 3, W - 1, W, W + 1, B + 1, 8 * B - 1, 8 * B, 8 * B + 1, 9 * B + 5]


def _sort_positions(g, kind, n, rng):
    """(lon, lat): cell centres with a per-element offset inside the cell (positions stay distinct)"""
    nx, ny = g['nx'], g['ny']
    cx, cy = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    cx, cy = cx.ravel(), cy.ravel()
    order = np.argsort(bm.cell_keys(g['x'], g['y'], g['x'][0] + cx + 0.5, g['y'][0] + cy + 0.5), kind='stable')
    cx, cy = cx[order], cy[order]                              # the cells in key order
    i = np.arange(n)
    outside = np.zeros(n, bool)
    if kind == 'sorted':                                       # runs of 64 equal keys: one run per wave
        c = i // W
    elif kind == 'one_cell':
        c = np.full(n, len(cx) // 2)
    elif kind == 'two_cells':                                  # alternating lane by lane
        c = np.where(i % 2 == 0, 5, len(cx) - 7)
    elif kind == 'runs_of_3':
        c = rng.integers(0, len(cx), n // 3 + 1)[i // 3]
    elif kind == 'all_outside':
        c, outside = np.zeros(n, int), np.ones(n, bool)
    elif kind == 'half_outside':
        c, outside = rng.integers(0, len(cx), n), rng.uniform(size=n) < 0.5
    else:
        c = rng.integers(0, len(cx), n)
    off = 0.25 + 0.5 * (i + 1.0) / (n + 2.0)
    lon, lat = g['x'][0] + cx[c] + off, g['y'][0] + cy[c] + off
    lon[outside] += nx + 3.0
    if kind == 'last_row_and_column':
        j = n // 2
        lon[j], lat[j] = g['x'][-1], g['y'][-1]                # xi == nx - 1, yi == ny - 1: inside, in the last cell
        assert bm.cell_keys(g['x'], g['y'], lon[j:j + 1], lat[j:j + 1])[0] < bm.sort_bins(ny, nx) - 1
    return lon, lat


def _sort_set(ctx, n, lon, lat, rng):
    """ids in shuffled memory order; plon / plat (the appended positions) differ from the uploaded lon / lat"""
    ids = rng.permutation(n)
    P = ctx.particles(max(n, 1))
    _append(P, ids)
    P.store_previous()
    P.upload(lon=lon, lat=lat, moving=(ids % 3 != 0).astype(np.int32))
    for k, v in enumerate(ENV2):
        P.env_upload(v, _env_value(ids, k))
    for k, s in enumerate(SLOTS2):
        P.set_property(s, _env_value(ids, k + len(ENV2)))
    return P


@pytest.mark.parametrize('keep_environment', [True, False], ids=['with_env', 'without_env'])
@pytest.mark.parametrize('shape', [(16, 24), (40, 40)], ids=['385_bins', '1601_bins'])
def test_sort_by_cell(ctx, shape, keep_environment):
    g = _sort_grid(ctx, *shape)
    assert bm.sort_bins(g['ny'], g['nx']) == {(16, 24): 385, (40, 40): 1601}[shape]       # one and two scan blocks of 1024 bins
    rng = np.random.default_rng(shape[0])
    for kind in SORT_INPUTS:
        for n in SORT_SIZES:
            what = (shape, kind, n)
            lon, lat = _sort_positions(g, kind, n, rng)
            P = _sort_set(ctx, n, lon, lat, rng)
            after, keys = _check_sort(P, g, ENV2, SLOTS2, keep_environment, what)
            nkeys = len(np.unique(keys))
            if kind in ('one_cell', 'all_outside'):
                assert nkeys == 1, what
            elif kind == 'two_cells':
                assert nkeys == 2, what
            elif kind == 'sorted':
                assert nkeys == (n + W - 1) // W, what
            if kind == 'all_outside':
                assert (keys == bm.sort_bins(g['ny'], g['nx']) - 1).all(), what
            _check_previous(P, what)
            P.close()


def test_sort_by_cell_of_one_element(ctx):
    g = _sort_grid(ctx, 16, 24)
    P = _sort_set(ctx, 1, np.array([3.5]), np.array([52.5]), np.random.default_rng(0))
    before = _snapshot(P, ENV2, SLOTS2)
    P.sort_by_cell(g['sid'])
    after = _snapshot(P, ENV2, SLOTS2)
    for k in before:
        assert _same_bits(before[k], after[k]), k
    _check_previous(P, 'n = 1')
    P.close()


# ------------------------------------------------------------------ c. every environment variable and every slot
@pytest.mark.parametrize('mode', MODES)
def test_compaction_and_sort_of_the_fullest_set(ctx, monkeypatch, mode):
    """All NVAR environment variables and all nine property slots: 3 + 4 + NVAR + 9 arrays of 32 bits, the capacity of
    CmpArrays (it was 40 once, and the arrays past it were written outside the struct)."""
    _set_mode(monkeypatch, mode)
    env, slots = tuple(range(NVAR)), tuple(range(9))
    assert 3 + 4 + len(env) + len(slots) == 42
    g = _sort_grid(ctx, 16, 24)
    n = 4 * B + 1
    rng = np.random.default_rng(42)
    P = ctx.particles(n)
    _append(P, np.arange(n))
    P.store_previous()
    _dress(P, env, slots)
    _deactivate(P, _removal('random_50', n, rng))
    what = (mode, 'fullest set')
    after, store = _check_compaction(P, env, slots, mode, _empty_store(), what)
    ids = after['ID']
    assert 0 < len(ids) < n and np.array_equal(np.sort(np.concatenate([ids, store['ID']])), np.arange(n))
    for k, v in enumerate(env):
        assert _same_bits(after['env:%s' % v], _env_value(ids, k)), (what, v)
    for k, s in enumerate(slots):
        assert _same_bits(after['slot:%d' % s], _env_value(ids, k + len(env))), (what, s)
    lon, lat = _sort_positions(g, 'runs_of_3', len(ids), rng)
    P.upload(lon=lon, lat=lat)
    after, keys = _check_sort(P, g, env, slots, True, what)
    assert len(np.unique(keys)) > 100
    ids = after['ID']
    for k, v in enumerate(env):
        assert _same_bits(after['env:%s' % v], _env_value(ids, k)), (what, 'sorted', v)
    for k, s in enumerate(slots):
        assert _same_bits(after['slot:%d' % s], _env_value(ids, k + len(env))), (what, 'sorted', s)
    _check_previous(P, what)
    P.close()


# ------------------------------------------------------------------ d. status bookkeeping
CODES = np.array([0, 1, 2, 99, 100, 101, 131, 163, 164], dtype=np.int32)


def _set_status(P, st):
    for c in np.unique(st):
        if c != 0:
            P.deactivate(st == c, int(c))


@pytest.mark.parametrize('n', [W + 1, 4 * B + 1, 1024 * B + 1])
def test_status_scan_count_and_remap(ctx, n):
    rng = np.random.default_rng(n)
    st = CODES[rng.permutation(n) % len(CODES)]              # every code is present at every size
    P = ctx.particles(n)
    P.append(_lon0(np.arange(n)), _lat0(np.arange(n)))
    _set_status(P, st)
    assert np.array_equal(P.download()['status'], st)
    flags = bm.status_flags(st)
    assert flags == 1 | 2 | 1 << 31 | 1 << 63
    assert P.scan_status() == (int((st == 0).sum()), flags)
    for c in list(CODES) + [3, 7, 130, 132]:
        assert P.count_status(int(c)) == int((st == c).sum()), c
    P.remap_status(131, 3)
    st = np.where(st == 131, 3, st).astype(np.int32)
    assert np.array_equal(P.download()['status'], st)
    assert P.scan_status() == (int((st == 0).sum()), flags & ~(1 << 31))
    assert P.count_status(131) == 0 and P.count_status(3) == int((st == 3).sum())
    # elements deactivated after the scan: its counts no longer describe the set
    one = np.zeros(n, bool)
    one[np.nonzero(st == 0)[0][-1]] = True
    P.deactivate(one, 5)
    with pytest.raises(OdrError) as e:
        P.compact_apply()
    assert e.value.code == -4                                  # ODR_ERR_STATE
    st[one] = 5
    assert len(P) == n and np.array_equal(P.download()['status'], st)
    _check_compaction(P, (), (), 'in_place', _empty_store(), ('status', n))
    P.close()


def test_status_flags_ignore_the_codes_outside_100_to_163(ctx):
    n = W + 1
    st = np.array([0, 99, 164, 1], np.int32)[np.arange(n) % 4]
    P = ctx.particles(n)
    P.append(_lon0(np.arange(n)), _lat0(np.arange(n)))
    _set_status(P, st)
    assert P.scan_status() == (int((st == 0).sum()), 0)
    for k in (0, 1, 31, 32, 62, 63):                           # one reason at a time: its bit and no other
        P.remap_status(164 if k == 0 else 100 + prev, 100 + k)
        prev = k
        assert P.scan_status() == (int((st == 0).sum()), 1 << k), k
    P.close()


# ------------------------------------------------------------------ e. the fold of the step launch's counts
STEP_VARIABLES = [U, V, WVEL, DEPTH, SSH, LAND]


@pytest.mark.parametrize('n', [W + 1, 3 * W, 4 * W, 4 * W + 1, B + 1, 2 * B, 4 * B + 1, 1024 * B + 1])
def test_fold_of_the_step_counts(ctx, n):
    """k_cmp_total: the counts one env_coast_advect left per wave, folded into the per-chunk counts of the compaction; the
    wave counts here are and are not multiples of the four a chunk holds"""
    g = synth.grid3d(nx=96, ny=80, nz=8, nt=3, seed=5, coast=True)
    names = [U, V, WVEL, KZ, DEPTH, LAND]
    levels = [(float(g['t'][k]), {v: g[v][k] for v in names}) for k in range(3)]
    Scenario([('grid', dict(x=g['x'], y=g['y'], z=g['z'], levels=levels))],
             fallbacks={U: 0.0, V: 0.0, WVEL: 0.0, KZ: 0.0, DEPTH: 10000.0, SSH: 0.0}).device(ctx)
    rng = np.random.default_rng(n)
    strand = rng.uniform(size=n) < 0.3
    strand[0], strand[-1] = False, True
    strand[W:2 * W] = True                                    # one whole wave goes
    x, y = g['x'].astype(np.float64), g['y'].astype(np.float64)
    assert (g[LAND][0][:, -2] == 1).all() and (g[LAND][0][:, :int(0.88 * len(x))] == 0).all()
    lon = np.where(strand, x[-2], rng.uniform(x[8], x[int(0.85 * len(x))], n))
    lat = rng.uniform(y[2], y[-3], n)
    P = ctx.particles(n)
    P.append(lon, lat, z=np.where(np.arange(n) % 2 == 0, 0.0, -5.0))
    P.store_previous()
    hit = P.env_coast_advect(STEP_VARIABLES, 0.0, 'runge-kutta4', 600.0, coastline='stranding', stranded_code=1,
                             store_previous=True)
    assert hit == int(strand.sum()) and 0 < hit < n
    assert P.scan_status_begin()                               # the path under test ran
    d = P.download()
    kept, flags = P.scan_status_end()
    assert np.array_equal(d['status'] != 0, strand)
    assert (kept, flags) == (int((d['status'] == 0).sum()), 0)
    assert 0 < kept < n                                        # some but not all strand
    after, store = _check_compaction(P, STEP_VARIABLES, (), 'in_place', _empty_store(), ('fold', n), apply=True)
    assert np.array_equal(np.sort(store['ID']), np.nonzero(strand)[0])
    P.close()


# ------------------------------------------------------------------ f. ranks
MEMBERS_U, MEMBERS_V = 1024, 1023


def _rank_world(ctx):
    """One geographic grid that covers every element; member m of the current's x component is the constant m (1024
    members), of its y component too (1023 members): a sample at a grid node is float32(rank % members), and the pair fixes
    every rank below 1024 * 1023."""
    x, y = np.arange(6, dtype=np.float64), 60.0 + np.arange(6, dtype=np.float64)
    sid = ctx.add_grid(x, y, lon_mode=2)
    ctx.upload_block(sid, 0, 0.0, {U: [np.full((6, 6), m, np.float32) for m in range(MEMBERS_U)],
                                   V: [np.full((6, 6), m, np.float32) for m in range(MEMBERS_V)]})
    ctx.bind(U, [sid], 0.0)
    ctx.bind(V, [sid], 0.0)


def _rank_set(ctx, ids):
    ids = np.asarray(ids, dtype=np.int64)
    assert len(np.unique(ids)) == len(ids)
    P = ctx.particles(len(ids))
    P.append(1.0 + ids % 4, 61.0 + (ids // 4) % 4, id=ids.astype(np.int32))      # on interior grid nodes
    return P


def _check_ranks(P, what):
    d = P.download()
    active = d['status'] == 0
    got = P.env_sample([U, V], 0.0, download=True)
    want = bm.ranks(d['ID'], active)
    assert np.array_equal(np.sort(want[active]), np.arange(int(active.sum())))
    assert _same_bits(got[U][active], (want[active] % MEMBERS_U).astype(np.float32)), what
    assert _same_bits(got[V][active], (want[active] % MEMBERS_V).astype(np.float32)), what
    return want[active]


def _ids_up_to(top, rng, n=3000):
    """distinct IDs in [0, top] in shuffled order, with 0 and top among them"""
    n = min(n, top + 1)
    ids = np.concatenate([[0, top], 1 + rng.choice(top - 1, size=n - 2, replace=False)])
    return rng.permutation(ids)


RANK_TOPS = [31, 32, 32767, 32768, 32769, 1048575, 1048576, 33554431, 33554432]


@pytest.mark.parametrize('top', RANK_TOPS)
def test_ranks_up_to_an_id(ctx, top):
    """32 IDs per word, 1024 words per block of k_scan_local (32 768 IDs), 1024 block sums per row of k_cmp_scan (33 554 432)"""
    _rank_world(ctx)
    P = _rank_set(ctx, _ids_up_to(top, np.random.default_rng(top)))
    r = _check_ranks(P, top)
    assert r.max() == len(P) - 1 and (len(P) <= MEMBERS_U or r.max() >= MEMBERS_U)
    P.close()


def test_ranks_of_dense_and_sparse_ids(ctx):
    _rank_world(ctx)
    rng = np.random.default_rng(5)
    k = rng.choice(40000, size=1500, replace=False)
    cases = {'dense, shuffled': rng.permutation(3000),
             'sparse': rng.choice(200000, size=3000, replace=False),
             'bit 0 and bit 31 of the words': rng.permutation(np.concatenate([32 * k, 32 * k + 31]))}
    for what, ids in cases.items():
        P = _rank_set(ctx, ids)
        _check_ranks(P, what)
        P.close()


@pytest.mark.parametrize('mode', MODES)
def test_ranks_count_the_active_elements_only(ctx, monkeypatch, mode):
    """deactivated but not yet compacted: not counted; after the compaction that removed every third ID: the same ranks"""
    _set_mode(monkeypatch, mode)
    _rank_world(ctx)
    rng = np.random.default_rng(6)
    P = _rank_set(ctx, _ids_up_to(32769, rng))
    ids = P.ids()
    P.deactivate(ids % 3 == 0, 9)
    before = _check_ranks(P, 'before the compaction')
    assert len(before) == int((ids % 3 != 0).sum()) < len(ids)
    P.compact()
    assert len(P) == len(before)
    after = _check_ranks(P, 'after the compaction')
    assert np.array_equal(np.sort(P.ids()), np.sort(ids[ids % 3 != 0]))
    assert np.array_equal(np.sort(after), np.sort(before))
    P.close()
