"""GPU: the keep ballots of the dense mixing launch formed by the static-layout step launch that runs in front of it
(StepDesc.keep; csrc/odr_kernels.hip.h k_step_grid, k_vmix_keep_scan, k_vmix_keep_fill, k_vmix_dense).  The reference of every
case is the same sequence in the same process with ODR_NO_STEP_KEEP=1 (k_vmix_keep's own pass over z, depth and ssh): lon, lat,
z, status, moving and age equal byte for byte, the sign of a zero in z included, and the counters of the skip and of the dense
launch equal too.  Covered: the element counts around the wave, workgroup, tile and scan-row edges; the surface patterns that
fill, empty and split waves, workgroups and tiles; every term of the predicate as the step launch sees it (elements it lifts to
the sea floor, onto a floor at the surface, a floor above the surface, a NaN depth, -0.0, deactivated elements not yet
compacted); the one-call form, the two-call form and the guarded form, with a guard that fails; on a reader level and between
two, on the 8-level column; every call between the two launches that voids the ballots; the settings that forbid the skip; and
the list of every element, which is not filled.  odr_particles_vmix_keep_stats says which producer every dense launch used."""
import numpy as np
import pytest

import bench
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu

KZ, DEPTH, SSH = 'ocean_vertical_diffusivity', 'sea_floor_depth_below_sea_level', 'sea_surface_height'
NO_STEP_KEEP, NO_SKIP, NO_DENSE = 'ODR_NO_STEP_KEEP', 'ODR_NO_VMIX_SKIP', 'ODR_NO_VMIX_DENSE'
WAVE, WG, TILE = 64, 256, 1024
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 1049125]    # the last: beyond the first row of the scan (1024 tiles)
PATTERNS = ['none', 'all', 'alternate', 'wave', 'workgroup', 'tile', 'last']
ROUTES = ('one', 'two', 'guarded')
FIELDS = ('lon', 'lat', 'z', 'status', 'moving', 'age')
STEP = dict(coastline='previous', store_previous=True, count=False, seafloor=True)


def _world(nz=12, odd_depths=False):
    """C3's readers and bindings (bench.Workload) on a block of 64 x 48 nodes: the static step layouts, and the static mixing
    configuration of 12 levels (two-quad launch) or 8.  odd_depths: bands of latitude whose sea floor is 3 m deep (elements below
    are lifted), at the surface (lifted onto -0.0), 5 m above it, and NaN (with a NaN fallback, so that it reaches the element)."""
    g = synth.grid3d(nx=64, ny=48, nz=nz, nt=3, seed=0)
    if odd_depths:
        d = g[DEPTH].copy()
        d[:, 4:10, :] = 3.0
        d[:, 11:17, :] = 0.0
        d[:, 18:24, :] = -5.0
        d[:, 26:, :] = np.nan        # (to the northern edge: the block preparation fills NaN nodes up to ten rows from a valid one)
        g = dict(g, **{DEPTH: d})
    f = dict(bench.make_fields('c3', small=True), g=g, z=g['z'])
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    wl = bench.Workload('c3', ctx, f, (0, 0, 1), via_torch=False)
    if odd_depths:
        ctx.bind(DEPTH, [wl.sid], np.nan)
        # the Workload compares the levels with ==, which a NaN fails: declare the depth as the same array at every level, as
        # it does for the plain field (the static layout gathers it at one level)
        wl.static_ids[DEPTH] = 1 + f['names'].index(DEPTH)
        for slot in range(3):
            ctx.upload_block(wl.sid, slot, float(g['t'][slot]), {q: g[q][slot] for q in f['names']}, content_ids=wl.static_ids)
    return ctx, wl, g


@pytest.fixture(scope='module')
def world():
    ctx, wl, g = _world()
    yield ctx, wl, g
    ctx.close()


@pytest.fixture(scope='module')
def odd_world():
    ctx, wl, g = _world(odd_depths=True)
    yield ctx, wl, g
    ctx.close()


def _seeds(g, n, pattern, seed=11):
    rng = np.random.default_rng(seed + n)
    lon = rng.uniform(g['x'][4], g['x'][int(0.85 * len(g['x']))], n)
    lat = rng.uniform(g['y'][4], g['y'][-5], n)
    z = -rng.uniform(0.5, 45.0, n)
    k = np.arange(n)
    surface = {'none': np.zeros(n, bool), 'all': np.ones(n, bool), 'alternate': k % 2 == 0, 'wave': (k // WAVE) % 2 == 0,
               'workgroup': (k // WG) % 2 == 0, 'tile': (k // TILE) % 2 == 0, 'last': k == n - 1}[pattern]
    z[surface] = 0.0
    return lon, lat, z


def _run(monkeypatch, world, seeds, route, keep, k=1, between=None, mix=None, env=(), gone=None, step=None, capacity=None):
    """Step k on fresh elements: the step launch and the mixing launch by `route`.  keep=False: ODR_NO_STEP_KEEP=1, the reference.
    between(P, wl): a call between the two launches (route 'two').  Returns the arrays and the statistics."""
    ctx, wl, _ = world
    for name in (NO_STEP_KEEP, NO_SKIP, NO_DENSE):
        monkeypatch.delenv(name, raising=False)
    if not keep:
        monkeypatch.setenv(NO_STEP_KEEP, '1')
    for name in env:
        monkeypatch.setenv(name, '1')
    lon, lat, z = seeds
    n = len(lon)
    mix = dict(mix or {})
    P = ctx.particles(capacity or n)
    try:
        P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
        if gone is not None:
            P.deactivate(gone, 1)            # deactivated, not compacted: the step launch and the mixing launch both see it
        t = wl.time_of(k)
        skw = dict(STEP, age_dt=wl.dt, **(step or {}))
        fell_back = False
        if route == 'one':
            P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, vmix=dict(dt_mix=wl.dt_mix, step=k,
                               vertical_advection=mix.get('fuse_vertical_advection', False),
                               mix_at_surface=mix.get('mix_at_surface', False)), **skw)
        else:
            P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, **skw)
            if between is not None:
                between(P, wl)
            mkw = dict(dict(fuse_vertical_advection=False), **mix)
            if route == 'guarded':
                assert P.scan_status_begin()
                ok = P.vmix(t, wl.dt, wl.dt_mix, step=k, guarded=True, **mkw)
                kept, _ = P.scan_status_end()
                if not (ok and kept == len(P)):
                    fell_back = True
                    P.vmix(t, wl.dt, wl.dt_mix, step=k, **mkw)
            else:
                P.vmix(t, wl.dt, wl.dt_mix, step=k, **mkw)
        out = P.download()
        out['age'] = P.download_f32('age_seconds')
        out['depth'], out['ssh'] = P.env_download(DEPTH), P.env_download(SSH)
        stats = dict(keep=P.vmix_keep_stats(), dense=P.vmix_dense_stats(), skip=P.vmix_skip_stats(), layout=P.step_layout_stats(),
                     onlevel=P.step_onlevel_stats(), vmix=P.vmix_layout_stats(), fell_back=fell_back)
        return out, stats
    finally:
        P.close()


def _same(a, b, what):
    assert len(a['z']) == len(b['z']), what
    if not np.array_equal(a['ID'], b['ID']):     # (a re-sort may order the elements of a cell differently from run to run)
        ia, ib = np.argsort(a['ID'], kind='stable'), np.argsort(b['ID'], kind='stable')
        assert np.array_equal(a['ID'][ia], b['ID'][ib]), what
        a, b = {q: a[q][ia] for q in FIELDS}, {q: b[q][ib] for q in FIELDS}
    for q in FIELDS:
        assert np.ascontiguousarray(a[q]).tobytes() == np.ascontiguousarray(b[q]).tobytes(), (what, q)


def _pair(monkeypatch, world, seeds, route, k=1, from_step=1, from_keep=0, dense=True, **kw):
    """The sequence on the step launch's ballots and on k_vmix_keep's: bytes, counters, and which producer served"""
    a, sa = _run(monkeypatch, world, seeds, route, True, k=k, **kw)
    b, sb = _run(monkeypatch, world, seeds, route, False, k=k, **kw)
    what = (route, len(seeds[0]), k)
    _same(a, b, what)
    # the step launches took a static layout: between two levels (LayoutC3) or on one (LayoutC3L1) -- or the case is void
    on_level = wl_on_level(world, k)
    for s in (sa, sb):
        assert s['layout']['static'] == (0 if on_level else 1) and s['onlevel'] == (1 if on_level else 0), (what, s)
    assert sa['fell_back'] == sb['fell_back'], what
    launches = from_step + from_keep
    assert sa['keep']['from_step'] == from_step and sa['keep']['from_keep'] == from_keep, (what, sa)
    assert sb['keep']['from_step'] == 0 and sb['keep']['from_keep'] == launches, (what, sb)
    assert sa['keep']['identity'] == sb['keep']['identity'], (what, sa, sb)
    assert sa['dense'] == sb['dense'] and sa['skip'] == sb['skip'] and sa['vmix'] == sb['vmix'], (what, sa, sb)
    assert sa['dense']['launches'] == (launches if dense else 0), (what, sa)
    return a, sa


def wl_on_level(world, k):
    wl, g = world[1], world[2]
    return bool(np.any(np.isclose(g['t'], wl.time_of(k))))


@pytest.mark.parametrize('n', SIZES)
def test_step_launch_ballots_change_no_byte(monkeypatch, world, n):
    for pattern in PATTERNS:
        seeds = _seeds(world[2], n, pattern)
        nsurf = int((seeds[2] == 0).sum())
        # (the million elements: every pattern through the one-call form, the other two forms on one pattern)
        for route in (ROUTES if n < 100000 or pattern == 'alternate' else ('one',)):
            a, s = _pair(monkeypatch, world, seeds, route)
            assert not s['fell_back']
            assert s['skip']['skipped'] == nsurf and s['dense']['listed'] == n - nsurf, (n, pattern, route, s)
            assert s['keep']['identity'] == (1 if nsurf == 0 else 0), (n, pattern, route, s)
            assert (a['z'][seeds[2] == 0].view(np.int64) == 0).all(), (n, pattern, route)
            if nsurf < n:
                assert (a['z'][seeds[2] != 0] != seeds[2][seeds[2] != 0]).any(), (n, pattern, route)    # the others were mixed


@pytest.mark.parametrize('route', ROUTES)
def test_list_of_every_element_is_not_filled(monkeypatch, world, route):
    """nothing at the surface: the scan flags the list, the fill returns, thread d mixes element d -- two tiles and a part"""
    seeds = _seeds(world[2], 2 * TILE + 77, 'none')
    a, s = _pair(monkeypatch, world, seeds, route)
    assert s['keep']['identity'] == 1 and s['dense']['listed'] == len(seeds[0]) and s['skip']['skipped'] == 0, s
    assert (a['z'] != seeds[2]).all()


@pytest.mark.parametrize('nz', [12, 8])
@pytest.mark.parametrize('k', [0, 1], ids=['on_level', 'between_levels'])
def test_both_static_layouts_and_both_columns(monkeypatch, world, nz, k):
    w = world if nz == 12 else _world(nz=8)
    try:
        assert wl_on_level(w, k) == (k == 0)
        for n, pattern in ((257, 'alternate'), (2049, 'wave'), (4100, 'last')):
            seeds = _seeds(w[2], n, pattern)
            for route in ROUTES:
                _, s = _pair(monkeypatch, w, seeds, route, k=k)
                assert s['skip']['skipped'] == int((seeds[2] == 0).sum()), (nz, k, n, route, s)
    finally:
        if nz != 12:
            w[0].close()


@pytest.mark.parametrize('route', ROUTES)
def test_every_term_of_the_predicate(monkeypatch, odd_world, route):
    """Elements over the bands of odd sea floors, at the surface, below it and on -0.0: the step launch lifts some to the floor
    (3 m: they are mixed; 0 m: onto -0.0, which the mixing call hands back as +0.0; 5 m above the surface: mixed), and finds a
    NaN depth (skipped at the surface, as the walk leaves it)"""
    g = odd_world[2]
    n = 3 * TILE + 131
    rng = np.random.default_rng(5)
    lon = rng.uniform(g['x'][4], g['x'][int(0.85 * len(g['x']))], n)
    lat = rng.uniform(g['y'][4], g['y'][-5], n)
    z = -rng.uniform(0.5, 45.0, n)
    z[np.arange(n) % 3 == 0] = 0.0
    z[np.arange(n) % 9 == 3] = -0.0
    a, s = _pair(monkeypatch, odd_world, (lon, lat, z), route)
    depth = a['depth']
    with np.errstate(invalid='ignore'):
        floor = -(depth + a['ssh'])
        lifted = z < floor
    # the bands reached the elements as the case needs them (or it tests nothing)
    assert np.isnan(depth).sum() > 50 and (depth < 0).sum() > 50 and (depth == 0).sum() > 50 and (depth == 3).sum() > 50, depth
    assert (lifted & (depth == 3)).sum() > 20 and (lifted & (depth == 0)).sum() > 20
    top = (z == 0) & ~lifted
    assert (np.signbit(z) & top).sum() > 50                      # -0.0 inputs that the step launch left at the surface
    with np.errstate(invalid='ignore'):
        pred = (np.where(lifted, floor.astype(np.float64), z) == 0) & ~(floor > 0)
    # (a floor above the surface never meets z == 0 here: the step launch has lifted the element onto it)
    assert (pred & np.isnan(depth)).any() and (lifted & (floor > 0)).sum() > 20 and not (top & (floor > 0)).any()
    assert s['skip']['skipped'] == int(pred.sum()) and s['dense']['listed'] == n - int(pred.sum()), (s, int(pred.sum()))
    assert (a['z'][pred].view(np.int64) == 0).all()             # +0.0 bit for bit, whatever zero came in or was lifted onto
    assert not pred[lifted & (floor != 0)].any()                 # lifted anywhere but onto the surface: mixed


@pytest.mark.parametrize('route', ROUTES)
def test_deactivated_elements_not_yet_compacted(monkeypatch, world, route):
    seeds = _seeds(world[2], 2049, 'alternate')
    gone = np.arange(2049) % 5 == 0
    if route == 'guarded':
        # the fold finds that not every element stays: the guarded launch does nothing and the loop calls again, unguarded
        a, s = _pair(monkeypatch, world, seeds, route, gone=gone, from_step=1, from_keep=1)
        assert s['fell_back']
    else:
        a, s = _pair(monkeypatch, world, seeds, route, gone=gone)
    assert (a['status'][gone] == 1).all() and (a['status'][~gone] == 0).all()


def test_guard_that_fails_on_an_element_the_step_launch_deactivates(monkeypatch, world):
    """one element seeded on land: the step launch deactivates it, the fold says so, the guarded launch -- which took the step
    launch's ballots -- does nothing, and the unguarded call that follows forms its own"""
    g = world[2]
    lon, lat, z = _seeds(g, 1025, 'alternate')
    lon[700], lat[700] = 0.5 * (g['x'][-2] + g['x'][-1]), g['y'][20]      # inside the coastal strip of the synthetic field
    a, s = _pair(monkeypatch, world, (lon, lat, z), 'guarded', step=dict(seeded_on_land_code=7), from_step=1, from_keep=1)
    assert s['fell_back'] and a['status'][700] == 7 and (np.delete(a['status'], 700) == 0).all()
    assert s['skip']['skipped'] == 513 and s['dense'] == dict(launches=2, listed=512), s      # only the call that ran counted


def _upload_z(P, wl):
    z = P.download()['z']
    z[::3] = 0.0
    z[1::7] = -0.0
    z[2::5] -= 1.0
    P.upload(z=z)


def _compact(P, wl):
    gone = np.zeros(len(P), bool)
    gone[5::11] = True
    P.deactivate(gone, 1)
    P.compact()


def _sort(P, wl):
    P.sort_by_cell(wl.sid, keep_environment=True)


def _append(P, wl):
    k = np.arange(300)
    P.append(np.full(300, 3.0) + 1e-3 * k, np.full(300, 62.0), z=np.where(k % 2 == 0, 0.0, -4.0),
             id=100000 + k.astype(np.int32))


def _mix_first(P, wl):
    P.vmix(wl.time_of(1), wl.dt, wl.dt_mix, step=77, fuse_vertical_advection=False)


def _depth(P, wl):
    d = P.env_download(DEPTH)
    d[::4] = -5.0
    P.env_upload(DEPTH, d)


@pytest.mark.parametrize('between', [_upload_z, _compact, _sort, _append, _depth, _mix_first], ids=lambda f: f.__name__.strip('_'))
def test_calls_that_void_the_ballots(monkeypatch, world, between):
    seeds = _seeds(world[2], 2 * TILE + 300, 'wave')
    first = 1 if between is _mix_first else 0                    # (a mixing call itself: the first takes them, the second may not)
    a, s = _pair(monkeypatch, world, seeds, 'two', between=between, capacity=len(seeds[0]) + 300, from_step=first, from_keep=1)
    assert s['dense']['launches'] == 1 + first and s['skip']['skipped'] > 0, s


@pytest.mark.parametrize('route', ['one', 'two'])
@pytest.mark.parametrize('why', ['mix_at_surface', 'vertical_advection_at_surface', NO_SKIP, NO_DENSE])
def test_settings_that_forbid_the_skip_never_read_the_ballots(monkeypatch, world, route, why):
    seeds = _seeds(world[2], 2049, 'alternate')
    mix = {'mix_at_surface': dict(mix_at_surface=True), 'vertical_advection_at_surface': dict(fuse_vertical_advection=True)}.get(why)
    env = () if mix else (why,)
    a, s = _pair(monkeypatch, world, seeds, route, mix=mix, env=env, from_step=0, from_keep=0, dense=False)
    assert s['dense'] == dict(launches=0, listed=0) and s['keep'] == dict(from_step=0, from_keep=0, identity=0), s
    if why != NO_DENSE:
        assert s['skip']['skipped'] == 0, s
    if mix:
        assert (a['z'][seeds[2] == 0] < 0).any()                 # surface elements do move under these settings
