"""GPU: the dense mixing launch (k_vmix_keep, k_vmix_keep_scan, k_vmix_keep_fill, k_vmix_dense; csrc/odr_kernels.hip.h) -- a
static configuration whose settings allow the surface skip builds ONE list of the elements to mix over the whole launch and runs
the one-element-per-thread routine over it.  Byte for byte it computes what the tiled launch computes (ODR_NO_VMIX_DENSE=1:
compaction per 1024-element tile) and what the launch computes that skips nothing (ODR_NO_VMIX_SKIP=1): at the sizes around the
wave, workgroup and tile edges, for the patterns that fill, empty and split waves and tiles, with -0.0, negative and NaN depths,
on a reader level and between two, on the 8-level column, through the redo path of the two-quad launch, and in the guarded
launch -- which, when it may not run, changes no byte and moves no counter.  odr_particles_vmix_dense_stats counts the launches
and the elements listed: n minus the NumPy count of the predicate.  Settings that forbid the skip, and host uniforms, never take
the dense launch."""
import numpy as np
import pytest

import bench
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu

KZ, DEPTH, SSH = 'ocean_vertical_diffusivity', 'sea_floor_depth_below_sea_level', 'sea_surface_height'
NO_DENSE, NO_SKIP = 'ODR_NO_VMIX_DENSE', 'ODR_NO_VMIX_SKIP'
MODES = ('dense', 'tiled', 'noskip')
TILE = 1024
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4100]
PATTERNS = ['none', 'all', 'alternate', 'wave', 'tile_last']
FIELDS = ('z', 'moving', 'status', 'lon', 'lat')


def _world(kscale=1, nz=12):
    """C3's readers and bindings (bench.Workload) on a block of 64 x 48 nodes: 12 levels -> the static two-quad launch (VMixC3W),
    8 levels -> the static whole-column launch of two quads (VMixC3, NQ = 2)"""
    g = synth.grid3d(nx=64, ny=48, nz=nz, nt=3, seed=0)
    if kscale != 1:
        g = dict(g, **{KZ: g[KZ] * np.float32(kscale)})
    f = dict(bench.make_fields('c3', small=True), g=g, z=g['z'])
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    return ctx, bench.Workload('c3', ctx, f, (0, 0, 1), via_torch=False), g


@pytest.fixture(scope='module')
def world():
    ctx, wl, g = _world()
    yield ctx, wl, g
    ctx.close()


def _seeds(g, n, pattern, seed=11):
    rng = np.random.default_rng(seed + n)
    lon = rng.uniform(g['x'][4], g['x'][int(0.85 * len(g['x']))], n)
    lat = rng.uniform(g['y'][4], g['y'][-5], n)
    z = -rng.uniform(0.5, 45.0, n)
    k = np.arange(n)
    surface = {'none': np.zeros(n, bool), 'all': np.ones(n, bool), 'alternate': k % 2 == 0, 'wave': (k // 64) % 2 == 0,
               'tile_last': (k % TILE == TILE - 1) | (k == n - 1)}[pattern]
    z[surface] = 0.0
    return lon, lat, z


def _set_mode(monkeypatch, mode):
    monkeypatch.delenv(NO_DENSE, raising=False)
    monkeypatch.delenv(NO_SKIP, raising=False)
    if mode == 'tiled':
        monkeypatch.setenv(NO_DENSE, '1')
    elif mode == 'noskip':
        monkeypatch.setenv(NO_SKIP, '1')


def _stats(P):
    return dict(skip=P.vmix_skip_stats(), layout=P.vmix_layout_stats(), window=P.vmix_window_stats(), dense=P.vmix_dense_stats())


def _once(monkeypatch, world, seeds, k, mode, depth=None, guarded=False, **mix):
    """One step launch and one mixing launch of step k on fresh elements.  Returns the download, the NumPy count of the skip
    predicate on what the mixing launch read, the predicate, z on entry, and the statistics."""
    ctx, wl, _ = world
    _set_mode(monkeypatch, mode)
    lon, lat, z = seeds
    n = len(lon)
    P = ctx.particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    t = wl.time_of(k)
    P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False, seafloor=True,
                       age_dt=wl.dt)
    if depth is not None:
        P.env_upload(DEPTH, depth)
    z_in = P.download()['z'].copy()
    with np.errstate(invalid='ignore'):
        zmin = np.float32(-1) * (P.env_download(DEPTH) + P.env_download(SSH))      # float32, as the walk forms it
        pred = (z_in == 0) & ~(zmin > 0)
    if guarded:
        assert P.scan_status_begin()
        assert P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False, guarded=True)
        kept, _ = P.scan_status_end()
        assert kept == n                                   # every element stays: the guarded launch ran
    else:
        P.vmix(t, wl.dt, wl.dt_mix, step=k, **dict(dict(fuse_vertical_advection=False), **mix))
    out = P.download()
    stats = _stats(P)
    P.close()
    return out, int(pred.sum()), pred, z_in, stats


def _same(a, b):
    for q in FIELDS:
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), q


def _triple(monkeypatch, world, seeds, k=1, dense=True, may_skip=True, static=True, windowed=True, **kw):
    """The same step through the dense launch, the tiled launch and the launch that skips nothing: bytes and counters"""
    n = len(seeds[0])
    runs = {m: _once(monkeypatch, world, seeds, k, m, **kw) for m in MODES}
    a, count, pred, z_in, sa = runs['dense']
    for m in ('tiled', 'noskip'):
        assert runs[m][1] == count
        _same(a, runs[m][0])
    sb, sc = runs['tiled'][4], runs['noskip'][4]
    assert sa['skip'] == sb['skip'] == dict(launches=1, skipped=count if may_skip else 0), (sa, sb, count)
    assert sc['skip'] == dict(launches=1, skipped=0), sc
    assert sa['dense'] == (dict(launches=1, listed=n - count) if dense else dict(launches=0, listed=0)), (sa, n, count)
    assert sb['dense'] == sc['dense'] == dict(launches=0, listed=0), (sb, sc)
    want = dict(runtime=0, static=1, other=0) if static else dict(runtime=1, static=0, other=0)
    assert sa['layout'] == sb['layout'] == sc['layout'] == want, (sa, sb, sc)
    for s in (sa, sb, sc):
        assert s['window']['windowed'] == (1 if static and windowed else 0) and s['window']['full'] == 0, s
    assert sa['window'] == sb['window'], (sa, sb)        # (the redone elements too: both launches mix the same elements)
    if may_skip:
        assert (a['z'][pred].view(np.int64) == 0).all()      # +0.0, bit for bit
    return a, count, pred, z_in, sa


@pytest.mark.parametrize('n', SIZES)
def test_dense_launch_changes_no_byte(monkeypatch, world, n):
    for pattern in PATTERNS:
        seeds = _seeds(world[2], n, pattern)
        a, count, pred, z_in, sa = _triple(monkeypatch, world, seeds)
        assert count == int((seeds[2] == 0).sum()), pattern         # (the sea floor is at 50 m or below: every surface element)
        if pattern == 'all':
            assert sa['dense']['listed'] == 0 and (a['z'].view(np.int64) == 0).all()   # every workgroup returned
        if pattern == 'none':
            assert sa['dense']['listed'] == n                       # every element listed, every one mixed as without a list
        if count < n:
            assert not np.array_equal(a['z'][~pred], z_in[~pred]), pattern    # the others were mixed


@pytest.mark.parametrize('k', [0, 1], ids=['on_level', 'between_levels'])
def test_on_a_reader_level_and_between_two(monkeypatch, world, k):
    _, count, _, _, _ = _triple(monkeypatch, world, _seeds(world[2], 2049, 'alternate'), k=k)
    assert count == 1025


def test_negative_zero_comes_out_as_positive_zero(monkeypatch, world):
    lon, lat, z = _seeds(world[2], 1025, 'alternate')
    neg = np.arange(1025) % 6 == 0
    z[neg] = -0.0
    assert np.signbit(z[neg]).all()
    a, count, pred, z_in, _ = _triple(monkeypatch, world, (lon, lat, z))
    assert np.signbit(z_in[neg]).all()                   # the mixing launch read -0.0
    assert count == 513 and pred[neg].all()
    assert (a['z'][neg].view(np.int64) == 0).all()


def test_sea_floor_above_the_surface_is_not_skipped(monkeypatch, world):
    seeds = _seeds(world[2], 2049, 'alternate')
    depth = np.full(2049, 80.0, np.float32)
    dry = np.arange(2049) % 8 == 0                       # surface elements over "land": Zmin = +5 m > 0
    depth[dry] = -5.0
    a, count, pred, _, _ = _triple(monkeypatch, world, seeds, depth=depth)    # (env_upload between the step and the mixing call)
    assert not pred[dry].any() and count == 1025 - int(dry.sum())
    assert (a['z'][dry] != 0).all()                      # the walk puts them onto that sea floor


def test_nan_depth_is_skipped_as_the_walk_leaves_it(monkeypatch, world):
    seeds = _seeds(world[2], 2049, 'alternate')
    depth = np.full(2049, 80.0, np.float32)
    nan = np.arange(2049) % 8 == 0
    depth[nan] = np.nan
    a, count, pred, _, _ = _triple(monkeypatch, world, seeds, depth=depth)
    assert pred[nan].all() and count == 1025
    assert (a['z'][nan].view(np.int64) == 0).all()


def test_redo_path_of_the_two_quad_launch(monkeypatch):
    """K x 2000: sub-steps of about 100 m leave the two resident quads; those elements are redone on the whole column"""
    ctx, wl, g = _world(kscale=2000)
    try:
        rng = np.random.default_rng(7)
        n = 4100
        lon = rng.uniform(2.3, 3.4, n)                   # depth >= 496 m over this rectangle of the synthetic field
        lat = rng.uniform(60.05, 60.5, n)
        z = -rng.uniform(0, 480, n)
        z[rng.random(n) < 0.4] = 0.0
        _, count, _, _, sa = _triple(monkeypatch, (ctx, wl, g), (lon, lat, z))
        assert 0 < count < n and sa['window']['redone'] > 0, (count, sa)
    finally:
        ctx.close()


def test_eight_level_column(monkeypatch):
    ctx, wl, g = _world(nz=8)
    try:
        for n, pattern in ((257, 'alternate'), (2049, 'wave'), (4100, 'tile_last')):
            seeds = _seeds(g, n, pattern)
            _, count, _, _, _ = _triple(monkeypatch, (ctx, wl, g), seeds, windowed=False)
            assert count == int((seeds[2] == 0).sum())
    finally:
        ctx.close()


def test_guarded_launch_that_runs(monkeypatch, world):
    _, count, _, _, _ = _triple(monkeypatch, world, _seeds(world[2], 2049, 'alternate'), guarded=True)
    assert count == 1025


def test_guarded_launch_that_may_not_run_changes_nothing(monkeypatch, world):
    """One element deactivated ahead of the step launch: the fold's verdict is "not every element stays", and the four kernels
    of the guarded dense launch leave every byte of z (-0.0 entries included) and both device counters as they were"""
    ctx, wl, g = world
    _set_mode(monkeypatch, 'dense')
    lon, lat, z = _seeds(g, 2049, 'alternate')
    n = len(lon)
    z[np.arange(n) % 6 == 0] = -0.0
    P = ctx.particles(n)
    try:
        P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
        t = wl.time_of(1)
        step = dict(coastline='previous', store_previous=True, count=False, seafloor=True, age_dt=wl.dt)
        # a launch that runs first: the counters and the list's length on the device are not zero when the guarded one comes
        P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, **step)
        P.vmix(t, wl.dt, wl.dt_mix, step=1, fuse_vertical_advection=False)
        before = _stats(P)
        assert before['dense']['launches'] == 1 and before['dense']['listed'] > 0 and before['skip']['skipped'] > 0, before
        gone = np.zeros(n, bool)
        gone[700] = True
        P.deactivate(gone, 1)
        P.upload(z=z)                                        # surface elements and -0.0 again
        P.env_coast_advect(wl.vars, wl.time_of(2), wl.scheme, wl.dt, **step)
        z_before = P.download()['z'].copy()
        assert np.signbit(z_before[z_before == 0]).any() and (z_before != 0).any()
        assert P.scan_status_begin()
        assert P.vmix(wl.time_of(2), wl.dt, wl.dt_mix, step=2, fuse_vertical_advection=False, guarded=True)
        kept, _ = P.scan_status_end()
        assert kept == n - 1                                 # not every element stays: the guarded launch may not run
        z_after = P.download()['z']
        assert np.array_equal(z_after.view(np.uint8), z_before.view(np.uint8))
        after = _stats(P)
        assert after['dense'] == dict(launches=2, listed=before['dense']['listed']), (before, after)   # enqueued, nothing listed
        assert after['skip']['skipped'] == before['skip']['skipped'], (before, after)
        assert after['window']['redone'] == before['window']['redone'], (before, after)
    finally:
        P.close()


def test_mixing_at_the_surface_never_takes_the_dense_launch(monkeypatch, world):
    a, _, _, z_in, _ = _triple(monkeypatch, world, _seeds(world[2], 2049, 'alternate'), dense=False, may_skip=False, static=False,
                               mix_at_surface=True)
    assert (a['z'][z_in == 0] < 0).any()


def test_vertical_advection_at_the_surface_never_takes_the_dense_launch(monkeypatch, world):
    a, _, _, z_in, _ = _triple(monkeypatch, world, _seeds(world[2], 4100, 'alternate'), dense=False, may_skip=False, static=False,
                               fuse_vertical_advection=True)
    assert (a['z'][z_in == 0] < 0).any()                 # surface elements are advected downwards where w < 0


def test_host_uniforms_never_take_the_dense_launch(monkeypatch, world):
    uni = np.random.default_rng(2).uniform(size=(10, 2049))
    seeds = _seeds(world[2], 2049, 'wave')
    _, count, _, _, _ = _triple(monkeypatch, world, seeds, dense=False, static=False, uniforms=uni)
    assert count == int((seeds[2] == 0).sum()) == 1025
