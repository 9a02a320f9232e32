"""GPU: the tiled K-column mixing launch (k_vmix_col, csrc/odr_kernels.hip.h) leaves out the elements it cannot change -- z == 0
on entry, no mixing and no vertical advection at the surface, the sea floor not above the surface -- and mixes the rest of each
1024-element tile densely packed.  Byte for byte it computes what the same launch computes with ODR_NO_VMIX_SKIP=1 (same tiling,
nothing skipped): at the sizes around the wave, workgroup and tile edges, for the patterns that fill, empty and split waves and
passes, with -0.0, negative and NaN depths, with the settings that forbid the skip, with host uniforms, on a reader level and
between two, through the redo path of the two-quad launch and in the guarded launch.  odr_particles_vmix_skip_stats counts the
skipped elements: the NumPy count of the predicate."""
import numpy as np
import pytest

import bench
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu

KZ, DEPTH, SSH = 'ocean_vertical_diffusivity', 'sea_floor_depth_below_sea_level', 'sea_surface_height'
SWITCH = 'ODR_NO_VMIX_SKIP'
TILE = 1024
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4100]
PATTERNS = ['none', 'all', 'alternate', 'wave', 'tile_last']
FIELDS = ('z', 'moving', 'status', 'lon', 'lat')


def _world(kscale=1):
    """C3's readers and bindings (bench.Workload) on a 12-level block of 64 x 48 nodes: the static two-quad launch (VMixC3W)"""
    g = synth.grid3d(nx=64, ny=48, nz=12, nt=3, seed=0)
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


def _once(monkeypatch, world, seeds, k, skip, depth=None, guarded=False, **mix):
    """One step launch and one mixing launch of step k on fresh elements.  Returns the download, the NumPy count of the skip
    predicate on what the mixing launch read, the predicate, z on entry, and the three statistics."""
    ctx, wl, _ = world
    if skip:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, '1')
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
    stats = P.vmix_skip_stats(), P.vmix_layout_stats(), P.vmix_window_stats()
    P.close()
    return out, int(pred.sum()), pred, z_in, stats


def _same(a, b):
    for q in FIELDS:
        x, y = np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), q


def _pair(monkeypatch, world, seeds, k=1, may_skip=True, static=True, **kw):
    """The launch with and without the skip on the same seeds: bytes, counters, +0.0 where the predicate holds"""
    a, count, pred, z_in, (sa, la, wa) = _once(monkeypatch, world, seeds, k, True, **kw)
    b, count_b, _, _, (sb, lb, wb) = _once(monkeypatch, world, seeds, k, False, **kw)
    assert count == count_b
    _same(a, b)
    assert sa == dict(launches=1, skipped=count if may_skip else 0), (sa, count)
    assert sb == dict(launches=1, skipped=0), sb
    want = dict(runtime=0, static=1, other=0) if static else dict(runtime=1, static=0, other=0)
    assert la == lb == want, (la, lb)
    assert wa['windowed'] == wb['windowed'] == (1 if static else 0) and wa['full'] == wb['full'] == 0, (wa, wb)
    if may_skip:
        assert (a['z'][pred].view(np.int64) == 0).all()      # +0.0, bit for bit
    return a, count, pred, z_in, wa


@pytest.mark.parametrize('n', SIZES)
def test_skipping_surface_elements_changes_no_byte(monkeypatch, world, n):
    for pattern in PATTERNS:
        seeds = _seeds(world[2], n, pattern)
        a, count, pred, z_in, _ = _pair(monkeypatch, world, seeds)
        assert count == int((seeds[2] == 0).sum()), pattern         # (the sea floor is at 50 m or below: every surface element)
        if count < n:
            assert not np.array_equal(a['z'][~pred], z_in[~pred]), pattern    # the others were mixed


@pytest.mark.parametrize('k', [0, 1], ids=['on_level', 'between_levels'])
def test_on_a_reader_level_and_between_two(monkeypatch, world, k):
    _, count, _, _, _ = _pair(monkeypatch, world, _seeds(world[2], 2049, 'alternate'), k=k)
    assert count == 1025


def test_negative_zero_comes_out_as_positive_zero(monkeypatch, world):
    lon, lat, z = _seeds(world[2], 1025, 'alternate')
    neg = np.arange(1025) % 6 == 0
    z[neg] = -0.0
    assert np.signbit(z[neg]).all()
    a, count, pred, _, _ = _pair(monkeypatch, world, (lon, lat, z))
    assert count == 513 and pred[neg].all()
    assert (a['z'][neg].view(np.int64) == 0).all()


def test_sea_floor_above_the_surface_is_not_skipped(monkeypatch, world):
    seeds = _seeds(world[2], 2049, 'alternate')
    depth = np.full(2049, 80.0, np.float32)
    dry = np.arange(2049) % 8 == 0                       # surface elements over "land": Zmin = +5 m > 0
    depth[dry] = -5.0
    a, count, pred, _, _ = _pair(monkeypatch, world, seeds, depth=depth)
    assert not pred[dry].any() and count == 1025 - int(dry.sum())
    assert (a['z'][dry] != 0).all()                      # the walk puts them onto that sea floor


def test_nan_depth_is_skipped_as_the_walk_leaves_it(monkeypatch, world):
    seeds = _seeds(world[2], 2049, 'alternate')
    depth = np.full(2049, 80.0, np.float32)
    nan = np.arange(2049) % 8 == 0
    depth[nan] = np.nan
    a, count, pred, _, _ = _pair(monkeypatch, world, seeds, depth=depth)
    assert pred[nan].all() and count == 1025
    assert (a['z'][nan].view(np.int64) == 0).all()


def test_mixing_at_the_surface_skips_nothing(monkeypatch, world):
    a, _, _, z_in, _ = _pair(monkeypatch, world, _seeds(world[2], 2049, 'alternate'), may_skip=False, static=False,
                             mix_at_surface=True)
    assert (a['z'][z_in == 0] < 0).any()


def test_vertical_advection_at_the_surface_skips_nothing(monkeypatch, world):
    a, _, _, z_in, _ = _pair(monkeypatch, world, _seeds(world[2], 4100, 'alternate'), may_skip=False, static=False,
                             fuse_vertical_advection=True)
    assert (a['z'][z_in == 0] < 0).any()                 # surface elements are advected downwards where w < 0


def test_host_uniforms(monkeypatch, world):
    uni = np.random.default_rng(2).uniform(size=(10, 2049))
    seeds = _seeds(world[2], 2049, 'wave')
    _, count, _, _, _ = _pair(monkeypatch, world, seeds, static=False, uniforms=uni)
    assert count == int((seeds[2] == 0).sum()) == 1025


def test_guarded_launch(monkeypatch, world):
    _, count, _, _, _ = _pair(monkeypatch, world, _seeds(world[2], 2049, 'alternate'), guarded=True)
    assert count == 1025


def test_redo_path_inside_a_compacted_pass(monkeypatch):
    """K x 2000: sub-steps of about 100 m leave the two resident quads; those elements are redone on the whole column in the
    pass that holds them"""
    ctx, wl, g = _world(kscale=2000)
    try:
        rng = np.random.default_rng(7)
        n = 4100
        lon = rng.uniform(2.3, 3.4, n)                   # depth >= 496 m over this rectangle of the synthetic field
        lat = rng.uniform(60.05, 60.5, n)
        z = -rng.uniform(0, 480, n)
        z[rng.random(n) < 0.4] = 0.0
        _, count, _, _, wa = _pair(monkeypatch, (ctx, wl, g), (lon, lat, z))
        assert 0 < count < n and wa['redone'] > 0, (count, wa)
    finally:
        ctx.close()
