"""GPU: the K plane of a reader level (csrc/odr_field.hip.h DevBlock::kplane) -- ocean_vertical_diffusivity a second time, as
4 * ((nz + 3) / 4) floats per node, written by the record writer of the level preparation -- and the mixing launches that gather
their K columns from it instead of from the node records.

  * the plane equals the K part of the records bit for bit on every way a level becomes resident, and after the slot was recycled;
  * odr_vmix computes the same z / moving / status from the planes as from the records (ODR_NO_KPLANE=1), bit for bit: on and
    between reader levels, 8 and 12 levels, with and without the fused vertical advection, the run-time and C3's static
    configuration, the five-level window kernel, and once at C3's full size with a re-sort among the steps;
  * a source with a level that has no plane gathers from the records; odr_particles_vmix_kplane_stats says which path ran."""
import numpy as np
import pytest

import bench
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu

U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
W, KZ = 'upward_sea_water_velocity', 'ocean_vertical_diffusivity'
DEPTH, SSH, LAND = 'sea_floor_depth_below_sea_level', 'sea_surface_height', 'land_binary_mask'
NAMES = [U, V, W, KZ, DEPTH, LAND]


def _grid(nz):
    """The synthetic C3 grid at its small size with nz levels: NaN on the land strip (filled by the dilation) and, added here,
    NaN below a sea floor that lies 1 .. nz - 1 levels down, varying from column to column (filled from the level above)."""
    g = synth.grid3d(nx=128, ny=96, nz=nz, nt=3, seed=0)
    iy, ix = np.indices(g[DEPTH][0].shape)
    below = np.arange(nz)[:, None, None] > (1 + (ix + 2 * iy) % (nz - 1))[None]    # [nz, ny, nx]
    assert below.any() and not below[0].any()
    for v in (U, V, W, KZ):
        g[v][:, below] = np.nan
    return g


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_plane(ctx, sid, slot, K, nz):
    got = ctx.kplane_read(sid, slot)
    assert got is not None
    plane, recs = got
    krec = 4 * ((nz + 3) // 4)
    assert plane.shape == K.shape[1:] + (krec,)
    assert np.array_equal(_bits(plane), _bits(recs))                     # every level slot, padding included
    assert not plane[..., nz:].any() and not np.signbit(plane[..., nz:]).any()
    src = np.moveaxis(K, 0, -1)
    ok = np.isfinite(src)
    assert np.array_equal(_bits(plane[..., :nz])[ok], _bits(src)[ok])    # cells that had a value keep it
    # a water column's levels below the sea floor hold the deepest value above them; the land strip was dilated
    wet = ok[..., 0]
    last = np.maximum(ok.cumsum(-1).max(-1) - 1, 0)
    deepest = np.take_along_axis(src, last[..., None], -1)
    filled = wet[..., None] & ~ok
    assert filled.any() and np.array_equal(_bits(plane[..., :nz])[filled], _bits(np.broadcast_to(deepest, src.shape))[filled])
    assert (~wet).any() and np.isfinite(plane[~wet]).sum() > 0


@pytest.mark.parametrize('nz', [8, 12, 6])
def test_plane_equals_the_k_part_of_the_records(nz):
    g = _grid(nz)
    ctx = Context(0, seed=0)
    sid = ctx.add_grid(g['x'], g['y'], z=g['z'])
    lev = lambda k, scale=1.0: {v: (g[v][k] * np.float32(scale) if v == KZ else g[v][k]) for v in NAMES}
    ctx.upload_block(sid, 0, 0.0, lev(0))
    _check_plane(ctx, sid, 0, g[KZ][0], nz)
    ctx.upload_block_async(sid, 1, 3600.0, lev(1))
    ctx.commit_block(sid, 1)
    _check_plane(ctx, sid, 1, g[KZ][1], nz)
    ctx.upload_block_device(sid, 2, 7200.0, lev(2), {v: (nz if g[v][2].ndim == 3 else 1) for v in NAMES})
    _check_plane(ctx, sid, 2, g[KZ][2], nz)
    _check_plane(ctx, sid, 0, g[KZ][0], nz)                              # (the later uploads left it alone)
    # the slot recycled with other content: the retired block of the same size is reused once the stream has passed it
    for rep in range(3):
        ctx.upload_block(sid, 0, 0.0, lev(2, 3.0 + rep))
        _check_plane(ctx, sid, 0, g[KZ][2] * np.float32(3.0 + rep), nz)
    # ... and with content that has no K: no plane, and none left over from the slot's earlier content
    ctx.upload_block(sid, 0, 0.0, {v: g[v][0] for v in NAMES if v != KZ})
    assert ctx.kplane_read(sid, 0) is None
    ctx.upload_block(sid, 0, 0.0, lev(1, 0.5))
    _check_plane(ctx, sid, 0, g[KZ][1] * np.float32(0.5), nz)
    ctx.close()


def _mix(monkeypatch, g, planes, times, lon_mode=1, vadv=False, n=20000, window=None, level_env=None, drop_k=None, seed=5):
    """odr_vmix at `times` on the levels of g; planes=False: ODR_NO_KPLANE=1.  level_env: {level: {environment variable: value}}
    set while that level is uploaded; drop_k: a level uploaded without K."""
    for k, v in (('ODR_NO_KPLANE', None if planes else '1'), ('ODR_VMIX_WINDOW', window)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    ctx = Context(0, seed=seed)
    sid = ctx.add_grid(g['x'], g['y'], z=g['z'], lon_mode=lon_mode)
    for k in range(3):
        for name, val in (level_env or {}).get(k, {}).items():
            monkeypatch.setenv(name, val)
        ctx.upload_block(sid, k, float(g['t'][k]), {v: g[v][k] for v in NAMES if not (v == KZ and k == drop_k)})
        for name in (level_env or {}).get(k, {}):
            monkeypatch.delenv(name)
    for v in NAMES:
        ctx.bind(v, [sid], {LAND: np.nan, DEPTH: 10000.0}.get(v, 0.0))
    ctx.bind(SSH, [], 0.0)
    rng = np.random.default_rng(seed + 1)
    lon = rng.uniform(g['x'][2], g['x'][-3], n)            # (the land strip included: its cells hold dilated values)
    lat = rng.uniform(g['y'][2], g['y'][-3], n)
    z = -rng.uniform(0, 1.1 * float(-g['z'][-1]), n)
    z[: n // 16] = 0.0
    P = ctx.particles(n)
    P.append(lon, lat, z=z, terminal_velocity=np.where(np.arange(n) % 3 == 0, -0.004, 0.002).astype(np.float32))
    for k, t in enumerate(times):
        P.env_sample([U, V, W, DEPTH, SSH], t)
        P.store_previous()
        P.vmix(t, 600.0, 60.0, step=k, fuse_vertical_advection=vadv)
    d = P.download()
    o = np.argsort(d['ID'], kind='stable')
    res = {q: np.ascontiguousarray(d[q][o]) for q in ('ID', 'z', 'moving', 'status', 'lon', 'lat')}
    stats = dict(P.vmix_kplane_stats(), **P.vmix_layout_stats())
    P.close()
    ctx.close()
    monkeypatch.delenv('ODR_NO_KPLANE', raising=False)
    monkeypatch.delenv('ODR_VMIX_WINDOW', raising=False)
    res['z0'] = z
    return res, stats


def _same(a, b):
    for q in a:
        assert np.array_equal(a[q].view(np.uint8), b[q].view(np.uint8)), q


# on a level (one K level), between two, on the next, past it
TIMES = (0.0, 0.37 * 3600.0, 3600.0, 4200.0)


@pytest.mark.parametrize('vadv', [False, True])
@pytest.mark.parametrize('lon_mode', [1, 2])
@pytest.mark.parametrize('nz', [8, 12])
def test_mixing_from_planes_equals_mixing_from_records(monkeypatch, nz, lon_mode, vadv):
    g = _grid(nz)
    a, sa = _mix(monkeypatch, g, True, TIMES, lon_mode=lon_mode, vadv=vadv)
    b, sb = _mix(monkeypatch, g, False, TIMES, lon_mode=lon_mode, vadv=vadv)
    assert sa['planes'] == len(TIMES) and sa['records'] == 0, sa
    assert sb['records'] == len(TIMES) and sb['planes'] == 0, sb
    # longitudes -180 .. 180 and the vertical advection fused below the surface are C3's configuration: static on both sides
    # (VMixC3 / VMixC3Rec); anything else reads its configuration at run time
    static = len(TIMES) if (lon_mode == 1 and vadv is False) else 0
    for s in (sa, sb):
        assert s['static'] == static and s['runtime'] == len(TIMES) - static and s['other'] == 0, s
    _same(a, b)
    assert (a['z'] <= 0).all() and np.abs(a['z'] - a['z0']).max() > 1.0


def test_window_kernel_from_planes_equals_records(monkeypatch):
    g = _grid(12)
    a, sa = _mix(monkeypatch, g, True, TIMES, window='1')
    b, sb = _mix(monkeypatch, g, False, TIMES, window='1')
    assert sa['planes'] == len(TIMES) and sa['records'] == 0 and sa['other'] == len(TIMES), sa
    assert sb['records'] == len(TIMES) and sb['planes'] == 0 and sb['other'] == len(TIMES), sb
    _same(a, b)
    assert np.abs(a['z'] - a['z0']).max() > 1.0


@pytest.mark.parametrize('nz', [8, 12])
def test_a_level_without_a_plane_sends_the_launch_to_the_records(monkeypatch, nz):
    """Level 1 prepared variable by variable (ODR_ROW_DILATE: the record writer that knows no plane): the source's levels disagree,
    both time levels are gathered from the records -- the same bits."""
    g = _grid(nz)
    ref, sr = _mix(monkeypatch, g, True, TIMES)
    a, sa = _mix(monkeypatch, g, True, TIMES, level_env={1: {'ODR_ROW_DILATE': '1'}})
    b, sb = _mix(monkeypatch, g, False, TIMES, level_env={1: {'ODR_ROW_DILATE': '1'}})
    assert sr['planes'] == len(TIMES) and sr['records'] == 0, sr
    for s in (sa, sb):
        assert s['records'] == len(TIMES) and s['planes'] == 0 and s['static'] == len(TIMES), s
    _same(a, b)
    _same(a, ref)


def test_a_source_without_k_on_a_level_keeps_the_generic_kernel(monkeypatch):
    """Level 2 uploaded without K: no plane there, and no fast column launch at all (build_vmix_desc wants K on every resident
    level) -- neither counter moves, the switch changes nothing."""
    g = _grid(8)
    times = TIMES[:3]
    a, sa = _mix(monkeypatch, g, True, times, drop_k=2)
    b, sb = _mix(monkeypatch, g, False, times, drop_k=2)
    for s in (sa, sb):
        assert s['planes'] == 0 and s['records'] == 0 and s['other'] == len(times), s
    _same(a, b)
    assert np.abs(a['z'] - a['z0']).max() > 1.0


def test_full_size_c3_planes_against_records(monkeypatch):
    """C3's block (1024 x 1024 x 12) and 10 M elements as tests/test_gpu_full_size.py builds them: three steps of the workload,
    the first behind a re-sort by grid cell; the whole z array, plane against records."""
    n, steps = 10_000_000, 3
    fields = bench.make_fields('c3')
    lon, lat, z = bench.seed_particles('c3', fields, n, np.random.default_rng(1))
    out = []
    for planes in (True, False):
        if planes:
            monkeypatch.delenv('ODR_NO_KPLANE', raising=False)
        else:
            monkeypatch.setenv('ODR_NO_KPLANE', '1')
        ctx = Context(0, seed=0)
        ctx.set_stage_math('fast')
        wl = bench.Workload('c3', ctx, fields, (0, 0, 1), via_torch=False)
        assert wl.sort_every and 0 % wl.sort_every == 0
        P = ctx.particles(n)
        P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
        for k in range(steps):
            wl.step(P, k)
        d = P.download()
        resorted = not np.array_equal(d['ID'], np.arange(n))
        o = np.argsort(d['ID'], kind='stable')     # (the re-sort's order inside a cell is not fixed from run to run)
        out.append(({q: np.ascontiguousarray(d[q][o]) for q in ('ID', 'z', 'moving', 'status')}, P.vmix_kplane_stats(),
                    P.vmix_layout_stats(), resorted))
        P.close()
        ctx.close()
    monkeypatch.delenv('ODR_NO_KPLANE', raising=False)
    (a, ka, la, ra), (b, kb, lb, rb) = out
    assert ka == dict(planes=steps, records=0) and kb == dict(planes=0, records=steps), (ka, kb)
    assert la == lb == dict(runtime=0, static=steps, other=0), (la, lb)
    assert len(a['z']) == n and np.array_equal(a['ID'], np.arange(n)) and ra and rb
    _same(a, b)
    assert np.abs(a['z'] - z).max() > 1.0
