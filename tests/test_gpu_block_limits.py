"""GPU: gridded blocks at the size limits that switch the sampling kernels.

The fast kernels (k_env_grid, k_step_grid / k_advect_grid, k_vmix_col, the LDS-tile step) find a node record with 24-bit
multiplies and a 32-bit byte offset.  That is valid only for a block the host marks `small` (odrift.hip, stage_block):
fewer than 2^24 nodes per level and fewer than 2^32 bytes of records; every other block must take the generic kernels.
The upload has a second switch: the one-pass preparation runs only for fewer than 65536 rows, the per-variable path
prepares the block otherwise.  Each case here is a pair of grids, one just below a limit and one just above it:

  A  node count:  4095 / 4097 rows x 4096 columns, 3-D (nz = 4), two time levels;
  B  byte count:  2048 x 3971 / 3973 nodes of 132-float records (u, v at nz = 64 = MAXNZ, depth, land), one level;
  C  rows:        65535 / 65536 rows x 8 columns with NaN patches that need the dilation.

Every field holds a ramp in the row index, so that a record read at a wrapped offset gives a sample far outside any
tolerance; the tests check that on the host for the grids above the limits.  Which side of a limit a grid is on is asserted
twice: from the record layout rules of stage_block (record_layout / is_small below), and through the launch counters of
the fused step (step_layout_stats), the guarded mixing call (refused unless the fast column kernel would run) and the
LDS-tile step (tile_stats)."""
import gc

import numpy as np
import pytest

from bookkeeping_model import cell_keys, sort_bins
from conftest import _gpu_tests_selected
from scenarios import Scenario
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U, V = 'x_sea_water_velocity', 'y_sea_water_velocity'
W, KZ = 'upward_sea_water_velocity', 'ocean_vertical_diffusivity'
DEPTH, SSH, LAND = 'sea_floor_depth_below_sea_level', 'sea_surface_height', 'land_binary_mask'
PAIRS = ((U, V), ('x_wind', 'y_wind'),
         ('sea_surface_wave_stokes_drift_x_velocity', 'sea_surface_wave_stokes_drift_y_velocity'),
         ('sea_ice_x_velocity', 'sea_ice_y_velocity'))
FALLBACKS = {U: 0.0, V: 0.0, W: 0.0, KZ: 0.0, DEPTH: 10000.0, SSH: 0.0}
FAST_STEP_BOUND = 3e-9   # deg per 600 s step: FAST stage arithmetic against the exact oracle (tests/test_gpu_stage_math.py)
DT, DT_MIX = 600.0, 60.0


# ------------------------------------------------------------------ the host's size rules
def record_layout(var_nz):
    """The node record of stage_block: vector pairs interleaved first, then the other 3-D variables, then the 2-D ones, in
    upload order; the length padded to 4 floats.  var_nz: {variable: layers} in upload order.  Returns (rec, {variable:
    (offset, element stride, element offset)}): layer k of a variable at node n is float n * rec + offset + k * stride + eo."""
    off, rec = {}, 0
    for a, b in PAIRS:
        if a in var_nz and b in var_nz and var_nz[a] == var_nz[b]:
            off[a], off[b] = (rec, 2, 0), (rec, 2, 1)
            rec += 2 * var_nz[a]
    for three_d in (True, False):
        for k, nz in var_nz.items():
            if k not in off and (nz > 1) == three_d:
                off[k] = (rec, 1, 0)
                rec += nz
    return (rec + 3) & ~3, off


def is_small(ny, nx, rec):
    """DevBlock::small: the fast kernels' 24-bit node numbers and 32-bit byte offsets hold."""
    plane = ny * nx
    return plane < 2 ** 24 and plane * rec * 4 < 2 ** 32 and rec * 4 < 2 ** 24


def one_pass_preparation(ny, var_nz):
    return ny < 65536 and sum(var_nz.values()) < 65536


def fast_read_address(node, byte_in_record, rec):
    """The byte offset a fast kernel forms for a node record: __umul24(node, rec * 4) plus the offset inside the record, in
    32 bits.  Equal to the true offset exactly when the block is small."""
    node = np.asarray(node, dtype=np.uint64)
    return ((node & np.uint64(0xFFFFFF)) * np.uint64(rec * 4) + np.uint64(byte_in_record)) & np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------ the three pairs of grids
CASES = {
    'A-below': dict(kind='A', ny=4095, nx=4096, small=True),
    'A-above': dict(kind='A', ny=4097, nx=4096, small=False),
    'B-below': dict(kind='B', ny=2048, nx=3971, small=True),
    'B-above': dict(kind='B', ny=2048, nx=3973, small=False),
    'C-65535': dict(kind='C', ny=65535, nx=8, small=True, one_pass=True),
    'C-65536': dict(kind='C', ny=65536, nx=8, small=True, one_pass=False),
}
A_B = ['A-below', 'A-above', 'B-below', 'B-above']
A_ONLY = ['A-below', 'A-above']


def _axes(ny, nx):
    f32 = np.float32
    r = np.arange(ny, dtype=f32)[:, None]
    sx = np.sin(np.arange(nx) * 0.0123).astype(f32)[None, :]
    cy = np.cos(np.arange(ny) * 0.0071).astype(f32)[:, None]
    return r, sx, cy


def _fields_a(ny, nx):
    """Node-count case: u, v, w, K on 4 levels, depth and land; two time levels.  Rows 0 .. ny-1 are the same for either
    ny (the ramp is in the row index), so the two grids share every node they have in common."""
    f32 = np.float32
    nz, nt = 4, 2
    z = np.array([0.0, -10.0, -25.0, -50.0])
    r, sx, cy = _axes(ny, nx)
    shape = (nt, nz, ny, nx)
    u, v, w, K = (np.empty(shape, f32) for _ in range(4))
    for it in range(nt):
        for k in range(nz):
            fk = f32(1.0 - 0.1 * k)
            u[it, k] = -(f32(0.1) + f32(5e-5) * r + f32(0.05) * sx) * fk + f32(0.01 * it)
            v[it, k] = -(f32(0.05) + f32(2e-5) * r + f32(0.03) * cy) * fk - f32(0.005 * it)
            w[it, k] = f32(1e-3) * fk * sx * cy + f32(1e-7) * r + f32(1e-5 * it)
            K[it, k] = f32(1e-2) * fk * (f32(1) + f32(0.5) * sx) + f32(1e-6) * r + f32(1e-5 + 1e-4 * it)
    depth = f32(30) + f32(0.05) * r + f32(5) * sx
    land = np.zeros((ny, nx), f32)
    land[4093:, 4050:] = 1.0                       # rows both grids have
    x = (np.arange(nx) * 0.01).astype(f32)
    y = (20.0 + np.arange(ny) * 0.01).astype(f32)
    levels = [(3600.0 * it, {U: u[it], V: v[it], W: w[it], KZ: K[it], DEPTH: depth, LAND: land}) for it in range(nt)]
    return dict(x=x, y=y, z=z, levels=levels)


def _fields_b(ny, nx):
    """Byte-count case: u, v on 64 levels, depth and land; one time level.  (No KZ: the mixing inside the fused step reads
    the fallback diffusivity.)"""
    f32 = np.float32
    nz = 64
    z = -2.0 * np.arange(nz)
    r, sx, cy = _axes(ny, nx)
    u = np.empty((nz, ny, nx), f32)
    v = np.empty((nz, ny, nx), f32)
    for k in range(nz):
        fk = f32(1.0 - k / 128.0)
        u[k] = -(f32(0.1) + f32(1e-4) * r + f32(0.05) * sx) * fk
        v[k] = -(f32(0.05) + f32(5e-5) * r + f32(0.03) * cy) * fk
    depth = f32(30) + f32(0.1) * r + f32(5) * sx
    land = np.zeros((ny, nx), f32)
    land[ny - 2:, nx - 40:] = 1.0
    x = (np.arange(nx) * 0.01).astype(f32)
    y = (40.0 + np.arange(ny) * 0.01).astype(f32)
    return dict(x=x, y=y, z=z, levels=[(0.0, {U: u, V: v, DEPTH: depth, LAND: land})])


def _fields_c(ny, nx):
    """Row case: u, v on 2 levels, depth, land; two time levels; NaN patches the dilation has to fill (a coastal band, the
    first and last rows, a stretch of the first column), a patch 40 rows deep (its middle stays NaN after ten sweeps), one
    at the last rows, and water under a deeper-level NaN (filled towards the sea floor)."""
    f32 = np.float32
    nz, nt = 2, 2
    z = np.array([0.0, -20.0])
    r, sx, cy = _axes(ny, nx)
    u = np.empty((nt, nz, ny, nx), f32)
    v = np.empty((nt, nz, ny, nx), f32)
    for it in range(nt):
        for k in range(nz):
            u[it, k] = f32(0.1) + f32(1e-5) * r + f32(0.05) * sx + f32(0.01 * (it + k))
            v[it, k] = f32(-0.05) - f32(1e-6) * r + f32(0.03) * cy - f32(0.02 * (it + k))
    depth = f32(30) + f32(1e-3) * r + f32(5) * sx
    land = np.zeros((ny, nx), f32)
    land[1000:1500, 6:] = 1.0
    depth = np.broadcast_to(depth, (ny, nx)).copy()
    for a in (u, v):
        a[:, :, 1000:1500, 6:] = np.nan            # coastal band
        a[:, :, 0, :] = np.nan                     # block edges
        a[:, :, ny - 1, :] = np.nan
        a[:, :, 30000:30100, 0] = np.nan
        a[:, :, 50000:50040, :] = np.nan           # deeper than ten cells
        a[:, :, ny - 30:ny - 5, 2:] = np.nan       # next to the last row
        a[:, 1, 20000:20100, 2:6] = np.nan         # filled from the level above
    depth[40000:40030, :] = np.nan
    depth[ny - 12:, 5:] = np.nan
    x = (np.arange(nx) * 0.01).astype(f32)
    y = (-30.0 + np.arange(ny) * 0.001).astype(f32)
    levels = [(3600.0 * it, {U: u[it], V: v[it], DEPTH: depth, LAND: land}) for it in range(nt)]
    return dict(x=x, y=y, z=z, levels=levels)


C_PATCHES = ((995, 1505, 4, 7), (0, 6, 0, 7), (29990, 30110, 0, 3), (49995, 50045, 0, 7), (65500, 65535, 0, 7),
             (19990, 20110, 1, 7), (39995, 40035, 0, 7))   # rows, columns around the NaN patches of _fields_c


def _seed(f, n, rng, zmin):
    """Most elements in the last 16 rows, some exactly on nodes of the last row and the last column, the rest anywhere."""
    x, y = f['x'], f['y']
    ny, nx = len(y), len(x)
    nlast, nnode = int(0.6 * n), 2000
    lon = np.empty(n)
    lat = np.empty(n)
    lon[:nlast] = rng.uniform(x[0], x[-1], nlast)
    lat[:nlast] = rng.uniform(y[ny - 16], y[-1], nlast)
    h = nnode // 2
    lon[nlast:nlast + h] = x[rng.integers(0, nx, h)]
    lat[nlast:nlast + h] = y[-1]
    lon[nlast + h:nlast + nnode] = x[-1]
    lat[nlast + h:nlast + nnode] = y[rng.integers(ny - 64, ny, nnode - h)]
    lon[nlast + nnode - 4:nlast + nnode] = x[-1]
    lat[nlast + nnode - 4:nlast + nnode] = y[-1]
    m = n - nlast - nnode
    lon[nlast + nnode:] = rng.uniform(x[0], x[-1], m)
    lat[nlast + nnode:] = rng.uniform(y[0], y[-1], m)
    z = -rng.uniform(0, zmin, n)
    z[:200] = 0.0
    return lon, lat, z


@pytest.fixture(scope='module')
def case(request, has_gpu):
    """One grid of CASES, uploaded to a context of its own, with its oracle world and elements.  Module scope: the tests of
    one grid share it; pytest finishes it before the next grid is built (peak host memory: one grid and its oracle copy)."""
    if not has_gpu:     # (as conftest's ctx fixture)
        if _gpu_tests_selected(request.config):
            pytest.fail('-m gpu was asked for and no GPU is visible on this box')
        pytest.skip('no GPU visible')
    from opendrift_amd.device import Context
    name = request.param
    spec = CASES[name]
    ny, nx = spec['ny'], spec['nx']
    f = {'A': _fields_a, 'B': _fields_b, 'C': _fields_c}[spec['kind']](ny, nx)
    var_nz = {k: (a.shape[0] if a.ndim == 3 else 1) for k, a in f['levels'][0][1].items()}
    rec, layout = record_layout(var_nz)
    ctx = Context(0, seed=0)
    sc = Scenario([('grid', dict(x=f['x'], y=f['y'], z=f['z'], levels=f['levels']))], fallbacks=FALLBACKS)
    sc.device(ctx)             # (first: the oracle world is built from the same arrays)
    if spec['kind'] == 'C':
        # ReaderBlock's fill_NaN_towards_seafloor (structured.py:58-60), which the upload does on the device: the oracle world
        # samples its arrays as given.  (Grids A and B hold no NaN.)
        for _, arrays in f['levels']:
            for a in arrays.values():
                for k in range(1, a.shape[0] if a.ndim == 3 else 1):
                    m = np.isnan(a[k])
                    a[k][m] = a[k - 1][m]
    rng = np.random.default_rng(sum(map(ord, name)))
    n = 20000 if spec['kind'] == 'C' else 30000
    lon, lat, z = _seed(f, n, rng, {'A': 45.0, 'B': 120.0, 'C': 25.0}[spec['kind']])
    if spec['kind'] == 'C':    # 300 elements in and around each NaN patch
        for k, (r0, r1, c0, c1) in enumerate(C_PATCHES):
            s = slice(len(lon) - 300 * (k + 1), len(lon) - 300 * k)
            lat[s] = rng.uniform(f['y'][r0], f['y'][min(r1, ny - 1)], 300)
            lon[s] = rng.uniform(f['x'][c0], f['x'][c1], 300)
    world = sc.oracle_world()
    # (the world points into the builder's copies of the arrays: kept with it.  Grids A and B hold no NaN, so the oracle's
    # dilation never writes into them and one world serves every call)
    d = dict(name=name, spec=spec, f=f, ny=ny, nx=nx, var_nz=var_nz, rec=rec, layout=layout, ctx=ctx, sc=sc,
             sid=0, lon=lon, lat=lat, z=z, world=world, builder=sc._wb)
    yield d
    ctx.close()
    d.clear()
    f.clear()
    gc.collect()


def _params(names):
    return pytest.mark.parametrize('case', names, indirect=True)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _maxerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(a) else 0.0


def _level0_sample(c, var, lon, lat, wrapped):
    """Bilinear sample of layer 0 of `var` at time level 0 on the host, each corner read at the byte offset a fast kernel
    would form (wrapped=True) or at the true one.  Returns (samples, elements with a corner of nonzero weight whose offset
    differs)."""
    f, rec, layout = c['f'], c['rec'], c['layout']
    ny, nx = c['ny'], c['nx']
    x, y = f['x'], f['y']
    arrays = f['levels'][0][1]
    inv = {}                         # float in the record -> (variable, layer)
    for k, (o, es, eo) in layout.items():
        for j in range(c['var_nz'][k]):
            inv[o + j * es + eo] = (k, j)
    xi = (lon - float(x[0])) / float(x[-1] - x[0]) * (nx - 1)
    yi = (lat - float(y[0])) / float(y[-1] - y[0]) * (ny - 1)
    ix0 = np.clip(np.floor(xi).astype(np.int64), 0, nx - 2)
    iy0 = np.clip(np.floor(yi).astype(np.int64), 0, ny - 2)
    tx, ty = xi - ix0, yi - iy0
    o, es, eo = layout[var]
    out = np.zeros(len(lon))
    moved = np.zeros(len(lon), bool)
    for dy, dx, wgt in ((0, 0, (1 - ty) * (1 - tx)), (0, 1, (1 - ty) * tx), (1, 0, ty * (1 - tx)), (1, 1, ty * tx)):
        node = (iy0 + dy) * nx + (ix0 + dx)
        true = node.astype(np.uint64) * np.uint64(rec * 4) + np.uint64(4 * (o + eo))
        addr = fast_read_address(node, 4 * (o + eo), rec) if wrapped else true
        moved |= (addr != true) & (wgt > 0)
        nd, fl = (addr // np.uint64(rec * 4)).astype(np.int64), ((addr % np.uint64(rec * 4)) // np.uint64(4)).astype(np.int64)
        val = np.zeros(len(lon))
        for q in np.unique(fl):
            sel = fl == q
            if int(q) in inv:
                k, j = inv[int(q)]
                a = arrays[k]
                plane = a[j] if a.ndim == 3 else a
                val[sel] = plane.reshape(-1)[nd[sel]]
        out += wgt * val
    return out, moved


# ------------------------------------------------------------------ which side of the limit
@_params(list(CASES))
def test_grid_is_on_the_expected_side(case):
    c, spec = case, case['spec']
    assert is_small(c['ny'], c['nx'], c['rec']) == spec['small'], (c['name'], c['rec'])
    assert one_pass_preparation(c['ny'], c['var_nz']) == spec.get('one_pass', True), c['name']
    plane = c['ny'] * c['nx']
    if spec['kind'] == 'A':
        assert c['rec'] == 20
        assert (plane < 2 ** 24) == spec['small'] and plane * c['rec'] * 4 < 2 ** 32
    elif spec['kind'] == 'B':
        assert c['rec'] == 132 and plane < 2 ** 24 and (plane * c['rec'] * 4 < 2 ** 32) == spec['small']
    if spec['kind'] in 'AB':
        # a fast kernel's read of the last rows: the true record below the limit, another node's above it -- and that one
        # holds values far from the true sample (the tests below would see a wrong read)
        sel = c['lat'] >= c['f']['y'][c['ny'] - 16]
        lon, lat = c['lon'][sel], c['lat'][sel]
        for var in (U, V, DEPTH):
            good, _ = _level0_sample(c, var, lon, lat, wrapped=False)
            bad, moved = _level0_sample(c, var, lon, lat, wrapped=True)
            if spec['small']:
                assert not moved.any() and _same_bits(good, bad), var
            else:
                assert moved.sum() > 500, (var, int(moved.sum()))
                off = np.abs(bad - good)[moved]
                assert np.median(off) > 1e-2 and (off > 1e-4).mean() > 0.95, (var, np.median(off), (off > 1e-4).mean())


# ------------------------------------------------------------------ 1. sampled environment
@_params(list(CASES))
def test_env_sample_bit_exact(case):
    c = case
    names = list(c['var_nz'])
    lon, lat, z = c['lon'], c['lat'], c['z']
    P = c['ctx'].particles(len(lon))
    P.append(lon, lat, z=z)
    times = (0.0,) if c['spec']['kind'] == 'B' else (0.0, 1234.5)    # on a time level; between the two
    for t in times:
        got = P.env_sample(names, t, download=True)
        w = c['world']
        if c['spec']['kind'] == 'C':       # the oracle's NaN dilation writes into its copies: a fresh world per call
            w = c['sc'].oracle_world()
        ref = orc.get_environment(w, [orc.VAR[k] for k in names], lon, lat, z, t)
        for k, r in zip(names, ref):
            a = got[k]
            same = (a == r) | (np.isnan(a) & np.isnan(r))
            assert same.all(), (c['name'], k, t, int((~same).sum()), a[~same][:4], r[~same][:4])
    P.close()


# ------------------------------------------------------------------ 2. advection
@pytest.mark.parametrize('mode', ['exact', 'fast'])
@_params(A_B)
def test_advection_matches_oracle(case, mode):
    c = case
    ctx, w = c['ctx'], c['world']
    lon, lat, z = c['lon'], c['lat'], c['z']
    n = len(lon)
    mv, cdf = np.ones(n, np.int32), np.ones(n, np.float32)
    t = 0.0 if c['spec']['kind'] == 'B' else 1500.0
    tol = 1e-10 if mode == 'exact' else FAST_STEP_BOUND
    ctx.set_stage_math(mode)
    try:
        for isch, scheme in enumerate(('euler', 'runge-kutta', 'runge-kutta4')):
            P = ctx.particles(n)
            P.append(lon, lat, z=z)
            P.env_sample([U, V], t)
            P.advect(scheme, t, DT)
            got = P.download()
            P.close()
            lo, la = lon.copy(), lat.copy()
            ue, ve = orc.get_environment(w, [orc.VAR[U], orc.VAR[V]], lo, la, z, t)
            orc.advect_ocean_current(w, isch, lo, la, z, mv, cdf, ue, ve, t, DT)
            err = max(_maxerr(got['lon'], lo), _maxerr(got['lat'], la))
            assert err < tol, (c['name'], mode, scheme, err)
    finally:
        ctx.set_stage_math('exact')


# ------------------------------------------------------------------ 3. vertical mixing
def _fast_column_mixing_taken(c, t):
    """Whether odr_vmix takes the fast column kernel (odr_mix.hip: a guarded call is refused -- returns 1, launches nothing --
    exactly when it would not).  A guarded call needs the fold of a fused step launch's counts: the C3 step first."""
    lon, lat, z = c['lon'][:4096], c['lat'][:4096], c['z'][:4096]
    Q = c['ctx'].particles(len(lon))
    Q.append(lon, lat, z=z)
    Q.env_coast_advect([U, V, W, DEPTH, SSH, LAND], t, 'runge-kutta4', DT, coastline='previous', store_previous=True,
                       count=False, seafloor=True, age_dt=DT)
    folded = Q.scan_status_begin()
    assert folded == c['spec']['small'], (c['name'], 'fold of the fused step counts', folded)
    taken = Q.vmix(t, DT, DT_MIX, step=0, guarded=True)
    if folded:
        Q.scan_status_end()
    Q.close()
    return taken


@_params(A_ONLY)
def test_vmix_matches_oracle(case):
    c = case
    t = 1800.0
    assert _fast_column_mixing_taken(c, t) == c['spec']['small'], c['name']
    names = [DEPTH, SSH, W]
    lon, lat, z0 = c['lon'], c['lat'], c['z']
    n = len(lon)
    tv = np.random.default_rng(23).normal(0, 0.002, n).astype(np.float32)
    uni = np.random.default_rng(3).uniform(size=(int(DT / DT_MIX), n))
    w = c['world']
    Kp = orc.get_profile(w, orc.VAR[KZ], lon, lat, t, len(c['f']['z']))
    for mix_at_surface in (False, True):
        P = c['ctx'].particles(n)
        P.append(lon, lat, z=z0, terminal_velocity=tv)
        env = P.env_sample(names, t, download=True)
        P.vmix(t, DT, DT_MIX, mix_at_surface=mix_at_surface, uniforms=uni)
        P.vertical_advection(DT)
        got = P.download()
        P.close()
        zz = z0.copy()
        orc.vertical_mixing(zz, np.ones(n, np.int32), tv, env[DEPTH], env[SSH], c['f']['z'], Kp, DT, DT_MIX,
                            int(mix_at_surface), uni)
        orc.vertical_advection(zz, np.ones(n, np.int32), env[W], DT)
        assert _maxerr(got['z'], zz) < 1e-9, (c['name'], mix_at_surface, _maxerr(got['z'], zz))


# ------------------------------------------------------------------ 4. the fused C3-style step against the generic kernels
def _fused_steps(c, monkeypatch, env, steps=3, scheme='runge-kutta4', vmix=True, sort=False):
    for k in ('ODR_NO_FAST_PATH', 'ODR_TILE', 'ODR_TILE_MIN_N'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    names = [U, V, W, DEPTH, SSH, LAND]
    lon, lat, z = c['lon'], c['lat'], c['z']
    n = len(lon)
    P = c['ctx'].particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    t0 = 0.0 if c['spec']['kind'] == 'B' else 600.0
    if sort:
        P.sort_by_cell(c['sid'])
    envs = []
    for k in range(steps):
        P.env_coast_advect(names, t0 + k * DT, scheme, DT, coastline='previous', store_previous=True, count=False,
                           seafloor=True, age_dt=DT,
                           vmix=dict(dt_mix=DT_MIX, step=k, vertical_advection=False) if vmix else None)
        o = np.argsort(P.ids(), kind='stable')
        envs.append({v: P.env_download(v)[o] for v in names})
    d = P.download()
    o = np.argsort(d['ID'], kind='stable')
    state = {k: np.ascontiguousarray(d[k][o]) for k in ('ID', 'lon', 'lat', 'z', 'status', 'moving')}
    stats, tiles = P.step_layout_stats(), P.tile_stats()
    P.close()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return state, envs, stats, tiles


def _assert_same_run(a, b, what):
    (sa, ea), (sb, eb) = a[:2], b[:2]
    for k in sa:
        assert _same_bits(sa[k], sb[k]), (what, k)
    for step, (x, y) in enumerate(zip(ea, eb)):
        for v in x:
            assert _same_bits(x[v], y[v]), (what, step, v)


@_params(A_B)
def test_fused_step_same_bits_as_generic_kernels(case, monkeypatch):
    c = case
    fast = _fused_steps(c, monkeypatch, {})
    generic = _fused_steps(c, monkeypatch, {'ODR_NO_FAST_PATH': '1'})
    fused = sum(fast[2].values())
    # the same scenario on both sides: fused step launches below the limit, none above
    assert (fused > 0) == c['spec']['small'], (c['name'], fast[2])
    if c['spec']['small']:
        assert fused == 3, fast[2]
    assert sum(generic[2].values()) == 0, generic[2]
    assert (fast[0]['lat'] != c['lat']).mean() > 0.5        # (elements are in ID order: they moved)
    _assert_same_run(fast, generic, c['name'])


# ------------------------------------------------------------------ 5. sort by cell
def _cell_keys(c, lon, lat):
    """sort_key of the host (k_sort_hist); lon_mode 2: the grid's longitudes are all >= 0"""
    assert (len(c['f']['y']), len(c['f']['x'])) == (c['ny'], c['nx'])
    return cell_keys(c['f']['x'], c['f']['y'], lon, lat, lon_mode=2)


@_params(A_ONLY)
def test_sort_by_cell_changes_only_the_layout(case):
    c = case
    nb = sort_bins(c['ny'], c['nx'])
    assert nb > 2 ** 24, nb          # on both sides: ~16 K block sums of 1024 bins through k_cmp_scan
    lon, lat, z = c['lon'], c['lat'], c['z']
    n = len(lon)
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    P = c['ctx'].particles(n)
    P.append(lon[perm], lat[perm], z=z[perm], id=perm.astype(np.int32))
    P.env_sample([U, V, DEPTH], 1200.0)
    before = P.download()
    env_before = {v: P.env_download(v) for v in (U, V, DEPTH)}
    P.sort_by_cell(c['sid'])
    after = P.download()
    env_after = {v: P.env_download(v) for v in (U, V, DEPTH)}
    P.close()
    ob, oa = np.argsort(before['ID']), np.argsort(after['ID'])
    assert np.array_equal(before['ID'][ob], after['ID'][oa]) and np.array_equal(after['ID'][oa], np.arange(n))
    for k in ('lon', 'lat', 'z', 'status', 'moving'):
        assert _same_bits(before[k][ob], after[k][oa]), k
    for v in env_before:
        assert _same_bits(env_before[v][ob], env_after[v][oa]), v
    keys = _cell_keys(c, after['lon'], after['lat'])
    assert (np.diff(keys) >= 0).all(), int((np.diff(keys) < 0).sum())
    assert len(np.unique(keys)) > 1000


# ------------------------------------------------------------------ 6. the LDS-tile step
@_params(A_ONLY)
def test_tile_step_gate(case, monkeypatch):
    c = case
    kw = dict(steps=2, scheme='runge-kutta', vmix=False, sort=True)
    plain = _fused_steps(c, monkeypatch, {}, **kw)
    tile = _fused_steps(c, monkeypatch, {'ODR_TILE': '1', 'ODR_TILE_MIN_N': '1'}, **kw)
    assert (tile[3]['launches'] > 0) == c['spec']['small'], (c['name'], tile[3])
    assert plain[3]['launches'] == 0
    _assert_same_run(plain, tile, c['name'])
