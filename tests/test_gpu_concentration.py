"""GPU: odr_density_map_proj, odr_species_layer_map, odr_proj_extent, odr_proj_grid_lonlat and odr_box_smooth, and the model methods on
them (get_density_array_proj, get_radionuclide_density_array, horizontal_smooth), against the reference's own output
(tests/golden/c3x_concentration.npz) and against NumPy restatements on the host mirror of the projections (tests/conc_host.py).

Counts and sums of integer-valued weights are integer additions resp. exact float64 additions: bit for bit.  Sums of real-valued
weights: 1e-12 relative per bin.  The device's projection and the references' (the C oracle behind the golden file, projection.Proj
behind the restatements) differ by rounding, 2e-9 m at most here; the golden file holds no entry within 1e-6 m of an edge and the
clouds below are drawn so (_clear_of_edges), so the same bins are expected.  Edges in metres agree to 1e-7 m (the issue's 1e-9 degrees
are 1e-4 m), lon_array / lat_array to 1e-9 degrees.  In the golden cases without corners the first two bins of either axis are merged
(conc_host.merge_first_bins: the reference puts its second edge on the smallest coordinate itself)."""
import numpy as np
import pytest

import conc_host
from conftest import golden
from opendrift_amd import projection

pytestmark = pytest.mark.gpu
STRANDED = 2
CATEGORIES = ['active', 'missing_data', 'stranded']
NAMES = ('H', 'H_submerged', 'H_stranded')
CORNERS = ('llcrnrlon', 'llcrnrlat', 'urcrnrlon', 'urcrnrlat')
LAEA = '+proj=laea +lat_0=60 +lon_0=5 +ellps=WGS84'
QUAD = '+proj=stere +lat_0=90 +lon_0=70 +lat_ts=60 +ellps=WGS84'
MOLL = '+proj=moll +ellps=WGS84 +lon_0=0.0'
Z_ARRAY = np.array([-10000.0, -100.0, -30.0, -10.0, -2.0, 0.0])
NSPECIES = 3


@pytest.fixture(scope='module')
def g():
    return golden('c3x_concentration.npz')


def grid(proj4, pixel=1000.0, nx=None, ny=None):
    """np.arange edges in `proj4` around the plume of cloud(): pixel metres, or nx / ny edges over the same spans.  For QUAD the lower
    left corner is far enough out for 1.5 * the maxima to fall inside."""
    P = projection.Proj(proj4)
    x, y = P(np.array([4.55, 5.25]), np.array([59.95, 60.25]))
    (x0, x1), (y0, y1) = sorted(x), sorted(y)
    if proj4 == QUAD:
        x1, y1 = x1 + 15000.0, y1 + 15000.0
        x0, y0 = 1.5 * x1 - 2.5 * pixel, 1.5 * y1 - 2.5 * pixel
    xs = np.arange(x0, x1, pixel if nx is None else (x1 - x0) / (nx - 0.5))
    ys = np.arange(y0, y1, pixel if ny is None else (y1 - y0) / (ny - 0.5))
    return P, xs, ys


def outside_bin(xs, ys):
    from opendrift_amd.oceandrift import edge_bin
    ix, iy = edge_bin(max(xs) * 1.5, xs), edge_bin(max(ys) * 1.5, ys)
    return ix * (len(ys) - 1) + iy if ix >= 0 and iy >= 0 else -1


_CLOUDS = {}


def cloud(ntraj, nt):
    """[trajectory, time] float32 lon, lat, z, status, specie, integer-valued and real-valued weights: a plume around 4.9 E 60.1 N, a
    fifth of the entries NaN (late releases), some outside the grids, z on layer bounds / 0 / -0.0 / NaN / positive, stranded entries,
    species 0 .. 2 and some that are none.  Made once per size and never written to."""
    if (ntraj, nt) not in _CLOUDS:
        rng = np.random.default_rng(77 * nt + ntraj)
        shape = (ntraj, nt)
        core = rng.uniform(size=(ntraj, 1)) < 0.5
        lon = np.where(core, rng.normal(4.9, 0.01, shape), rng.uniform(4.5, 5.3, shape))
        lat = np.where(core, rng.normal(60.1, 0.005, shape), rng.uniform(59.9, 60.3, shape))
        z = -rng.uniform(0.1, 150.0, shape)
        u = rng.uniform(size=shape)
        z[u < 0.3] = 0.0
        z[u < 0.08] = -0.0
        z[(u > 0.80) & (u < 0.9)] = rng.choice(Z_ARRAY, shape)[(u > 0.80) & (u < 0.9)]
        z[(u > 0.9) & (u < 0.92)] = 0.5
        z[u > 0.98] = np.nan
        status = np.where(rng.uniform(size=shape) < 0.15, STRANDED, np.where(rng.uniform(size=shape) < 0.05, 1, 0)).astype(float)
        specie = rng.integers(0, NSPECIES + 1, shape).astype(float)
        specie[rng.uniform(size=shape) < 0.02] = np.nan
        wint = rng.integers(1, 10, shape).astype(float)
        wreal = rng.uniform(0.05, 3.0, shape) * 10.0 ** rng.integers(-3, 4, shape)
        late = np.arange(nt)[None, :] < np.where(rng.uniform(size=ntraj) < 0.4, rng.integers(0, nt + 1, ntraj), 0)[:, None]
        out = [lon, lat, z, status, specie, wint, wreal]
        for a in out:
            a[late] = np.nan
        _CLOUDS[ntraj, nt] = tuple(np.ascontiguousarray(a, np.float32) for a in out)
        for a in _CLOUDS[ntraj, nt]:
            a.setflags(write=False)
    return _CLOUDS[ntraj, nt]


def _clear_of_edges(P, a, xs, ys, tol=1e-6):
    """no finite entry within tol of an edge: the device and the host mirror then agree on every bin"""
    with np.errstate(invalid='ignore'):
        x, y = P(a[0].astype(np.float64), a[1].astype(np.float64))
    ok = np.isfinite(x) & np.isfinite(y)
    dx = np.abs(x[ok][:, None] - xs[np.clip(np.searchsorted(xs, x[ok])[:, None] + np.array([-1, 0]), 0, len(xs) - 1)]).min()
    dy = np.abs(y[ok][:, None] - ys[np.clip(np.searchsorted(ys, y[ok])[:, None] + np.array([-1, 0]), 0, len(ys) - 1)]).min()
    return min(dx, dy) > tol


def same(got, want, what, names=NAMES):
    for h, w, name in zip(got, want, names):
        assert h.dtype == np.float64 and h.shape == w.shape, (what, name)
        assert np.array_equal(h, w, equal_nan=True), '%s %s: %d bins differ, sums %r / %r' % (what, name, (h != w).sum(), np.nansum(h), np.nansum(w))


def close(got, want, what, rtol=1e-12):
    for h, w, name in zip(got, want, NAMES):
        assert np.array_equal(np.isnan(h), np.isnan(w)), (what, name)
        ok = ~np.isnan(w)
        assert (np.abs(h[ok] - w[ok]) <= rtol * np.abs(w[ok])).all(), (what, name, np.abs(h[ok] - w[ok]).max())


def masks_both(ctx, proj4, a, xs, ys, P, weight=None, code=STRANDED, **kw):
    lon, lat, z, status = a[:4]
    ob = outside_bin(xs, ys)
    got = ctx.density_map_proj(P.params, lon, lat, z, status, xs, ys, weight=weight, stranded_code=code, outside_bin=ob, **kw)
    return got, conc_host.density_proj_maps(P, lon, lat, z, status, xs, ys, weight, code), ob


# ------------------------------------------------------------------------------------------------ the golden cases, through the model
def _model(g, pop='nan', cls=None, categories=CATEGORIES, times=None):
    from opendrift_amd.oceandrift import OceanDrift
    o = (cls or OceanDrift)(loglevel=50)
    arrays = {k: g['%s_%s' % (pop, k)] for k in ('lon', 'lat', 'z', 'status', 'specie', 'mass', 'mass_int')}
    if times is not None:
        arrays = {k: np.ascontiguousarray(v[:, times]) for k, v in arrays.items()}
    o.result = dict(time=list(range(arrays['lon'].shape[1])), **arrays)
    o.status_categories = list(categories)
    o.nspecies = int(g['nspecies'])
    return o


def _grid_agrees(g, case, lon_array, lat_array):
    assert lon_array.dtype == lat_array.dtype == np.float64 and lon_array.shape == lat_array.shape == g[case + '_lon_array'].shape
    assert np.abs(lon_array - g[case + '_lon_array']).max() < 1e-9 and np.abs(lat_array - g[case + '_lat_array']).max() < 1e-9


@pytest.mark.parametrize('case,pop,weight', [('laea', 'nan', None), ('laea_nostr', 'nan', None), ('laea_wint', 'nan', 'mass_int'),
                                             ('laea_wreal', 'nan', 'mass'), ('laea_single', 'nan', None), ('utm', 'full', None),
                                             ('default', 'full', None), ('quad', 'nan', None), ('quad_wreal', 'nan', 'mass')])
def test_golden_density_cases_through_the_model(has_gpu, g, case, pop, weight):
    times = [int(g['single_time_index'])] if case.endswith('single') else None
    o = _model(g, pop, categories=CATEGORIES[:2] if case == 'laea_nostr' else CATEGORIES, times=times)
    kw = {k: float(g['%s_%s' % (case, k)]) for k in CORNERS} if case + '_llcrnrlon' in g else {}
    out = o.get_density_array_proj(float(g[case + '_pixelsize_m']), density_proj=str(g[case + '_proj4']) or None, weight=weight, **kw)
    merge = (lambda a: a) if kw else conc_host.merge_first_bins
    want = [g['%s_%s' % (case, n)] for n in NAMES]
    assert all(h.shape == w.shape for h, w in zip(out[:3], want))
    if weight == 'mass':
        close([merge(h) for h in out[:3]], [merge(w) for w in want], case)
    else:
        same([merge(h) for h in out[:3]], [merge(w) for w in want], case)
    _grid_agrees(g, case, out[3], out[4])
    if case.startswith('quad'):
        ix, iy = g[case + '_outside_bin']
        assert np.nansum(out[0][:, ix, iy]) > 0 and (np.isnan(out[2][:, ix, iy]).any() == (weight is not None))


@pytest.mark.parametrize('case,pop', [('rn', 'nan'), ('rn_full', 'full'), ('rn_single', 'nan')])
def test_golden_radionuclide_cases_through_the_model(has_gpu, g, case, pop):
    from opendrift_amd.radionuclides import RadionuclideDrift
    times = [int(g['single_time_index'])] if case.endswith('single') else None
    o = _model(g, pop, cls=RadionuclideDrift, times=times)
    kw = {k: float(g['%s_%s' % (case, k)]) for k in CORNERS} if case + '_llcrnrlon' in g else {}
    H, lon_array, lat_array = o.get_radionuclide_density_array(float(g[case + '_pixelsize_m']), g['z_array'], density_proj=str(g[case + '_proj4']), **kw)
    merge = (lambda a: a) if kw else conc_host.merge_first_bins
    assert H.shape == g[case + '_H'].shape
    same([merge(H)], [merge(g[case + '_H'])], case, names=('H', ))
    _grid_agrees(g, case, lon_array, lat_array)
    assert o.ctx.conc_last_kernel_ms() > 0


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('nt', [1, 6, 63, 64, 65])
@pytest.mark.parametrize('ntraj', [257, 300])
def test_shapes_equal_the_numpy_restatement(ctx, ntraj, nt):
    """the combining loop and its end (n_times below, at and above a wave), a partial workgroup; counts, integer weights and species"""
    a = cloud(ntraj, nt)
    for proj4 in (LAEA, QUAD):
        P, xs, ys = grid(proj4, 20000.0 if proj4 == QUAD else 1000.0)
        assert _clear_of_edges(P, a, xs, ys)
        got, want, ob = masks_both(ctx, proj4, a, xs, ys, P)
        same(got, want, 'counts ' + proj4)
        assert (ob >= 0) == (proj4 == QUAD) and all(w.sum() > 0 for w in want)
        got, want, _ = masks_both(ctx, proj4, a, xs, ys, P, weight=a[5])
        same(got, want, 'integer weights ' + proj4)
    P, xs, ys = grid(LAEA)
    got = ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, NSPECIES)
    want = conc_host.species_layer_maps(P, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, NSPECIES)
    same([got], [want], 'species', names=('H', ))
    assert (want.sum(axis=(0, 2, 3, 4)) > 0).all() and (want.sum(axis=(0, 1, 3, 4)) > 0).all()      # every species, every layer


def test_no_stranded_category_and_real_weights(ctx):
    a = cloud(300, 6)
    P, xs, ys = grid(QUAD, 20000.0)
    got, want, _ = masks_both(ctx, QUAD, a, xs, ys, P, code=-1)
    same(got, want, 'no stranded category')
    assert not got[2].any()
    got, want, ob = masks_both(ctx, QUAD, a, xs, ys, P, weight=a[6])
    close(got, want, 'real weights')
    assert np.isnan(want[2].reshape(6, -1)[:, ob]).any()      # a NaN weight of a removed entry


def test_three_slabs(ctx, monkeypatch):
    """257 trajectories x 6 times, four host arrays: a budget of 100 rows of 4 * 6 * 4 B makes three slabs of whole trajectories, the
    boundaries inside the data; then one trajectory per slab"""
    a = cloud(257, 6)
    P, xs, ys = grid(QUAD, 20000.0)
    whole = masks_both(ctx, QUAD, a, xs, ys, P)[0]
    whole_w = masks_both(ctx, QUAD, a, xs, ys, P, weight=a[5])[0]
    species = ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, NSPECIES)
    extent = ctx.proj_extent(P.params, a[0], a[1])
    monkeypatch.setenv('ODR_CONC_SLAB_BYTES', str(100 * 4 * 6 * 4))
    same(masks_both(ctx, QUAD, a, xs, ys, P)[0], whole, 'counts in slabs')
    same(masks_both(ctx, QUAD, a, xs, ys, P, weight=a[5])[0], whole_w, 'integer weights in slabs')
    same([ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, NSPECIES)], [species], 'species in slabs', names=('H', ))
    assert ctx.proj_extent(P.params, a[0], a[1]) == extent
    monkeypatch.setenv('ODR_CONC_SLAB_BYTES', '1')
    same(masks_both(ctx, QUAD, a, xs, ys, P)[0], whole, 'one trajectory per slab')
    assert ctx.proj_extent(P.params, a[0], a[1]) == extent


def test_device_pointers(ctx):
    """the inputs as device arrays: the float32 environment slots of a particle set with one element per entry hold them"""
    a = cloud(300, 65)
    P, xs, ys = grid(QUAD, 20000.0)
    n = a[0].size
    S = ctx.particles(n)
    S.append(np.zeros(n), np.zeros(n))
    for k in range(6):
        S.env_upload(k, a[k].ravel())
    ctx.sync()
    ptr = [S.device_ptr('env:%d' % k) for k in range(6)]
    ob = outside_bin(xs, ys)
    want = conc_host.density_proj_maps(P, *a[:4], xs, ys, a[5], STRANDED)
    got = ctx.density_map_proj(P.params, *ptr[:4], xs, ys, weight=ptr[5], stranded_code=STRANDED, outside_bin=ob, shape=a[0].shape)
    same(got, want, 'device pointers')
    got = ctx.density_map_proj(P.params, ptr[0], a[1], ptr[2], a[3], xs, ys, weight=a[5], stranded_code=STRANDED, outside_bin=ob, shape=a[0].shape)
    same(got, want, 'device and host arrays mixed')
    got = ctx.species_layer_map(P.params, ptr[0], ptr[1], a[2], ptr[4], xs, ys, Z_ARRAY, NSPECIES, shape=a[0].shape)
    same([got], [conc_host.species_layer_maps(P, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, NSPECIES)], 'species', names=('H', ))
    assert ctx.proj_extent(P.params, ptr[0], ptr[1], n=n) == ctx.proj_extent(P.params, a[0], a[1])
    S.close()


@pytest.mark.parametrize('nx,ny', [(2040, 2050), (3000, 1200)])
def test_edge_counts_around_the_lds_limit(ctx, nx, ny):
    """4090 edges sit in LDS, 4200 are read from memory (the limit is 4096); a few hundred entries, one output time"""
    a = cloud(300, 1)
    P, xs, ys = grid(LAEA, nx=nx, ny=ny)
    assert (len(xs), len(ys)) == (nx, ny) and _clear_of_edges(P, a, xs, ys, 1e-7)
    got, want, _ = masks_both(ctx, LAEA, a, xs, ys, P)
    same(got, want, 'counts')
    assert want[0].sum() > 50 and want[1].sum() > 50
    zb = Z_ARRAY[[0, 3, 5]]
    got = ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], xs, ys, zb, 2)
    same([got], [conc_host.species_layer_maps(P, a[0], a[1], a[2], a[4], xs, ys, zb, 2)], 'species', names=('H', ))


@pytest.mark.parametrize('proj4', ['', LAEA, MOLL])
def test_extent_with_nan_in_the_first_and_last_workgroup(ctx, proj4):
    """257 x 7 entries = 8 workgroups, the last partial; every entry of the first workgroup and the last 100 are NaN or hold one NaN
    coordinate; the extremes are those of the finite projected positions (longlat: exactly)"""
    lon, lat = (np.array(v) for v in cloud(257, 7)[:2])
    flat_lon, flat_lat = lon.reshape(-1), lat.reshape(-1)
    flat_lon[:256:2] = np.nan
    flat_lat[1:256:2] = np.nan
    flat_lon[-100:] = np.nan
    params = projection.parse_proj4(proj4) if proj4 else None
    got = ctx.proj_extent(params, lon, lat)
    with np.errstate(invalid='ignore'):
        x, y = projection.Proj(proj4 or '+proj=longlat')(lon.astype(np.float64), lat.astype(np.float64))
    ok = np.isfinite(x) & np.isfinite(y)
    assert 0 < ok.sum() < ok.size - 356
    want = (x[ok].min(), x[ok].max(), y[ok].min(), y[ok].max())
    assert np.abs(np.array(got) - want).max() <= (1e-7 if proj4 else 0.0), (got, want)
    assert ctx.proj_extent(params, np.full(70, np.nan), np.zeros(70)) == (np.inf, -np.inf, np.inf, -np.inf)


@pytest.mark.parametrize('proj4', [LAEA, QUAD, MOLL, '+proj=utm +zone=31 +ellps=WGS84', '+proj=merc +lat_ts=60 +ellps=WGS84'])
def test_grid_lonlat_is_the_inverse_projection_of_the_meshgrid(ctx, proj4):
    P, xs, ys = grid(proj4, 1500.0)
    lon, lat = ctx.proj_grid_lonlat(P.params, xs, ys)
    Y, X = np.meshgrid(ys, xs)
    wlon, wlat = P(X, Y, inverse=True)
    assert lon.shape == (len(xs), len(ys)) and len(xs) != len(ys)
    assert np.abs(lon - wlon).max() < 1e-9 and np.abs(lat - wlat).max() < 1e-9


@pytest.mark.parametrize('n', [0, 1, 3, 60])
def test_box_smooth(ctx, g, n):
    """n = 60 is larger than the plane.  The golden plane against the reference, the 5-D H plane by plane against the host build."""
    a = g['smooth_in']
    assert np.array_equal(ctx.box_smooth(a, n), g['smooth_n%d' % n])
    H = g['rn_H']
    s = ctx.box_smooth(H, n)
    assert s.shape == H.shape
    for idx in ((0, 0, 0), (4, 1, 2), (5, 2, 4)):
        assert np.array_equal(s[idx], conc_host.box(H[idx], n))


# ------------------------------------------------------------------------------------------------ Mollweide, the model run
def test_mollweide_default_of_the_radionuclide_method(has_gpu, g):
    from opendrift_amd.radionuclides import RadionuclideDrift
    o = _model(g, 'full', cls=RadionuclideDrift)
    H, lon_array, lat_array = o.get_radionuclide_density_array(1000.0, g['z_array'])
    P = projection.Proj(MOLL)
    x, y = P(g['full_lon'].astype(np.float64), g['full_lat'].astype(np.float64))
    xs, ys = np.arange(x.min() - 1000.0, x.max() + 1000.0, 1000.0), np.arange(y.min() - 1000.0, y.max() + 1000.0, 1000.0)
    assert H.shape[3:] == (len(xs) - 1, len(ys) - 1)
    want = conc_host.species_layer_maps(P, *(g['full_' + k] for k in ('lon', 'lat', 'z', 'specie')), xs, ys, g['z_array'], 3)
    same([conc_host.merge_first_bins(H)], [conc_host.merge_first_bins(want)], 'moll', names=('H', ))
    assert H.sum() == want.sum() > 1000
    Y, X = np.meshgrid(ys, xs)
    wlon, wlat = P(X, Y, inverse=True)
    assert np.abs(lon_array - wlon).max() < 1e-9 and np.abs(lat_array - wlat).max() < 1e-9


def test_existing_entry_points_refuse_mollweide(ctx):
    from opendrift_amd import _abi, device
    d = device.proj_desc(projection.parse_proj4(MOLL), map_grid=True)
    with pytest.raises(ValueError):
        ctx.ftle_map(d, np.arange(3.0), np.arange(4.0), 1.0, 3600.0, np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32))
    assert d.kind == _abi.PROJ_MOLL


def test_invalid_arguments(ctx):
    a = cloud(257, 6)
    P, xs, ys = grid(LAEA)
    bad = [(xs[:1], ys), (xs[::-1], ys), (xs, np.array([0.0, 1.0, 1.0])), (np.array([0.0, np.nan, 5.0]), ys), (xs, np.array([0.0, np.inf]))]
    for ex, ey in bad:
        with pytest.raises(ValueError):
            ctx.density_map_proj(P.params, *a[:4], ex, ey)
        with pytest.raises(ValueError):
            ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], ex, ey, Z_ARRAY, NSPECIES)
    for zb in ([-1.0], [-1.0, -1.0], [0.0, -1.0], [-1.0, np.nan], [-np.inf, 0.0]):
        with pytest.raises(ValueError):
            ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], xs, ys, zb, NSPECIES)
    with pytest.raises(ValueError):
        ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, 0)
    with pytest.raises(ValueError):      # 2^28 bins per output time, species and layers included
        ctx.species_layer_map(P.params, a[0], a[1], a[2], a[4], np.arange(4098.0), np.arange(4098.0), np.arange(-17.0, 1.0), 1)
    with pytest.raises(ValueError):
        ctx.density_map_proj(P.params, *a[:4], xs, ys, outside_bin=(len(xs) - 1) * (len(ys) - 1))
    from opendrift_amd import device
    for refused in ('+proj=ob_tran +o_proj=longlat +o_lat_p=30 +o_lon_p=10 +lon_0=5', ):
        d = device.proj_desc(projection.parse_proj4(refused))
        with pytest.raises(ValueError):
            ctx.density_map_proj(d, *a[:4], xs, ys)
        with pytest.raises(ValueError):
            ctx.proj_extent(d, a[0], a[1])
        with pytest.raises(ValueError):
            ctx.proj_grid_lonlat(d, xs, ys)
    d = device.proj_desc(P.params)
    d.kind = 3      # ODR_PROJ_CURVILINEAR
    with pytest.raises(ValueError):
        ctx.species_layer_map(d, a[0], a[1], a[2], a[4], xs, ys, Z_ARRAY, NSPECIES)
    d.kind = 10
    with pytest.raises(ValueError):
        ctx.density_map_proj(d, *a[:4], xs, ys)
    with pytest.raises(ValueError):
        ctx.box_smooth(np.array([[1.0, np.nan], [0.0, 2.0]]), 1)
    with pytest.raises(ValueError):
        ctx.box_smooth(np.ones((3, 4)), -1)


def test_radionuclide_run_then_maps():
    """a short RadionuclideDrift run of C30's case (a), a few hundred elements: per output time H sums to the elements inside the grid
    and the layers, and get_density_array_proj's maps sum to get_density_array's"""
    import radio_host as R
    import test_gpu_radionuclides as tr
    G = R.Golden()
    o, steps = tr._model(G, 'a', 'device', seed=2, n=300, steps=6)
    o.run(time_step=G.dt('a'), steps=steps)
    r = o.result
    nt = r['lon'].shape[1]
    assert nt == steps + 1 and r['lon'].shape[0] == 300 and hasattr(o, 'depthintervals')
    zb = [-10000.0, -20.0, -5.0, -1.0, 0.0]
    H, lon_array, lat_array = o.get_radionuclide_density_array(500.0, zb)
    assert H.shape[:3] == (nt, o.nspecies, 4) and H.shape[3:] == (lon_array.shape[0] - 1, lon_array.shape[1] - 1)
    z, sp = r['z'].astype(np.float64), r['specie']
    inside = np.isfinite(r['lon']) & (z > zb[0]) & (z <= zb[-1]) & (sp >= 0) & (sp < o.nspecies)      # the grid holds every finite position
    assert np.array_equal(H.sum(axis=(1, 2, 3, 4)), inside.sum(axis=0)) and inside.sum() > 0
    for k in range(o.nspecies):
        assert np.array_equal(H[:, k].sum(axis=(1, 2, 3)), (inside & (sp == k)).sum(axis=0))
    s = o.horizontal_smooth(H, 1)
    assert s.shape == H.shape and np.array_equal(s[-1, 0, 0], conc_host.box(H[-1, 0, 0], 1))
    Hp = o.get_density_array_proj(500.0, density_proj='+proj=utm +zone=31 +ellps=WGS84')      # (x, y > 0: the removed entries fall outside)
    Hd = o.get_density_array(500.0)
    for a, b, name in zip(Hp[:3], Hd[:3], NAMES):
        assert np.array_equal(a.sum(axis=(1, 2)), b.sum(axis=(1, 2))), name
    assert Hp[0].sum() + Hp[1].sum() > 0
