"""GPU: StructuredReader.set_convolution_kernel -- the convolution pass of the level preparation (k_blk_convolve, k_blk_convolve_zy;
csrc/odr_convolve.hip.h) against the reference's own results (golden C41, tools/gen_golden_reader_convolution.py).

  a  prepared levels, read back with odr_block_read, against the reference's __convolve_block__ output bit for bit wherever the
     convolved and then masked value is finite (the sea-floor fill and the dilation only give values to NaN cells), on every way a
     level becomes resident: synchronous, asynchronous, from device memory (the way regridded s-levels arrive), and prepared variable
     by variable (ODR_ROW_DILATE); the K plane against the node records with a kernel set;
  b  odr_env_sample of a reader with convolve = 3 against the reference's get_variables_interpolated, bit for bit; the profile of a
     3-D variable by sampling at the depths of the levels;
  c  the reference's two runs on a convolved current and wind: every status equal, positions within the 1e-7 deg that
     tests/test_gpu_parity.py applies to runs against the reference's golden vectors (replay.compare, tol_pos);
  d  a reader whose kernel was set and cleared, and one never touched, give the same levels bit for bit."""
from datetime import datetime, timedelta

import numpy as np
import pytest

import convolve_host as H
from opendrift_amd import readers
from opendrift_amd._abi import VARIABLES

pytestmark = pytest.mark.gpu

T0 = datetime(2020, 1, 1)
U, V, W, KZ = 'x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity', 'ocean_vertical_diffusivity'
XW, YW, TEMP, DEPTH, LAND = 'x_wind', 'y_wind', 'sea_water_temperature', 'sea_floor_depth_below_sea_level', 'land_binary_mask'
RUN_BOUND = 1e-7      # deg: tests/test_gpu_parity.py, runs against the reference's golden vectors (replay.compare(..., tol_pos=1e-7))
CASES = H.block_cases()
IDS = [c[0] for c in CASES]


def _source(ctx, raw, conv):
    ny, nx = next(iter(raw.values())).shape[-2:]
    nz = max([a.shape[0] for a in raw.values() if a.ndim == 3] + [1])
    sid = ctx.add_grid(4.0 + 0.05 * np.arange(nx), 59.0 + 0.05 * np.arange(ny), z=-5.0 * np.arange(nz) if nz > 1 else None)
    if conv is not None:
        ctx.set_convolution(sid, readers.convolution_weights(conv), three_d=[v for v, a in raw.items() if a.ndim == 3 and a.shape[0] == 1])
    return sid


def _check_level(ctx, sid, slot, raw, out, what):
    for v in raw:
        got = ctx.read_block(sid, slot, v)
        H.assert_prepared_equals(got.reshape(raw[v].shape), out[v], '%s %s' % (what, v))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_prepared_levels_equal_the_reference_on_every_upload_path(ctx, monkeypatch, case):
    name, conv, raw, out = case
    sid = _source(ctx, raw, conv)
    ctx.upload_block(sid, 0, 0.0, {v: a.copy() for v, a in raw.items()})
    _check_level(ctx, sid, 0, raw, out, name + ' synchronous')
    pinned = {v: ctx.pin(np.ascontiguousarray(a)) for v, a in raw.items()}
    ctx.upload_block_async(sid, 1, 3600.0, pinned)
    ctx.commit_block(sid, 1)
    _check_level(ctx, sid, 1, raw, out, name + ' asynchronous')
    for a in pinned.values():
        ctx.unpin(a)
    # device memory: each variable parked in an environment array of a particle set (the way regridded s-levels arrive)
    n = max(a.size for a in raw.values())
    P = ctx.particles(n)
    P.append(np.full(n, 4.0), np.full(n, 59.0))
    ptrs, nzv = {}, {}
    for v, a in raw.items():
        P.env_upload(v, np.resize(a.ravel(), n))
        ptrs[v] = P.device_ptr('env:%d' % VARIABLES[v])
        nzv[v] = a.shape[0] if a.ndim == 3 else 1
    ctx.upload_block_device(sid, 2, 7200.0, ptrs, nzv)
    _check_level(ctx, sid, 2, raw, out, name + ' device memory')
    _check_level(ctx, sid, 0, raw, out, name + ' synchronous, after the others')
    P.close()
    # the preparation variable by variable takes the same pass
    monkeypatch.setenv('ODR_ROW_DILATE', '1')
    ctx.upload_block(sid, 3, 10800.0, {v: a.copy() for v, a in raw.items()})
    monkeypatch.delenv('ODR_ROW_DILATE')
    _check_level(ctx, sid, 3, raw, out, name + ' variable by variable')
    # switched off: the next level is the raw block again
    ctx.set_convolution(sid, None)
    ctx.upload_block(sid, 1, 3600.0, {v: a.copy() for v, a in raw.items()})
    _check_level(ctx, sid, 1, raw, raw, name + ' switched off')


def test_a_nan_under_a_zero_weight_does_not_spread(ctx):
    g = H.golden()
    raw, want = {XW: g['a_zero_raw']}, g['a_zero_out']
    sid = _source(ctx, raw, CASES[IDS.index('k35')][1])
    ctx.upload_block(sid, 0, 0.0, raw)
    H.assert_prepared_equals(ctx.read_block(sid, 0, XW), want, 'zero weight')
    assert np.isnan(want).sum() == 14 and np.isfinite(ctx.read_block(sid, 0, XW)).all()      # (the dilation filled the 14 cells)


def test_kernel_larger_than_the_grid_and_the_largest_kernel(ctx):
    rng = np.random.default_rng(3)
    m = H.max_edge()
    for (ky, kx), shapes in (((m, m), {XW: (3, 5), U: (2, 3, 5)}), ((m, 4), {XW: (40, 70), U: (3, 40, 70)})):
        k = rng.normal(size=(ky, kx))
        raw = {v: rng.normal(size=s).astype(np.float32) for v, s in shapes.items()}
        sid = _source(ctx, raw, k)
        ctx.upload_block(sid, 0, 0.0, raw)
        want = readers.convolve_block({v: a.copy() for v, a in raw.items()}, k)
        _check_level(ctx, sid, 0, raw, want, '%d x %d' % (ky, kx))
    with pytest.raises(ValueError, match='at most %d x %d' % (m, m)):
        ctx.set_convolution(sid, np.ones((m + 1, 2)))
    w = np.ones((m + 1, 2))
    import ctypes as C
    rc = ctx.lib.odr_source_set_convolution(ctx.h, sid, m + 1, 2, w.ctypes.data_as(C.POINTER(C.c_double)), 0, None)
    assert rc != 0 and b'at most' in ctx.lib.odr_last_error()


def test_ensemble_members_are_refused_by_name(ctx):
    rng = np.random.default_rng(4)
    members = [rng.normal(size=(6, 7)).astype(np.float32) for _ in range(3)]
    sid = _source(ctx, {XW: members[0]}, 3)
    with pytest.raises(ValueError, match='ensemble members'):
        ctx.upload_block(sid, 0, 0.0, {XW: members})


def test_the_k_plane_is_written_from_the_convolved_values(ctx):
    rng = np.random.default_rng(8)
    nz, ny, nx = 6, 33, 41
    raw = {U: rng.normal(size=(nz, ny, nx)).astype(np.float32), V: rng.normal(size=(nz, ny, nx)).astype(np.float32),
           KZ: rng.uniform(1e-4, 1e-1, (nz, ny, nx)).astype(np.float32), DEPTH: rng.uniform(20, 60, (ny, nx)).astype(np.float32)}
    raw[KZ][3:, 5, 7] = np.nan
    sid = _source(ctx, raw, 3)
    ctx.upload_block(sid, 0, 0.0, raw)
    plane, recs = ctx.kplane_read(sid, 0)
    assert np.array_equal(H.bits(plane), H.bits(recs))
    want = readers.convolve_block({KZ: raw[KZ].copy()}, 3)[KZ]
    H.assert_prepared_equals(np.moveaxis(plane[..., :nz], -1, 0), want, 'K plane')
    assert not np.array_equal(np.moveaxis(plane[..., :nz], -1, 0), raw[KZ])


def test_sigma_reader_is_convolved_after_the_regridding(ctx):
    """SigmaGridReader: the s-levels are regridded to the z levels on the device (odr_sgrid_zslice) and handed to the preparation as
    device pointers; the convolution sees the regridded arrays, as the reference convolves what get_variables returns."""
    rng = np.random.default_rng(9)
    N, ny, nx = 5, 19, 35
    x, y = 4.0 + 0.05 * np.arange(nx), 59.0 + 0.05 * np.arange(ny)
    h = rng.uniform(30, 120, (ny, nx))
    Cs_r = -np.linspace(0.9, 0.05, N) ** 2
    a3 = {v: rng.normal(size=(1, N, ny, nx)).astype(np.float32) for v in (U, V)}
    a2 = {DEPTH: h[None].astype(np.float32)}
    r = readers.SigmaGridReader(x, y, [T0], a3, a2, h=h, hc=10.0, Cs_r=Cs_r)
    r.set_convolution_kernel(3)
    b = readers.DeviceReaderBinding(ctx, r)
    b.ensure_levels(T0, T0, times=[T0])
    raw = {}
    for v in (U, V):
        _, z64 = b.sgrid.zslice(a3[v][0], r.z, want_float64=True, slot=7)
        raw[v] = z64.astype(np.float32)
    raw[DEPTH] = a2[DEPTH][0]
    want = readers.convolve_block({v: a.copy() for v, a in raw.items()}, 3)
    for v in raw:
        got = ctx.read_block(b.sid, b.slots[0], v)
        H.assert_prepared_equals(got, want[v], 'sigma ' + v)
        assert not np.array_equal(got, raw[v])


def test_a_convolving_leaf_of_a_reader_expression(ctx):
    g = H.golden()
    current, _ = _run_readers(g, 3)
    plain, _ = _run_readers(g, 'untouched')
    n = 200
    rng = np.random.default_rng(2)
    lon, lat = rng.uniform(g['c_x'][3], g['c_x'][-4], n), rng.uniform(g['c_y'][3], g['c_y'][-4], n)
    t = T0 + timedelta(seconds=900)
    out = {}
    for tag, leaf in (('conv', current), ('plain', plain)):
        b = readers.DeviceReaderBinding(ctx, leaf + readers.ConstantReader({U: 0.25, V: -0.5}), variables=[U, V])
        P = ctx.particles(n)
        P.append(lon, lat)
        b.sample_combined(P, [U, V], [True, True], t)
        out[tag] = {v: P.env_download(v) for v in (U, V)}
        P.close()
    own = readers.DeviceReaderBinding(ctx, _run_readers(g, 3)[0])
    own.ensure_levels(t, t, times=[t])
    for v in (U, V):
        ctx.bind(v, [own.sid], np.nan)
    P = ctx.particles(n)
    P.append(lon, lat)
    direct = P.env_sample([U, V], readers._epoch(t), download=True)
    P.close()
    for v, c in ((U, 0.25), (V, -0.5)):
        assert np.array_equal(out['conv'][v], (direct[v].astype(np.float64) + c).astype(np.float32)) or \
            np.array_equal(out['conv'][v], direct[v] + np.float32(c)), v
        assert np.abs(out['conv'][v] - out['plain'][v]).max() > 1e-3, v


def _times(seconds):
    return [T0 + timedelta(seconds=float(s)) for s in seconds]


def test_env_sample_equals_the_reference_interpolation(ctx):
    g = H.golden()
    variables = [str(v) for v in g['b_vars']]
    r = readers.GridReader(g['b_x'], g['b_y'], _times(g['b_seconds']), {v: g['b_field_' + v] for v in variables}, z=g['b_z'])
    r.set_convolution_kernel(3)
    b = readers.DeviceReaderBinding(ctx, r)
    t = T0 + timedelta(seconds=float(g['b_call_seconds']))
    b.ensure_levels(t, t, times=[t])
    for v in variables:
        ctx.bind(v, [b.sid], np.nan)
    P = ctx.particles(len(g['b_lon']))
    P.append(g['b_lon'], g['b_lat'], z=g['b_zq'])
    got = P.env_sample(variables, readers._epoch(t), download=True)
    for v in variables:
        want = g['b_env_' + v]
        diff = np.flatnonzero(H.bits(got[v]) != H.bits(want))
        print(v, 'differing', len(diff), got[v][diff[:3]], want[diff[:3]])
        assert H.same_bits(got[v], want), (v, len(diff))
    # the profile of the reference: the horizontal interpolation at every level of the block
    prof = g['b_profile_' + TEMP]
    for k, zk in enumerate(g['b_profile_z']):
        Pk = ctx.particles(len(g['b_lon']))
        Pk.append(g['b_lon'], g['b_lat'], z=np.full(len(g['b_lon']), float(zk)))
        gk = Pk.env_sample([TEMP], readers._epoch(t), download=True)[TEMP]
        Pk.close()
        diff = np.flatnonzero(H.bits(gk) != H.bits(prof[k]))
        print('profile level', k, zk, 'differing', len(diff), gk[diff[:3]], prof[k][diff[:3]])
        assert H.same_bits(gk, prof[k]), (k, len(diff))
    P.close()


def _run_readers(g, conv):
    times = _times(g['c_seconds'])
    current = readers.GridReader(g['c_x'], g['c_y'], times, {v: g['c_field_' + v] for v in (U, V)}, name='current')
    wind = readers.GridReader(g['c_x'], g['c_y'], times, {v: g['c_field_' + v] for v in (XW, YW)}, name='wind')
    if conv != 'untouched':
        current.set_convolution_kernel(conv)
        wind.set_convolution_kernel(conv)
    return current, wind


def _run(g, scheme, conv):
    from opendrift_amd.oceandrift import OceanDrift
    o = OceanDrift(loglevel=50, seed=0, rng='numpy')
    o.add_reader(list(_run_readers(g, conv)))
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:advection_scheme', scheme)
    o.set_config('drift:stokes_drift', False)
    o.seed_elements(lon=g['c_lon'], lat=g['c_lat'], time=T0, wind_drift_factor=float(g['c_wdf']))
    o.run(time_step=float(g['c_dt']), steps=int(g['c_steps']))
    return o


@pytest.mark.parametrize('scheme,tag', [('euler', 'euler'), ('runge-kutta4', 'rk4')])
def test_runs_on_a_convolved_current_and_wind(scheme, tag):
    g = H.golden()
    o = _run(g, scheme, int(g['c_kernel']))
    e = o.elements
    lon, lat, status = g['c_%s_lon' % tag], g['c_%s_lat' % tag], g['c_%s_status' % tag]
    assert len(e) == lon.shape[1] and np.array_equal(np.asarray(e.status), status[-1][e.ID])
    dmax = max(np.abs(e.lon - lon[-1][e.ID]).max(), np.abs(e.lat - lat[-1][e.ID]).max())
    print(tag, 'convolved readers on the device vs the reference: %.2e deg' % dmax)
    assert dmax < RUN_BOUND
    assert np.hypot(e.lon - lon[0][e.ID], e.lat - lat[0][e.ID]).min() > 1000 * RUN_BOUND      # every element moved
    grids = [b for b in o.readers.values() if b.is_grid()]
    assert len(grids) == 2 and all(len(b.slots) + len(b.staged) >= 2 for b in grids)      # the run crossed a level change


def test_a_cleared_kernel_and_an_untouched_reader_give_the_same_levels(ctx):
    g = H.golden()
    levels = {}
    for how in ('untouched', None, 3):
        current, _ = _run_readers(g, how)
        if how is None:
            current.set_convolution_kernel(5)
            current.set_convolution_kernel(None)
        b = readers.DeviceReaderBinding(ctx, current)
        b.prefetch = False
        b.ensure_levels(T0, T0, times=[T0])
        levels[how] = {v: ctx.read_block(b.sid, b.slots[0], v) for v in (U, V)}
    for v in (U, V):
        assert np.array_equal(H.bits(levels['untouched'][v]), H.bits(levels[None][v])), v
        assert np.array_equal(H.bits(levels['untouched'][v]), H.bits(g['c_field_' + v][0])), v
        assert not np.array_equal(levels[3][v], levels['untouched'][v]), v
