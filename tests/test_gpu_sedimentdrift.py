"""GPU: SedimentDrift -- the resuspension kernel (odr_resuspend) against what the reference did, the sea-floor action
ODR_SEAFLOOR_SETTLE in every kernel that honours it against a NumPy restatement of the reference's sub-step loop with the
model's hook, and the model run end to end against the reference's own SedimentDrift (golden c26,
tools/gen_golden_sediment.py)."""
from datetime import datetime, timedelta

import numpy as np
import pytest

from conftest import golden
from opendrift_amd import readers
from opendrift_amd._abi import OdrError
from opendrift_amd.device import Context
from opendrift_amd.sedimentdrift import SedimentDrift

import sediment_host
from test_sediment_device_arithmetic import golden_steps

pytestmark = pytest.mark.gpu
T0 = datetime(2020, 1, 1)
U, V, W, KZ = 'x_sea_water_velocity', 'y_sea_water_velocity', 'upward_sea_water_velocity', 'ocean_vertical_diffusivity'
DEPTH, SSH, LAND = 'sea_floor_depth_below_sea_level', 'sea_surface_height', 'land_binary_mask'
XW, YW, MLD = 'x_wind', 'y_wind', 'ocean_mixed_layer_thickness'
NAMES = [U, V, W, KZ, DEPTH, LAND]
# no decision of a comparison below is marginal (as condition (e) of the golden's generator): the restatement measures the
# distances and the tests require them
Z_MARGIN = 1e-4


# ------------------------------------------------------------------------------------------------ k_resuspend
def _resuspend(ctx, u, v, threshold, moving, z, count=True):
    n = len(u)
    P = ctx.particles(n)
    P.append(np.linspace(3, 4, n), np.full(n, 60.0), z=z, moving=moving)
    P.env_upload(U, u)
    P.env_upload(V, v)
    got = P.resuspend(threshold, count=count)
    d = P.download()
    P.close()
    return d['moving'], d['z'], got


def test_kernel_reproduces_the_reference_and_the_host_build(ctx):
    """moving and z after resuspension() bit for bit, for every step of the golden (about 400 elements: two workgroups, the
    second one partial); the returned count is the reference's; device and host build agree."""
    g = golden('c26_sedimentdrift.npz')
    threshold = float(g['threshold'])
    total = 0
    for u, v, m0, z0, m1, z1 in golden_steps(g):
        m, z, count = _resuspend(ctx, u, v, threshold, m0, z0)
        assert np.array_equal(m, m1) and np.array_equal(z.view(np.uint64), z1.view(np.uint64))
        assert count == int(((m0 == 0) & (m1 == 1)).sum())
        hm, hz, hcount = sediment_host.resuspend(u, v, threshold, m0, z0)
        assert np.array_equal(m, hm) and np.array_equal(z.view(np.uint64), hz.view(np.uint64)) and count == hcount
        total += count
    assert total >= 20


def test_kernel_over_several_workgroups_equals_the_host_build(ctx):
    """3001 elements (twelve workgroups, one element in the last), half of them settled, speeds on both sides of the threshold
    and exactly on it; with and without the count."""
    n = 3001
    rng = np.random.default_rng(11)
    t32 = np.float32(0.2)
    u = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    v = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    u[::50], v[::50] = t32, 0            # exactly the threshold: not resuspended
    u[1::50], v[1::50] = np.nextafter(t32, np.float32(1)), 0
    moving = (rng.random(n) < 0.5).astype(np.int32)
    moving[-1] = 0
    u[-1], v[-1] = 0.3, 0.3
    z = -rng.uniform(4, 34, n)
    hm, hz, hcount = sediment_host.resuspend(u, v, 0.2, moving, z)
    assert 300 < hcount < 1200 and hm[-1] == 1
    for count in (True, False):
        m, zz, got = _resuspend(ctx, u, v, 0.2, moving, z, count=count)
        assert np.array_equal(m, hm) and np.array_equal(zz.view(np.uint64), hz.view(np.uint64))
        assert got == (hcount if count else None)
    m, zz, got = _resuspend(ctx, u, v, 3, moving, z)       # nothing is that fast
    assert got == 0 and np.array_equal(m, moving) and np.array_equal(zz, z)


def test_entry_reports_missing_currents(ctx):
    P = ctx.particles(8)
    P.append(np.linspace(3, 4, 8), np.full(8, 60.0), z=np.full(8, -5.0), moving=np.zeros(8, np.int32))
    with pytest.raises(OdrError, match='x_sea_water_velocity') as e:
        P.resuspend(0.2)
    assert e.value.code == -4                               # ODR_ERR_STATE
    P.env_upload(U, np.full(8, 1.0, np.float32))
    with pytest.raises(OdrError) as e:                      # the other component still missing
        P.resuspend(0.2)
    assert e.value.code == -4
    assert (P.download()['moving'] == 0).all()
    P.env_upload(V, np.zeros(8, np.float32))
    assert P.resuspend(0.2) == 8 and (P.download()['moving'] == 1).all()
    P.close()


# ------------------------------------------------------------------------------------------------ the settle action
def _reference_mixing(z, moving, tv, Zmin, mixing_z, Kprofiles, dt, dt_mix, uniforms):
    """oceandrift.py:500-561 in NumPy (drift:vertical_mixing_at_surface False, no surface_wave_mixing) with
    interact_with_seafloor 'lift_to_seafloor' and SedimentDrift.bottom_interaction (sedimentdrift.py:108-116) as the hook.
    Returns z, moving and, per element, the smallest |z - Zmin| at a sea-floor check while it was moving."""
    z, moving = z.copy(), moving.copy()
    cols = np.arange(len(z))
    gradK = -np.gradient(Kprofiles, mixing_z, axis=0)
    gradK[np.abs(gradK) < 1e-10] = 0
    margin = np.full(len(z), np.inf)
    for i in range(abs(int(dt / dt_mix))):
        surface = z == 0
        zi = np.round(np.interp(-z, -mixing_z, np.arange(len(mixing_z)))).astype(int)    # (interp1d, ends extended)
        Kz, dKdz = Kprofiles[zi, cols], gradK[zi, cols]
        R = 2 * uniforms[i] - 1
        r = 1.0 / 3
        z = z - moving * (dKdz * dt_mix - R * np.sqrt((Kz * np.abs(dt_mix) * 2 / r)))
        z[z >= 0] = -z[z >= 0]
        b = (z < Zmin) & (moving == 1)
        z[b] = 2 * Zmin[b] - z[b]
        z = z + tv * dt_mix * moving
        z[surface] = 0.
        z[z > 0] = 0
        mv = moving == 1
        margin[mv] = np.minimum(margin[mv], np.abs(z[mv] - Zmin[mv]))
        below = z < Zmin
        if below.any():
            z[below] = Zmin[below]                              # interact_with_seafloor()
            moving[(z <= Zmin) & (moving == 1)] = 0             # bottom_interaction(Zmin)
    return z, moving, margin


def _settle_case(g, n=3100, seed=5):
    """Candidate elements over the golden's shallow sea floor, up to 8 m above it, sinking at 2 - 20 mm/s; every tenth lies
    settled on it.  (The tests drop the candidates whose decision would be marginal and keep about 3000: twelve workgroups,
    the last one partial.)"""
    rng = np.random.default_rng(seed)
    x, y = g['g_x'], g['g_y']
    lon, lat = rng.uniform(x[4], x[-5], n), rng.uniform(y[4], y[-5], n)
    tv = -rng.uniform(0.002, 0.02, n).astype(np.float32)
    moving = np.ones(n, np.int32)
    moving[::10] = 0
    return lon, lat, rng.uniform(0.05, 8.0, n), tv, moving, rng.uniform(0, 1, (10, n))


def _device_world(g, klev=None):
    """The golden's grid; klev: a diffusivity that is the same at every node of a level (the column of every element is klev,
    whatever the horizontal interpolation does to the last bit)."""
    ctx = Context(seed=1)
    sid = ctx.add_grid(g['g_x'], g['g_y'], z=g['g_z'])
    for k in range(3):
        blk = {nm: g['g_' + nm][k] for nm in NAMES}
        if klev is not None:
            blk[KZ] = np.broadcast_to(np.float32(klev)[:, None, None], blk[KZ].shape).copy()
        ctx.upload_block(sid, k, float(g['g_t'][k]), blk)
    for nm in NAMES:
        ctx.bind(nm, [sid], {DEPTH: 10000.0}.get(nm, 0.0))
    for nm, fb in ((SSH, 0.0), (XW, 0.0), (YW, 0.0), (MLD, 50.0)):
        ctx.bind(nm, [], fb)
    return ctx


KLEV = np.float32([1e-2, 9e-3, 7e-3, 4e-3, 3e-3, 2e-3, 1.5e-3, 1e-3])      # the golden's eight levels, 0 ... -100 m


@pytest.mark.parametrize('lane', ['column', 'window', 'generic', 'constant', 'windspeed_Large1994'])
def test_settle_action_in_the_mixing_kernels(monkeypatch, lane):
    """ODR_SEAFLOOR_SETTLE with host uniforms in k_vmix_col (K columns of a reader), k_vmix_win (the same, five levels in
    registers), the generic k_vmix (the same profiles; and 'constant': no K source at all) and k_vmix_wind (the analytic
    lane; calm, so that Large et al.'s profile is depth / MLD * background): moving, status and the z of every settled
    element equal the restatement's; the other elements' z within 1e-6 m (the device forms K and the walk in its own
    operation order: differences of a few float64 / float32 roundings of metre-sized values)."""
    g = golden('c26_sedimentdrift.npz')
    dt, dt_mix = 600.0, 60.0
    lon, lat, above, tv, moving, uni = _settle_case(g)
    if lane == 'windspeed_Large1994':
        bg = 1e-2
        mixing_z = -np.arange(0, 52.0)             # -arange(0, MLD.max() + 2), MLD = 50 (oceandrift.py:430)
        kcol = np.where(np.arange(52) >= 50, bg, np.arange(52) / 50.0 * bg)      # physics_methods.py:246-247 without wind
    else:
        mixing_z = g['g_z'].astype(np.float64)
        kcol = np.full(8, 0.02) if lane == 'constant' else KLEV.astype(np.float64)
    # the input: the candidates no decision of which is marginal, by the restatement on the sea floor the device samples
    c = _device_world(g)
    P = c.particles(len(lon))
    P.append(lon, lat, z=np.full(len(lon), -1.0))
    P.env_sample([DEPTH, SSH], 0.0)
    Zmin = -1. * (P.env_download(DEPTH) + P.env_download(SSH))
    P.close()
    c.close()
    z0 = Zmin + above
    z0[moving == 0] = Zmin[moving == 0]
    _, _, margin = _reference_mixing(z0, moving, tv, Zmin, mixing_z, np.repeat(kcol[:, None], len(lon), axis=1), dt, dt_mix, uni)
    keep = margin > 10 * Z_MARGIN
    assert 0.95 * len(lon) < keep.sum() and keep.sum() % 256 != 0
    lon, lat, tv, moving, uni, z0, Zmin_cpu = lon[keep], lat[keep], tv[keep], moving[keep], np.ascontiguousarray(uni[:, keep]), z0[keep], Zmin[keep]
    n = len(lon)
    monkeypatch.setenv('ODR_VMIX_WINDOW', '1' if lane == 'window' else '0')
    if lane == 'generic':
        monkeypatch.setenv('ODR_NO_FAST_PATH', '1')
    ctx = _device_world(g, KLEV)
    if lane == 'constant':      # vertical_mixing 'constant' (oceandrift.py:445-449): the fallback at every level, no reader
        ctx.bind(KZ, [], 0.02)
    P = ctx.particles(n)
    P.append(lon, lat, z=np.full(n, -1.0), terminal_velocity=tv)
    P.env_sample([U, V, W, DEPTH, SSH, XW, YW, MLD], 0.0)
    Zmin = -1. * (P.env_download(DEPTH) + P.env_download(SSH))
    assert Zmin.dtype == np.float32 and -35 < Zmin.min() and Zmin.max() < -3.9 and np.array_equal(Zmin, Zmin_cpu)
    P.upload(z=z0, moving=moving)
    P.store_previous()
    ctx.set_seafloor_action('settle')
    if lane == 'windspeed_Large1994':
        P.vmix_analytic(lane, bg, dt, dt_mix, uniforms=uni)
    else:
        P.vmix(0.0, dt, dt_mix, uniforms=uni)
    d = P.download()
    P.close()
    ctx.close()
    zr, mr, margin = _reference_mixing(z0, moving, tv, Zmin, mixing_z, np.repeat(kcol[:, None], n, axis=1), dt, dt_mix, uni)
    print('%s: settled %d of %d, smallest |z - Zmin| at a check %.3g m, largest |dz| %.3g m'
          % (lane, int(((moving == 1) & (mr == 0)).sum()), n, margin.min(), np.abs(d['z'] - zr).max()))
    assert margin.min() > Z_MARGIN
    newly = (moving == 1) & (mr == 0)
    assert newly.sum() > n // 10 and (mr == 1).sum() > n // 10          # both outcomes in numbers
    assert np.array_equal(d['moving'], mr)
    assert (d['status'] == 0).all()                                      # settled elements stay active
    settled = mr == 0
    assert np.array_equal(d['z'][settled], Zmin[settled].astype(np.float64))      # on the sea floor, bit for bit
    assert np.array_equal(d['z'][moving == 0], z0[moving == 0])                   # (the ones that lay there did not move)
    assert np.abs(d['z'] - zr).max() < 1e-6
    assert np.array_equal(d['lon'], lon) and np.array_equal(d['lat'], lat)


def test_settle_action_in_vertical_buoyancy(ctx):
    """odr_vertical_buoyancy (oceandrift.py:352-368) with the hook: bit for bit (one float32 product, one float64 sum)."""
    g = golden('c26_sedimentdrift.npz')
    lon, lat, above, tv, moving, _ = _settle_case(g, seed=6)
    n, dt = len(lon), 600.0
    c = _device_world(g)
    P = c.particles(n)
    P.append(lon, lat, z=np.full(n, -1.0), terminal_velocity=tv)
    P.env_sample([DEPTH, SSH], 0.0)
    Zmin = -1. * (P.env_download(DEPTH) + P.env_download(SSH))
    z0 = Zmin + above                # up to 8 m above the floor, sinking 1.2 - 12 m
    z0[moving == 0] = Zmin[moving == 0]
    # the input: an element that would come to lie within 1 mm of the sea floor starts 1 m higher
    near = (moving == 1) & (np.abs(z0 + tv * dt - Zmin) < 10 * Z_MARGIN)
    z0[near] += 1.0
    P.upload(z=z0, moving=moving)
    P.store_previous()
    c.set_seafloor_action('settle')
    P.vertical_buoyancy(dt)
    d = P.download()
    P.close()
    c.close()
    z = z0.copy()
    oc = z < 0
    z[oc] = np.minimum(0, z[oc] + tv[oc] * dt)
    assert np.abs(z[moving == 1] - Zmin[moving == 1]).min() > Z_MARGIN
    below = z < Zmin
    mr = moving.copy()
    z[below] = Zmin[below]
    mr[(z <= Zmin) & (mr == 1)] = 0
    assert below.sum() > n // 10 and (mr == 1).sum() > n // 10
    assert np.array_equal(d['moving'], mr) and (d['status'] == 0).all()
    assert np.array_equal(d['z'].view(np.uint64), z.view(np.uint64))


# ------------------------------------------------------------------------------------------------ the model
class _Recording(SedimentDrift):
    """SedimentDrift that keeps the state of the active elements after every update() (its own update(): still the
    call-by-call lane)."""

    def update(self):
        super().update()
        d = self.P.download()
        self.records.append({k: d[k].copy() for k in ('ID', 'lon', 'lat', 'z', 'status', 'moving')})


def _reader(g):
    times = [T0 + timedelta(seconds=float(t)) for t in g['g_t']]
    return readers.GridReader(g['g_x'], g['g_y'], times, {k: g['g_' + k] for k in NAMES}, z=g['g_z'])


def _final(o, n):
    lon, lat, z, status = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1)
    for d in (o.elements, o.elements_deactivated):
        lon[d.ID], lat[d.ID], z[d.ID], status[d.ID] = d.lon, d.lat, d.z, d.status
    return lon, lat, z, status


def test_run_numpy_rng_reproduces_the_reference():
    """rng='numpy': np.random is drawn in the reference's call order, so the run reproduces the reference's SedimentDrift:
    status and moving of every element after every step identical, lon / lat / z at the tolerances of the PelagicEggDrift run
    test (tests/test_gpu_pelagicegg.py).  The largest differences are printed."""
    g = golden('c26_sedimentdrift.npz')
    steps, n = g['lon'].shape[0] - 1, g['lon'].shape[1]
    o = _Recording(loglevel=50, seed=0, rng='numpy')
    o.records = []
    o.add_reader(_reader(g))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('vertical_mixing:timestep', 60)
    o.seed_elements(lon=g['lon'][0], lat=g['lat'][0], z=g['z'][0], time=T0, terminal_velocity=g['terminal_velocity'])
    res = o.run(time_step=600, steps=steps)
    assert o.steps_calculation == steps and len(o.records) == steps
    worst = dict(lon=0.0, lat=0.0, z=0.0)
    for k, r in enumerate(o.records):
        ID = r['ID']
        assert np.array_equal(np.sort(ID), np.flatnonzero(g['moving_after'][k] >= 0))      # the same elements are present
        assert np.array_equal(r['moving'], g['moving'][k + 1][ID]), 'moving after step %d' % k
        assert np.array_equal(r['status'], g['status'][k + 1][ID]), 'status after step %d' % k
        for q in worst:
            worst[q] = max(worst[q], float(np.abs(r[q] - g[q][k + 1][ID]).max()))
    lon, lat, z, status = _final(o, n)
    print('largest differences over all steps: lon %.3g lat %.3g deg, z %.3g m' % (worst['lon'], worst['lat'], worst['z']))
    assert worst['lon'] < 1e-7 and worst['lat'] < 1e-7 and worst['z'] < 1e-5
    assert np.abs(lon - g['lon'][-1]).max() < 1e-7 and np.abs(lat - g['lat'][-1]).max() < 1e-7
    assert np.abs(z - g['z'][-1]).max() < 1e-5
    assert np.array_equal(status, g['status'][-1])
    # the input covers settling, staying settled and resuspension (conditions (a) - (c) of the generator)
    m = np.stack([r['moving'].sum() for r in o.records])
    assert (m < n).any()
    e = o.elements
    assert e.terminal_velocity.dtype == np.float32 and np.array_equal(e.terminal_velocity, g['terminal_velocity'][e.ID])
    assert np.array_equal(e.moving, g['moving'][-1][e.ID]) and (e.settled == 0).all()
    for k in ('settled', 'moving', 'terminal_velocity', U):
        assert res[k].shape == (n, steps + 1)
    assert 'sea_surface_wave_mean_period_from_variance_spectral_density_second_frequency_moment' not in res
    # nothing speculated the mixing launch, nothing took a static or fused lane
    assert o._vmix_speculated is False


def _device_run(threshold, n=3000, steps=6, seed=3):
    g = golden('c26_sedimentdrift.npz')
    o = _Recording(loglevel=50, seed=seed, rng='device')
    o.records = []
    o.add_reader(_reader(g))
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('vertical_mixing:timestep', 60)
    o.set_config('vertical_mixing:resuspension_threshold', threshold)
    rng = np.random.default_rng(7)
    x, y = g['g_x'], g['g_y']
    lon, lat = rng.uniform(x[6], x[-12], n), rng.uniform(y[6], y[-7], n)
    tv = -np.exp(rng.uniform(np.log(0.0005), np.log(0.02), n)).astype(np.float32)
    o.seed_elements(lon=lon, lat=lat, z=rng.uniform(-3.5, -0.5, n), time=T0, terminal_velocity=tv)
    o.run(time_step=600, steps=steps)
    by_id = []
    for r in o.records:     # by element ID (NaN / -1: not present)
        row = {q: np.full(n, np.nan) for q in ('lon', 'lat', 'z')}
        row['moving'] = np.full(n, -1)
        for q in row:
            row[q][r['ID']] = r[q]
        by_id.append(row)
    return o, by_id


def test_device_rng_is_reproducible_and_settled_elements_do_not_move():
    a, ra = _device_run(0.2)
    b, rb = _device_run(0.2)
    for u, v in zip(ra, rb):
        for q in u:
            assert np.array_equal(u[q], v[q], equal_nan=True), q
    frozen = resuspended = 0
    for p, q in zip(ra[:-1], ra[1:]):
        still = (p['moving'] == 0) & (q['moving'] == 0)       # settled after one step and after the next: not resuspended in between
        assert np.array_equal(p['lon'][still], q['lon'][still]) and np.array_equal(p['lat'][still], q['lat'][still])
        frozen += int(still.sum())
        resuspended += int(((p['moving'] == 0) & (q['moving'] == 1)).sum())
        moved = (p['moving'] == 1) & (q['moving'] >= 0)
        assert (p['lon'][moved] != q['lon'][moved]).mean() > 0.99
    print('settled over two consecutive steps: %d element-steps; resuspended a step later: %d' % (frozen, resuspended))
    assert frozen > 100


def test_threshold_3_resuspends_nothing_and_threshold_0_everything():
    o, rec = _device_run(3.0)
    settled = [int((r['moving'] == 0).sum()) for r in rec]
    print('threshold 3: settled after each step', settled)
    assert settled == sorted(settled) and settled[-1] > 300
    for p, q in zip(rec[:-1], rec[1:]):
        assert not ((p['moving'] == 0) & (q['moving'] == 1)).any()
    o, rec = _device_run(0.0)
    speed = np.hypot(o.environment.x_sea_water_velocity, o.environment.y_sea_water_velocity)
    assert (speed > 0).all()
    for r in rec:
        assert not (r['moving'] == 0).any()
    assert o.elements.z.min() < -3.9      # (elements did reach the sea floor: 4 m at its shallowest)


def _sorted_run(sort_every, n=80000, steps=5):
    g = golden('c26_sedimentdrift.npz')
    o = SedimentDrift(loglevel=50, seed=1, rng='device')
    o.add_reader(_reader(g))
    o.set_config('drift:advection_scheme', 'euler')
    o.set_config('vertical_mixing:timestep', 60)
    o.set_config('vertical_mixing:resuspension_threshold', 0.25)
    o.set_config('environment:fallback:x_sea_water_velocity', None)      # leaving the reader's domain: missing data
    o.set_config('environment:fallback:y_sea_water_velocity', None)
    o.sort_every = sort_every
    rng = np.random.default_rng(5)
    x, y = g['g_x'], g['g_y']
    lon, lat = rng.uniform(x[0], x[-8], n), rng.uniform(y[0], y[-1], n)
    settled = (np.arange(n) % 7).astype(np.float32) / 7
    tv = -rng.uniform(0.002, 0.02, n).astype(np.float32)
    o.seed_elements(lon=lon, lat=lat, z=rng.uniform(-3.5, -0.5, n), time=T0, terminal_velocity=tv, settled=settled)
    o.run(time_step=900, steps=steps)
    return o, settled


def test_moving_and_settled_survive_compaction_and_the_periodic_sort():
    """More elements than the re-sort threshold of run(), a re-sort in EVERY step, elements that leave the domain at its edge:
    the device order is no longer the seeding order, every element still carries the `settled` it was seeded with, and
    moving / z / lon / lat by element ID are those of the same run without any re-sort (the draws are keyed by element ID)."""
    a, settled = _sorted_run(1)
    b, _ = _sorted_run(0)
    ea, eb = a.elements, b.elements
    gone = a.num_elements_deactivated()
    print('deactivated', gone, 'settled at the end', int((ea.moving == 0).sum()), 'of', len(ea.ID))
    assert gone > 0 and len(ea.ID) + gone == len(settled) and len(ea.ID) > 65536
    assert not (np.diff(a.P.ids()) > 0).all()                # the device order is no longer the seeding order
    assert np.array_equal(ea.settled, settled[ea.ID])
    assert (ea.moving == 0).sum() > 1000 and (ea.moving == 1).sum() > 1000
    ia, ib = np.argsort(ea.ID), np.argsort(eb.ID)
    assert np.array_equal(ea.ID[ia], eb.ID[ib])
    for q in ('moving', 'z', 'lon', 'lat', 'settled', 'terminal_velocity'):
        assert np.array_equal(getattr(ea, q)[ia], getattr(eb, q)[ib]), q
