"""GPU: the static 12-level mixing launch that gathers two aligned K quads per particle (k_vmix_col<3, TL, VMixC3W / VMixC3RecW>,
csrc/odr_kernels.hip.h) computes what the whole-column static launch (ODR_NO_VMIX_WINDOW=1) and the run-time launch
(ODR_NO_VMIX_SPEC=1) compute, byte for byte -- for starting levels at both ends of the profile and on both sides of the switch
of the resident quads, from the K planes and from the node records, and when sub-steps leave the resident levels (those elements
are redone on the whole column inside the launch: odr_particles_vmix_window_stats counts them)."""
import functools

import numpy as np
import pytest

import bench
from opendrift_amd import synthetic as synth
from opendrift_amd.device import Context

pytestmark = pytest.mark.gpu

KZ = 'ocean_vertical_diffusivity'
N = 20000
MODES = {'window': None, 'full': 'ODR_NO_VMIX_WINDOW', 'runtime': 'ODR_NO_VMIX_SPEC'}
# depth >= 496 m over this rectangle of the synthetic field (its sea floor: 50 + 450 (0.5 + 0.5 sin(2 X + 1) cos(1.5 Y)))
DEEP = dict(lon=(2.3, 3.4), lat=(60.05, 60.5))


@functools.lru_cache(maxsize=None)
def _fields(kscale=1):
    f = bench.make_fields('c3', small=True)
    g = synth.grid3d(nx=128, ny=96, nz=12, nt=3, seed=0)
    if kscale != 1:
        g = dict(g, **{KZ: g[KZ] * np.float32(kscale)})
    return dict(f, g=g, z=g['z'])


def _run(monkeypatch, mode, seeds, steps, kscale=1, records=False):
    for var in MODES.values():
        if var:
            monkeypatch.delenv(var, raising=False)
    if MODES[mode]:
        monkeypatch.setenv(MODES[mode], '1')
    if records:
        monkeypatch.setenv('ODR_NO_KPLANE', '1')
    else:
        monkeypatch.delenv('ODR_NO_KPLANE', raising=False)
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    wl = bench.Workload('c3', ctx, _fields(kscale), (0, 0, 1), via_torch=False)
    lon, lat, z = seeds
    P = ctx.particles(len(lon))
    P.append(lon, lat, z=z, id=np.arange(len(lon), dtype=np.int32))
    for k in steps:
        t = wl.time_of(k)
        if k % 2 == 0:   # bench.Workload.step's one-call form: the step launch, then the mixing launch
            P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False,
                               seafloor=True, age_dt=wl.dt, vmix=dict(dt_mix=wl.dt_mix, step=k, vertical_advection=False))
        else:
            P.env_coast_advect(wl.vars, t, wl.scheme, wl.dt, coastline='previous', store_previous=True, count=False,
                               seafloor=True, age_dt=wl.dt)
            P.vmix(t, wl.dt, wl.dt_mix, step=k, fuse_vertical_advection=False)
    out = P.download(), P.vmix_window_stats(), P.vmix_layout_stats(), P.vmix_kplane_stats()
    P.close()
    ctx.close()
    return out


def _same(a, b):
    assert len(a['ID']) == len(b['ID'])
    for k in ('ID', 'lon', 'lat', 'z', 'status', 'moving'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def _three(monkeypatch, seeds, steps, kscale=1, records=False):
    """The three launches on the same seeds; checks the counters and the bytes.  Returns the windowed run."""
    nl = len(list(steps))
    w, ww, lw, kw = _run(monkeypatch, 'window', seeds, steps, kscale, records)
    f, wf, lf, kf = _run(monkeypatch, 'full', seeds, steps, kscale, records)
    r, wr, lr, kr = _run(monkeypatch, 'runtime', seeds, steps, kscale, records)
    assert ww['windowed'] == nl and ww['full'] == 0, ww
    assert wf == dict(windowed=0, full=nl, redone=0), wf
    assert wr == dict(windowed=0, full=0, redone=0), wr
    assert lw == lf == dict(runtime=0, static=nl, other=0), (lw, lf)
    assert lr == dict(runtime=nl, static=0, other=0), lr
    assert kw == kf == kr == (dict(planes=0, records=nl) if records else dict(planes=nl, records=0)), (kw, kf, kr)
    _same(w, f)
    _same(w, r)
    return w, ww


def _mixed_seeds():
    """C3's seeding over the whole water column, plus elements in the NaN coast strip and outside the grid (fallback K)."""
    rng = np.random.default_rng(3)
    f = _fields()
    lon, lat, _ = bench.seed_particles('c3', f, N, rng)
    z = -rng.uniform(0, 480, N)
    z[:200] = 0.0
    lon[1000:1400] = rng.uniform(9.75, 9.99, 400)      # X > 0.97: land, K is NaN there
    lon[1400:1600] = rng.uniform(10.2, 11.0, 200)      # east of the grid
    lat[1600:1800] = rng.uniform(58.0, 59.9, 200)      # south of it
    return lon, lat, z


@pytest.mark.parametrize('records', [False, True], ids=['planes', 'records'])
def test_two_quad_launch_is_bit_identical(monkeypatch, records):
    seeds = _mixed_seeds()
    w, _ = _three(monkeypatch, seeds, range(7), records=records)      # steps 0 and 6 on a reader level
    assert not np.array_equal(w['z'], seeds[2][w['ID']])


def _level_of(d, zm):
    """vmix_col_walk's starting level: boundaries below d (odd ones count when d >= zm, even ones when d > zm)"""
    k = np.arange(len(zm))
    return np.where(k % 2 == 1, d[:, None] >= zm, d[:, None] > zm).sum(axis=1)


@pytest.mark.parametrize('first', [0, 1], ids=['on_level', 'between_levels'])
def test_window_placement_at_every_level_boundary(monkeypatch, first):
    zl = -_fields()['z']
    zm = 0.5 * (zl[:-1] + zl[1:])
    d = np.concatenate([[0.0], zm, np.nextafter(zm, 0), np.nextafter(zm, 1e9), zm - 1e-3, zm + 1e-3, zl[1:],
                        [1000.0, 1000.0]])          # (the last two: below the sea floor, the step launch lifts them onto it)
    lv0 = np.clip(_level_of(np.minimum(d, 496.0), zm), 1, 10)
    q0 = np.minimum(np.maximum(lv0 - 2, 0) >> 2, 1)
    assert {1, 5, 6, 10} <= set(lv0.tolist()) and set(q0.tolist()) == {0, 1}
    rng = np.random.default_rng(5)
    rep = 64
    z = -np.repeat(d, rep)
    lon = rng.uniform(*DEEP['lon'], len(z))
    lat = rng.uniform(*DEEP['lat'], len(z))
    _three(monkeypatch, (lon, lat, z), range(first, first + 2))


def test_sub_steps_that_leave_the_resident_levels_are_redone(monkeypatch):
    rng = np.random.default_rng(7)
    lon = rng.uniform(*DEEP['lon'], N)
    lat = rng.uniform(*DEEP['lat'], N)
    z = -rng.uniform(0, 480, N)
    # K x 2000: about 100 m per sub-step at the surface -- a sub-step spans several levels
    _, ww = _three(monkeypatch, (lon, lat, z), range(3), kscale=2000)
    assert ww['redone'] > 0, ww
