"""CPU: readers.SchismReader without a device -- its host mirror (scipy's cKDTree and NumPy, written from the reference's
expressions) against the reference's own answers (tests/golden/c41_schism.npz) bit for bit, construction and shapes, every refusal by
name, the use_3d rules, the time selection, the lane a model with such a reader takes, what run() refuses, and the C ABI names."""
from datetime import datetime, timedelta

import numpy as np
import pytest

import schism_host as S
from opendrift_amd import _abi, readers
from opendrift_amd.oceandrift import OceanDrift

T0 = datetime(2020, 1, 1)
H = timedelta(hours=1)
SSH, DEPTH, U_, V_ = S.SSH, S.DEPTH, S.U_, S.V_


@pytest.fixture(scope='module')
def g():
    return np.load(S.GOLDEN)


@pytest.mark.parametrize('case', ['a', 'b'])
def test_host_mirror_equals_the_reference(g, case):
    r = S.golden_reader(g, case)
    assert r.device_kind == 'schism' and r.use_3d == (case == 'a') and r.geographic == (case == 'b')
    names = [str(n) for n in g['names_' + case]]
    x, y = g[case + '_x'], g[case + '_y']
    for k, sec in enumerate(g['query_seconds']):
        m = g[case + '_group'] == k
        z = g[case + '_z'][m].astype(np.float64)
        t = T0 + timedelta(seconds=int(sec))
        plain = r.get_variables(names, t, x[m], y[m], z, rotate=False)      # (a: the positions as the reference searched with them)
        for n in names:
            assert S.same_bits(plain[n], g['%s_%s' % (case, n)][m]), (case, sec, n)
        turned = r.get_variables_interpolated(names, t, g[case + '_lon'][m], g[case + '_lat'][m], z)
        if case == 'b':      # a geographic mesh is not rotated; lon / lat ARE its coordinates
            for n in names:
                assert S.same_bits(turned[n], plain[n])
            continue
        if not r.covers_time(t):
            continue
        # the neighbours and distances of the mirror's trees are the reference's
        cov = r.covers_positions(x[m], y[m])
        kk = np.flatnonzero(m)[cov]
        d, i = r.nearest3(x[kk], y[kk])
        assert np.array_equal(i, g['a_i2'][kk]) and np.array_equal(d, g['a_d2'][kk])
        kb = r.time_weight(t, names)[0]
        d, i = r.nearest3(x[kk], y[kk], z[cov], kb)
        assert np.array_equal(i, g['a_i3b'][kk]) and np.array_equal(d, g['a_d3b'][kk])
        # rotated: the mirror forms the angle with this package's geodesic routine, the reference with PROJ's: one float32 ulp
        u, v = g['a_' + U_][m], g['a_' + V_][m]
        bound = S.ulp32(np.maximum(np.abs(u), np.abs(v)))
        for n, key in ((U_, 'a_rot_u'), (V_, 'a_rot_v')):
            want = g[key][m]
            assert np.array_equal(np.isnan(turned[n]), np.isnan(want))
            ok = np.isfinite(want)
            assert (np.abs(turned[n][ok].astype(np.float64) - want[ok]) <= bound[ok]).all(), (sec, n)


def small(**kw):
    rng = np.random.default_rng(0)
    x, y = 400000.0 + 1000.0 * rng.random(7), 6500000.0 + 1000.0 * rng.random(7)
    zcor = np.tile(np.array([-10.0, -5.0, 0.0], np.float32), (3, 7, 1))
    args = dict(x=x, y=y, times=[T0, T0 + H, T0 + 2 * H], proj4=S.UTM, zcor=zcor,
                node_arrays={DEPTH: np.arange(7.0), SSH: np.arange(21.0).reshape(3, 7), U_: np.arange(3 * 7 * 3.0).reshape(3, 7, 3),
                             V_: np.ones((3, 7, 3))})
    args.update(kw)
    return readers.SchismReader(**args), args


def test_construction_and_shapes():
    r, a = small()
    assert r.use_3d is True and not r.geographic and r.n_levels == 3 and r.zcor.dtype == np.float32
    assert all(v.dtype == np.float32 for v in r.node_arrays.values())
    assert r.levels_of(U_) == 3 and r.levels_of(SSH) == 0 and r.level(DEPTH, 2).shape == (7,) and r.level(U_, 1).shape == (7, 3)
    assert len(r.hull_x) >= 3 and r.covers_positions(a['x'].mean(), a['y'].mean()).all()
    assert not r.covers_positions([a['x'].min() - 1.0, np.nan], [a['y'].mean(), a['y'].mean()]).any()
    out = r.get_variables([DEPTH, SSH, U_], T0 + H, [a['x'].mean()], [a['y'].mean()], [-5.0])
    assert all(v.dtype == np.float32 and v.shape == (1,) and np.isfinite(v).all() for v in out.values())
    # exactly ON an inner node, at its middle level, at a time level: that point's own values (the 1e-10 floor)
    from scipy.spatial import ConvexHull
    k = [k for k in range(7) if k not in ConvexHull(np.c_[a['x'], a['y']]).vertices][0]      # (a hull vertex is not strictly inside)
    on = r.get_variables([DEPTH, SSH, U_], T0 + H, a['x'][k:k + 1], a['y'][k:k + 1], [-5.0], rotate=False)
    assert np.allclose([on[DEPTH][0], on[SSH][0], on[U_][0]], [k, 7.0 + k, 21 + k * 3 + 1.0], rtol=1e-6)
    masked = np.ma.masked_less(np.arange(21.0).reshape(3, 7), 3.0)
    r2, _ = small(node_arrays={SSH: masked})
    assert np.isnan(r2.node_arrays[SSH][0, :3]).all() and np.isfinite(r2.node_arrays[SSH][0, 3:]).all()
    inf = a['zcor'].copy()
    inf[0, 0, 2], inf[1, 1, 0] = np.inf, -np.inf
    r3, _ = small(zcor=inf)
    assert r3.zcor[0, 0, 2] == 15.0 and r3.zcor[1, 1, 0] == 15.0


def test_use_3d_rules():
    two_d = {DEPTH: np.arange(7.0), U_: np.ones((3, 7)), V_: np.ones((3, 7))}
    assert small(node_arrays=two_d, zcor=None)[0].use_3d is False
    with pytest.raises(ValueError, match='zcor must be present'):
        small(zcor=None, use_3d=True)
    with pytest.raises(NotImplementedError, match='depth-averaged'):      # None without zcor: 2-D, and the 3-D arrays have no place
        small(zcor=None)
    with pytest.raises(NotImplementedError, match='depth-averaged'):
        small(use_3d=False)
    rng = np.random.default_rng(1)
    with pytest.raises(NotImplementedError, match='geographic'):      # degrees by the proj4
        small(x=4 + rng.random(7), y=60 + rng.random(7), proj4='+proj=latlong')
    with pytest.raises(NotImplementedError, match='geographic'):      # degrees by the reference's test: no x above 360
        small(x=100 + rng.random(7), y=60 + rng.random(7))
    geo = small(x=4 + rng.random(7), y=60 + rng.random(7), proj4=None, node_arrays=two_d, use_3d=True)[0]
    assert geo.use_3d is False and geo.geographic and geo.proj4 == '+proj=latlong'


def test_refusals_by_name():
    r, a = small()
    with pytest.raises(NotImplementedError, match='land_binary_mask'):
        small(node_arrays={'land_binary_mask': np.zeros(7)})
    with pytest.raises(NotImplementedError, match='ob_tran'):
        small(proj4='+proj=ob_tran +o_proj=longlat +lon_0=-40 +o_lat_p=22 +o_lon_p=0')
    with pytest.raises(NotImplementedError):
        small(proj4='+proj=robin')
    with pytest.raises(NotImplementedError, match='set_convolution_kernel'):
        r.set_convolution_kernel(3)
    with pytest.raises(NotImplementedError, match='ensemble'):
        small(node_arrays={SSH: [np.zeros((3, 7)), np.zeros((3, 7))]})
    with pytest.raises(NotImplementedError, match='129 vertical levels'):
        small(node_arrays={U_: np.zeros((3, 7, 129))}, zcor=np.zeros((3, 7, 129)))
    with pytest.raises(ValueError, match='three nearest'):
        small(x=a['x'][:2], y=a['y'][:2])
    few = np.full((3, 7, 3), np.nan, np.float32)
    few[:, 0, :2] = [-3.0, 0.0]
    with pytest.raises(ValueError, match='fewer than three finite'):
        small(zcor=few)
    with pytest.raises(ValueError, match='node coordinates'):
        small(y=np.zeros(6))
    with pytest.raises(ValueError, match='not finite'):
        small(x=np.r_[a['x'][:6], np.nan])
    with pytest.raises(ValueError, match='expected'):
        small(node_arrays={SSH: np.zeros((2, 7))})      # two time levels of three
    with pytest.raises(ValueError, match='zcor of shape'):
        small(zcor=np.zeros((3, 7, 4)))
    with pytest.raises(ValueError, match='disagree'):
        small(node_arrays={U_: np.zeros((3, 7, 3)), V_: np.zeros((3, 7, 4))})
    with pytest.raises(ValueError, match='times must increase'):
        small(times=[T0, T0, T0 + H])
    with pytest.raises(ValueError, match='Variable not available'):
        r.get_variables(['x_wind'], T0, [0.5], [0.5], [0.0])


def test_time_selection_follows_the_reference():
    r, a = small()
    assert r.nearest_time(T0 + timedelta(minutes=40))[1:3] == (T0, T0 + H) and r.nearest_time(T0 + timedelta(minutes=40))[4:] == (0, 1)
    assert r.time_weight(T0, [U_]) == (0, None, 0.0) and r.time_weight(T0 + H, [U_]) == (1, None, 0.0)
    assert r.time_weight(T0 + 2 * H, [U_]) == (2, None, 0.0)
    assert r.time_weight(T0 + timedelta(minutes=20), [U_, DEPTH]) == (0, 1, 1200.0 / 3600.0)
    assert r.time_weight(T0 + timedelta(minutes=90), [SSH]) == (1, 2, 0.5)
    assert r.time_weight(T0 + timedelta(minutes=90), [DEPTH]) == (1, None, 0.0)      # static variables alone: no blend
    one, _ = small(times=[T0], zcor=a['zcor'][:1], node_arrays={SSH: np.zeros((1, 7))})
    assert one.time_weight(T0, [SSH]) == (0, None, 0.0)
    assert not r.covers_time(T0 - H) and not r.covers_time(T0 + 3 * H) and r.covers_time(T0 + 2 * H)
    nan = r.get_variables([SSH], T0 + 3 * H, [a['x'].mean()], [a['y'].mean()], [0.0])
    assert np.isnan(nan[SSH]).all()
    # between two levels the value lies between the levels' values; at the level it is the level's
    xm, ym = [a['x'].mean()], [a['y'].mean()]
    v0, v1, vm = (r.get_variables([SSH], t, xm, ym, [0.0])[SSH][0] for t in (T0, T0 + H, T0 + timedelta(minutes=30)))
    assert v1 == v0 + 7 and abs(vm - (v0 + 3.5)) < 1e-5


def model(scheme='euler', **kw):
    o = OceanDrift(loglevel=50, **kw)
    r, a = small()
    o.add_reader(r)
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:advection_scheme', scheme)
    lon, lat = r.xy2lonlat(a['x'].mean(), a['y'].mean())
    o.seed_elements(lon=lon, lat=lat, time=T0, number=3)
    return o


@pytest.mark.parametrize('scheme', ['euler', 'runge-kutta4'])
def test_a_model_with_a_schism_reader_takes_the_call_by_call_lane(scheme, monkeypatch):
    monkeypatch.delenv('ODR_RUN_UNFUSED', raising=False)
    o = model(scheme)
    assert o._run_lane() == 'call_by_call'
    assert o._ctx is None      # answered without a device


def test_what_run_refuses():
    o = model()
    o._world, o._rank = 2, 1
    with pytest.raises(NotImplementedError, match='SchismReader .* sharded'):
        o.run(time_step=600, steps=2)
    assert o._ctx is None
    r, _ = small()
    with pytest.raises(NotImplementedError, match='operators on a SchismReader'):
        readers.check_device_expression(2 * r)
    with pytest.raises(NotImplementedError, match='operators on a SchismReader'):
        readers.check_device_expression(r + readers.ConstantReader({U_: 1.0, V_: 0.0}))
    k = {'ocean_vertical_diffusivity': np.full((3, 7, 3), 0.01), U_: np.zeros((3, 7, 3))}
    o = OceanDrift(loglevel=50)
    o.add_reader(small(node_arrays=k)[0])
    o.set_config('environment:constant:land_binary_mask', 0)
    o.set_config('drift:vertical_mixing', True)
    o.set_config('vertical_mixing:diffusivitymodel', 'environment')
    o.seed_elements(lon=14.0, lat=58.6, time=T0, number=3)
    with pytest.raises(NotImplementedError, match='ocean_vertical_diffusivity profiles'):
        o.run(time_step=600, steps=2)
    assert o._ctx is None


def test_abi_names():
    counts = {'odr_schism_create': 10, 'odr_schism_destroy': 2, 'odr_schism_set_zcor': 5, 'odr_schism_set_level': 7, 'odr_schism_sample': 9,
              'odr_schism_nearest3': 10, 'odr_schism_last_kernel_ms': 2}
    for name, n in counts.items():
        assert name in _abi.EXPORTS and len(_abi._SIGNATURES[name]) == n, name
    assert _abi.SCHISM_LEVELS == 4 and _abi.SCHISM_MAX_VERTICAL == 128
