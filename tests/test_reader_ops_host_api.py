"""CPU: the reader operators of opendrift_amd.readers -- grammar, names, variables, time coverage and the rejected expressions of the
reference's readers/operators/ (tests/golden/c38_reader_ops.npz part 3 lists what the reference itself rejects); the three known
answers of the reference's tests/readers/operators/test_numops.py; TimeseriesReader; the host evaluation against golden part 1 where
every leaf is a ContinuousReader; what the device program refuses; the ABI entries."""
from datetime import datetime, timedelta

import numpy as np
import pytest

import combine_host as H
from opendrift_amd import _abi, readers
from opendrift_amd.oceandrift import OceanDrift

T0 = H.T0
AT = dict(lon=np.array([5.]), lat=np.array([60.]))


def constants():
    return (readers.ConstantReader({'wind_speed': 5, 'wind_from_direction': 45, 'land_binary_mask': 0}),
            readers.ConstantReader({'wind_speed': 7, 'wind_from_direction': 30, 'land_binary_mask': 0}))


def test_known_answers_of_the_references_test_numops():
    r1, r2 = constants()
    r = r1 + 5
    assert r.variables == r1.variables
    assert r.get_variables_interpolated(variables=['wind_speed'], **AT)[0]['wind_speed'] == 10
    r = r1.filter_vars(['wind_speed']) + r2
    assert r.get_variables_interpolated(variables=['wind_speed'], **AT)[0]['wind_speed'] == [12]
    r = r1.exclude_vars(['wind_from_direction']) + r2
    with pytest.raises(AssertionError):
        r.get_variables_interpolated(variables=['wind_from_direction'], **AT)
    r = (r1.filter_vars(['wind_from_direction']) + r2) / 2
    assert r.get_variables_interpolated(variables=['wind_from_direction'], **AT)[0]['wind_from_direction'] == [75 / 2]
    assert r1.exclude_vars(['wind_from_direction']).variables == ['wind_speed', 'land_binary_mask']


def test_grammar_and_what_the_reference_rejects():
    g = np.load(H.GOLDEN)
    r1, r2 = constants()
    rejected = {'r1 - r2': lambda: r1 - r2, 'r1 + 2 * r2': lambda: r1 + 2 * r2, '2 * (3 * r1)': lambda: 2 * (3 * r1),
                '(2 * r1) + 1': lambda: (2 * r1) + 1}
    assert [str(n) for n in g['rejected']] == list(rejected) + ['variable outside the intersection: AssertionError']
    for make in rejected.values():
        with pytest.raises(TypeError):
            make()
    s = r1 + r2
    assert isinstance(s, readers.CombinedReader) and isinstance(s, readers.BaseReader) and isinstance((s + r1) + s, readers.CombinedReader)
    for n in (2 * r1, r1 * 2, r1 / 2, r1 - 3, 3 + r1, s / 2):
        assert isinstance(n, readers.NumCombinedReader) and not isinstance(n, readers.BaseReader)
    assert (r1 - 3).op == 'add' and (r1 - 3).n == -3 and (r1 / 2).op == 'div' and (0.9 * r1).op == 'mul'
    f = r1.filter_vars(['wind_speed'])
    assert isinstance(f, readers.FilteredReader) and not isinstance(f, readers.BaseReader) and isinstance(f + r2, readers.CombinedReader)
    assert isinstance(r2 + f, readers.CombinedReader)      # (Python falls back to the filter's __radd__, as with the reference's)
    with pytest.raises(AssertionError):
        r1.filter_vars(['x_wind'])
    with pytest.raises(AssertionError):
        2 * f      # numops.Combined asserts a BaseReader
    with pytest.raises(TypeError):
        r1 + 'wind'
    with pytest.raises(TypeError):
        r1 * r2


def test_names_variables_and_time_coverage():
    g = np.load(H.GOLDEN)
    a, b, c, d, ts = H.golden_readers(g)
    s = a + b
    assert s.name == str(g['name_a_plus_b']) == 'Combined(a | b)'
    assert s.variables == H.WIND + H.CURRENT and (a + d).variables == H.CURRENT and (a.filter_vars(H.WIND) + b).variables == H.WIND
    assert ((a + b) + c).name == 'Combined(Combined(a | b) | constant_reader)'
    assert s.device_kind == (2 * a).device_kind == a.filter_vars(H.WIND).device_kind == 'combined'
    late = readers.GridReader(g['a_x'], g['a_y'], [T0 + timedelta(hours=1), T0 + timedelta(hours=5)], {'x_wind': np.zeros((2, 5, 6), np.float32)}, name='late')
    m = a + late
    assert (m.start_time, m.end_time) == (T0 + timedelta(hours=1), T0 + timedelta(hours=2))      # the later start, the earlier end
    assert (c + a).start_time == a.start_time and (c + c).start_time is None and (c + c).end_time is None      # None: no limit
    assert m.covers_time(T0 + timedelta(hours=1.5)) and not m.covers_time(T0) and not m.covers_time(T0 + timedelta(hours=3))
    assert (2 * m).covers_time(T0 + timedelta(hours=2)) and not (2 * m).covers_time(T0)      # forwarded
    gb = a.combine_gaussian(ts[0], 1000.0)
    assert gb.name == 'Combined(a | reader_timeseries)' and gb.variables == H.WIND and gb.end_time == ts[0].end_time
    with pytest.raises(NotImplementedError, match='list of measurement readers'):
        a.combine_gaussian(ts, [1000.0, 2000.0])
    with pytest.raises(TypeError, match='TimeseriesReader'):
        a.combine_gaussian(c, 1000.0)
    with pytest.raises(ValueError, match='std'):
        a.combine_gaussian(ts[0], -1.0)


def test_timeseries_reader_takes_the_nearest_level():
    times = [T0 + timedelta(hours=k) for k in range(3)]
    r = readers.TimeseriesReader({'time': times, 'x_wind': [1., 2., 3.], 'y_wind': [4., 5., 6.], 'lon': 4.5, 'lat': 60.})
    assert r.variables == ['x_wind', 'y_wind'] and (r.lon, r.lat) == (4.5, 60.) and r.device_kind is None
    assert isinstance(r, readers.ContinuousReader) and (r.start_time, r.end_time, r.time_step) == (times[0], times[2], timedelta(hours=1))
    for minutes, want in ((0, 1.), (29, 1.), (30, 2.), (31, 2.), (60, 2.), (119, 3.), (120, 3.)):      # midway: the later level
        assert r.value('x_wind', T0 + timedelta(minutes=minutes)) == want, minutes
    out = r.get_variables(['x_wind', 'y_wind'], T0 + timedelta(minutes=95), np.zeros(3), np.zeros(3))
    assert list(out['x_wind']) == [3.] * 3 and list(out['y_wind']) == [6.] * 3
    env, _ = r.get_variables_interpolated(['x_wind'], time=T0 + timedelta(hours=3), lon=[4.], lat=[60.])
    assert np.isnan(env['x_wind']).all()      # outside its time coverage
    with pytest.raises(ValueError, match='same length'):
        readers.TimeseriesReader({'time': times, 'x_wind': [1., 2.]})
    with pytest.raises(ValueError, match='array of datetime'):
        readers.TimeseriesReader({'time': T0, 'x_wind': [1.]})


def test_host_evaluation_against_the_golden_where_every_leaf_is_continuous():
    """c + c, 2.5 * c and the Gaussian blend of the constant reader: the reference's own numbers are in the golden only for gridded
    operands, so the blend is checked against its definition over the golden's pyproj distances (Vincenty's distance on the host:
    within a millimetre, 1e-7 of the weight at these ranges)."""
    g = np.load(H.GOLDEN)
    a, b, c, d, ts = H.golden_readers(g)
    lon, lat = g['q_all_lon'], g['q_all_lat']
    t = T0 + timedelta(seconds=int(g['call_seconds']))
    env, prof = ((c + c) / 2).get_variables_interpolated(['x_wind'], time=t, lon=lon, lat=lat)
    assert prof is None and env['x_wind'].dtype == np.float64 and (env['x_wind'] == 10.0).all()
    blend = c.combine_gaussian(ts[1], float(g['std'][1]))
    env, _ = blend.get_variables_interpolated(H.WIND, time=t, lon=lon, lat=lat, z=g['q_z'])
    f = np.exp(-np.power(g['gauss_distance_all_1'] / float(g['std'][1]), 2.) / 2)
    for v, const in (('x_wind', 10.0), ('y_wind', 0.5)):
        b_value = float(g['ts1_' + v][1])      # 1200 s: nearest to the level at 1800 s
        assert np.allclose(env[v], const * (1 - f) + b_value * f, rtol=1e-6, atol=0)
    assert f.max() > 0.99 and f.min() < 1e-3
    with pytest.raises(NotImplementedError, match='device only'):
        (a + c).get_variables_interpolated(['x_wind'], time=t, lon=lon, lat=lat)
    assert np.abs(readers.wgs84_distance(lon, lat, 4.8, 60.2) - g['gauss_distance_all_1']).max() < 1e-3


def test_postfix_and_what_the_device_program_refuses():
    g = np.load(H.GOLDEN)
    a, b, c, d, ts = H.golden_readers(g)
    post = readers.expression_postfix(((a + b) + (c + a)) / 2)
    assert [k for k, _, _ in post] == [0, 0, 2, 0, 0, 2, 2, 7] and readers.expression_depth(post) == 3 and post[-1][2][0] == 2.0
    assert post[0][1] is a and post[4][1] is a
    post = readers.expression_postfix(a.filter_vars(H.WIND).combine_gaussian(ts[0], 500.0))
    assert [k for k, _, _ in post] == [0, 3, 4] and post[1][2] == (4.5, 60.0, 500.0) and post[1][1] is ts[0]
    assert [k for k, _, _ in readers.expression_postfix(ts[0] + a)] == [1, 0, 2]
    eight = a
    for r in (b, c, d, a, b, c, d):      # eight leaves, left-deep: two values at a time
        eight = eight + r
    assert readers.expression_depth(readers.check_device_expression(eight)) == 2

    class Mine(readers.ContinuousReader):
        name, variables = 'mine', H.WIND
    mesh = type('M', (readers.BaseReader,), dict(device_kind='umesh', name='mesh', variables=H.WIND))()
    shape = readers.ShapeReader([np.array([[0, 0], [1, 0], [1, 1.]])])
    members = readers.GridReader(g['a_x'], g['a_y'], [T0], {'x_wind': [np.zeros((1, 5, 6), np.float32)] * 2}, name='members')
    too_deep = a + (b + (c + (d + a)))
    for expr, reason in ((a + Mine(), 'evaluated on the host'), (2 * (a + mesh), 'mesh or shape'), (shape + shape, 'mesh or shape'),
                         (a + members, 'ensemble members'), (too_deep, 'deeper than the device program supports'),
                         (readers.ConstantReader({'x_wind': [1.0], 'element_ID': [0]}) + a, 'evaluated on the host')):
        with pytest.raises(NotImplementedError, match=reason):
            readers.check_device_expression(expr)
        o = OceanDrift(loglevel=50)
        o.add_reader(expr)
        with pytest.raises(NotImplementedError, match=reason):
            o._check_reader_expressions()


def test_run_refuses_profiles_sharded_runs_and_too_many_sources(monkeypatch):
    g = np.load(H.GOLDEN)
    a, b, c, d, ts = H.golden_readers(g)
    times = [T0, T0 + timedelta(hours=1)]
    k = readers.GridReader(g['d_x'], g['d_y'], times, {'ocean_vertical_diffusivity': np.zeros((2, 3, 5, 6), np.float32)}, z=g['d_z'], name='k')
    o = OceanDrift(loglevel=50)
    o.add_reader(k + k)
    o.set_config('drift:vertical_mixing', True)
    o.set_config('vertical_mixing:diffusivitymodel', 'environment')
    with pytest.raises(NotImplementedError, match='yields no vertical profiles'):
        o._check_reader_expressions()
    o.set_config('drift:vertical_mixing', False)
    o._check_reader_expressions()
    o = OceanDrift(loglevel=50)
    o.add_reader(a + b)
    o._world = 2
    with pytest.raises(NotImplementedError, match='sharded run'):
        o._check_reader_expressions()
    o = OceanDrift(loglevel=50)
    for n in range(9):      # 9 x 2 leaves
        o.add_reader(readers.ConstantReader({'x_wind': 1.0}) + readers.ConstantReader({'x_wind': 2.0}))
    with pytest.raises(NotImplementedError, match='18 device sources, a context holds 16'):
        o._check_reader_expressions()
    o = OceanDrift(loglevel=50)
    o.add_reader([c + a, a])
    assert o._unbound_off_list_readers() == ['Combined(constant_reader | a)'] and o._run_lane() == 'call_by_call'
    assert o.priority_list['x_wind'] == ['Combined(constant_reader | a)', 'a']


def test_abi_entries():
    for name, n in (('odr_combined_create', 4), ('odr_combined_destroy', 2), ('odr_combined_sample', 9), ('odr_combined_last_kernel_ms', 2)):
        assert name in _abi.EXPORTS and len(_abi._SIGNATURES[name]) == n, name
    assert _abi.NVAR == 26
    import ctypes as C
    assert C.sizeof(_abi.CombineOp) == 32
    assert (_abi.COMBINE_MAX_OPS, _abi.COMBINE_MAX_UNIFORM, _abi.COMBINE_MAX_VARIABLES, _abi.COMBINE_STACK) == (32, 8, 8, 3)
