"""CPU: OpenDriftSimulation.clone / calculate_ftle around the device call: the grid, the argument forms, the forward fill, the order of
the trajectories, the masks and the refusal -- against the reference's own calculate_ftle (tests/golden/c33_ftle.npz (b), written by
tools/gen_golden_ftle.py).  The device call is replaced by the host build of csrc/odr_ftle.hip.h (tests/ftle_host.py) behind the
signature of opendrift_amd.device.Context.ftle_map, the runs by the recorded [trajectory, time] arrays; tests/test_gpu_ftle.py runs
the whole on the device.  lon / lat bit for bit; the maps within ftle_host.ARITHMETIC_BOUND (4 x the 1.04e-07 measured on the
golden's CPU) with identical masks."""
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

import ftle_host as fh
from conftest import ROOT, golden
from opendrift_amd import _abi, projection
from opendrift_amd.oceandrift import OceanDrift, OpenDriftSimulation, last_valid
from opendrift_amd.leeway import Leeway
from opendrift_amd.readers import ConstantReader, DoubleGyreReader, OscillatingReader


class HostContext:
    """Stands in for the model's device context: ftle_map by the host build, every call recorded."""

    def __init__(self):
        self.calls = []

    def ftle_map(self, proj, xs, ys, delta, duration_seconds, lon, lat, displacement=False):
        self.calls.append(dict(proj=proj, xs=xs, ys=ys, delta=delta, duration_seconds=duration_seconds, lon=lon, lat=lat))
        X, Y = np.meshgrid(xs, ys)
        bx, by = projection.Proj.__call__(_Params(proj), lon.astype(np.float64).reshape(X.shape), lat.astype(np.float64).reshape(X.shape))
        return fh.ftle_map(bx - X, by - Y, delta, duration_seconds)


class _Params:
    def __init__(self, params):
        self.params = params


@pytest.fixture(scope='module')
def g():
    return golden('c33_ftle.npz')


def replay(g, monkeypatch, **kwargs):
    """calculate_ftle with the golden's arguments; the runs hand out the recorded arrays, in cell order in both directions"""
    times = [datetime.fromisoformat(str(t)) for t in g['b_times']]
    duration = float(g['b_duration'])
    o = OceanDrift(loglevel=50)
    o._ctx = HostContext()
    runs = []

    def trajectories(lon, lat, z, start, time_step, dur):
        backward = time_step.total_seconds() < 0
        i = times.index(start - dur if backward else start)
        runs.append((i, backward, lon, lat, z, dur, time_step))
        d = 'b' if backward else 'f'
        return g['b_hist_%s_lon' % d][i], g['b_hist_%s_lat' % d][i]
    monkeypatch.setattr(o, '_ftle_trajectories', trajectories)
    args = dict(reader=str(g['b_proj4']), delta=float(g['b_delta']), domain=list(g['b_domain']), time=list(times),
                time_step=float(g['b_time_step']), duration=duration)
    args.update(kwargs)
    return o, runs, o.calculate_ftle(**args)


def check_map(got, want, mask, duration):
    assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.ma.getmaskarray(got), mask)
    for i in range(want.shape[0]):
        m = fh.measure(got.data[i].astype(np.float32), want[i].astype(np.float32), duration)
        print('time %d: measure %.3g (bound %.3g)' % (i, m, fh.ARITHMETIC_BOUND))
        assert m <= fh.ARITHMETIC_BOUND


def test_entry_points_exist():
    assert callable(OpenDriftSimulation.calculate_ftle) and callable(OpenDriftSimulation.clone)
    assert 'odr_ftle_map' in _abi.EXPORTS and 'odr_ftle_last_kernel_ms' in _abi.EXPORTS
    header = open(os.path.join(ROOT, 'include', 'odrift.h')).read()
    assert 'int odr_ftle_map(' in header and 'physics_methods.py:458-484' in header


def test_golden_replay(g, monkeypatch):
    o, runs, lcs = replay(g, monkeypatch)
    assert lcs['lon'].dtype == np.float64 and np.array_equal(lcs['lon'].view(np.uint64), g['b_lon'].view(np.uint64))
    assert np.array_equal(lcs['lat'].view(np.uint64), g['b_lat'].view(np.uint64))
    assert lcs['time'] == [datetime.fromisoformat(str(t)) for t in g['b_times']]
    assert [(r[0], r[1]) for r in runs] == [(0, False), (0, True), (1, False), (1, True)]
    for r in runs:      # every run is seeded with the whole grid, row by row
        assert np.array_equal(r[2], g['b_lon'].ravel()) and np.array_equal(r[3], g['b_lat'].ravel()) and r[4] == 0
        assert r[5] == timedelta(seconds=float(g['b_duration']))
    assert (np.isnan(g['b_hist_f_lon'][0][:, -1])).mean() >= 0.05      # the forward fill is exercised
    duration = float(g['b_duration'])
    check_map(lcs['RLCS'], g['b_RLCS'], g['b_RLCS_mask'], duration)
    check_map(lcs['ALCS'], g['b_ALCS'], g['b_ALCS_mask'], duration)
    for c in o.ctx.calls:
        assert c['proj'] == dict(kind='latlong') and c['duration_seconds'] == duration and c['lon'].dtype == np.float32


def test_backward_rows_are_not_flipped(g, monkeypatch):
    """the reference's [::-1] belongs to ITS backward runs: flipping the rows here gives another map"""
    o, runs, lcs = replay(g, monkeypatch)
    i = 0
    lon, lat = last_valid(g['b_hist_b_lon'][i])[::-1], last_valid(g['b_hist_b_lat'][i])[::-1]
    flipped = HostContext().ftle_map(dict(kind='latlong'), o.ctx.calls[0]['xs'], o.ctx.calls[0]['ys'], float(g['b_delta']),
                                     float(g['b_duration']), lon, lat)
    assert not np.allclose(flipped, g['b_ALCS'][i], atol=1e-5)


def test_maps_not_asked_for_stay_zero(g, monkeypatch):
    o, runs, lcs = replay(g, monkeypatch, ALCS=False)
    assert [r[1] for r in runs] == [False, False]
    assert not lcs['ALCS'].any() and not np.ma.getmaskarray(lcs['ALCS']).any() and lcs['ALCS'].shape == g['b_ALCS'].shape
    check_map(lcs['RLCS'], g['b_RLCS'], g['b_RLCS_mask'], float(g['b_duration']))
    o, runs, lcs = replay(g, monkeypatch, RLCS=False)
    assert [r[1] for r in runs] == [True, True] and not lcs['RLCS'].any()


def test_argument_forms(g, monkeypatch):
    base = replay(g, monkeypatch)[2]
    t0 = datetime.fromisoformat(str(g['b_times'][0]))
    for kwargs in (dict(duration=timedelta(seconds=float(g['b_duration']))), dict(reader=projection.Proj('+proj=latlong')),
                   dict(time_step=timedelta(seconds=600))):
        lcs = replay(g, monkeypatch, **kwargs)[2]
        assert np.array_equal(lcs['RLCS'].data, base['RLCS'].data) and np.array_equal(lcs['ALCS'].data, base['ALCS'].data)
    o, runs, lcs = replay(g, monkeypatch, time=t0)      # a scalar time
    assert lcs['time'] == [t0] and lcs['RLCS'].shape == (1, ) + g['b_lon'].shape
    assert np.array_equal(lcs['RLCS'].data[0], base['RLCS'].data[0])
    assert runs[1][6] == timedelta(seconds=-600) and runs[0][6] == timedelta(seconds=600)


def test_reader_object_and_default_reader(monkeypatch):
    """reader=None: the first reader, its bounds and its start time; a reader object: its projection and bounds"""
    r = DoubleGyreReader(initial_time=datetime(2000, 1, 1), epsilon=.25, A=.1)
    for reader in (None, r):
        o = OceanDrift(loglevel=50)
        o.add_reader(r)
        o.add_reader(ConstantReader({'x_wind': 1.0, 'y_wind': 0.0}))
        o._ctx = HostContext()
        starts = []

        def trajectories(lon, lat, z, start, time_step, dur):
            starts.append(start)
            return np.float32(lon)[:, None] + np.zeros((1, 2), np.float32), np.float32(lat)[:, None] + np.zeros((1, 2), np.float32)
        monkeypatch.setattr(o, '_ftle_trajectories', trajectories)
        lcs = o.calculate_ftle(reader=reader, delta=.25, time=r.initial_time, time_step=0.5, duration=15)
        xs, ys = np.arange(0., 2., .25), np.arange(0., 1., .25)
        assert lcs['lon'].shape == (len(ys), len(xs)) == (4, 8)
        assert np.array_equal(o.ctx.calls[0]['xs'], xs) and np.array_equal(o.ctx.calls[0]['ys'], ys)
        assert o.ctx.calls[0]['proj'] == r.proj.params and o.ctx.calls[0]['proj']['kind'] == 'stere_equit_sphere'
        want_lon, want_lat = r.proj(*np.meshgrid(xs, ys), inverse=True)
        assert np.array_equal(lcs['lon'], want_lon) and np.array_equal(lcs['lat'], want_lat)
        assert lcs['time'] == [r.initial_time] and starts == [r.initial_time, r.initial_time + timedelta(seconds=15)]
    o = OceanDrift(loglevel=50)
    o._ctx = HostContext()
    with pytest.raises(ValueError):
        o.calculate_ftle(delta=.25, duration=15, time=datetime(2000, 1, 1))      # no reader at all
    with pytest.raises(ValueError, match='domain'):
        o.calculate_ftle(reader='+proj=latlong', delta=.25, duration=15, time=datetime(2000, 1, 1))      # a projection has no bounds


def test_last_valid_is_the_forward_fill():
    a = np.array([[1, 2, 3], [4, np.nan, np.nan], [np.nan, 5, np.nan], [np.nan, np.nan, np.nan], [6, np.nan, 7]], np.float32)
    out = last_valid(a)
    assert out.dtype == np.float32 and np.array_equal(out, np.array([3, 4, 5, np.nan, 7], np.float32), equal_nan=True)
    assert np.isnan(a[1, 2])      # the input is left as it is
    lon, lat = np.array([[1, np.nan]], np.float32), np.array([[2, 3]], np.float32)      # each variable on its own
    assert last_valid(lon)[0] == 1 and last_valid(lat)[0] == 3


def test_clone_keeps_class_config_and_readers(objectprop_path):
    r1 = DoubleGyreReader()
    r2 = ConstantReader({'x_wind': 3.0, 'y_wind': 1.0})
    r3 = OscillatingReader('x_wind', amplitude=5)
    r4 = ConstantReader({'x_wind': -1.0, 'y_wind': 0.0})      # a second reader of the same name
    o = OceanDrift(loglevel=50, seed=7, rng='numpy')
    o.add_reader([r1, r2])
    o.add_reader(r3, first=True)
    o.add_reader(r4, variables=['x_wind'])
    o.set_config('drift:advection_scheme', 'runge-kutta4')
    o.set_config('drift:max_speed', 3.5)
    o.set_config('environment:constant:y_wind', 2.0)
    o.set_config('seed:ocean_only', True)
    c = o.clone()
    assert type(c) is OceanDrift and c is not o and c.mode == 'Config'
    assert (c._seed, c.rng, c.stage_math, c._device) == (o._seed, o.rng, o.stage_math, o._device)
    assert list(c._config) == list(o._config)
    for k in o._config:
        assert c.get_config(k) == o.get_config(k) or (c.get_config(k) is None and o.get_config(k) is None), k
        assert c._config[k] is not o._config[k]
    assert list(c._readers_host) == list(o._readers_host) == ['double_gyre', 'constant_reader', 'oscillating_reader', 'constant_reader_2']
    for name in o._readers_host:
        assert c._readers_host[name][0] is o._readers_host[name][0] and c._readers_host[name][1] == o._readers_host[name][1]
    assert c.priority_list == o.priority_list and c.priority_list['x_wind'] == ['oscillating_reader', 'constant_reader', 'constant_reader_2']
    assert all(c.priority_list[v] is not o.priority_list[v] for v in o.priority_list)
    c.set_config('drift:max_speed', 1.0)      # the clone's config is its own
    assert o.get_config('drift:max_speed') == 3.5
    lw = Leeway(d=objectprop_path, loglevel=50)
    lw.set_config('seed:object_type', list(lw.leewayprop.values())[1]['Description'])
    c = lw.clone()
    assert type(c) is Leeway and c.get_config('seed:object_type') == lw.get_config('seed:object_type')
    assert c.leewayprop == lw.leewayprop


def test_sharded_run_is_refused():
    o = OceanDrift(loglevel=50)
    o._ctx = HostContext()
    o.add_reader(DoubleGyreReader())
    o._world, o._rank = 2, 1
    with pytest.raises(NotImplementedError, match='sharded'):
        o.calculate_ftle(delta=.25, time_step=0.5, duration=15)
    assert o.ctx.calls == []
