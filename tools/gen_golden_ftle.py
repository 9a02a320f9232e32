"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c33_ftle.npz from the REFERENCE ITSELF.

(a) The reference's own physics_methods.ftle (opendrift/models/physics_methods.py:458-484), imported through oracle/refshim.py, on
    recorded float64 displacement fields [ny, nx] with delta = 0.02:
      sheared     23 x 37 (ny x nx), a sheared and stretched field with a sinusoidal part, T = 15
      block       the same with a 5 x 4 (columns x rows) block of identical displacement: lambda = 0, -inf in the cells whose stencil
                  lies inside the block
      small22     2 x 2
      small29     2 x 9 (ny x nx)
      negative    `sheared` with duration = -15
(b) The reference's own OpenDriftSimulation.calculate_ftle (opendrift/models/basemodel/__init__.py:4844-4923) called UNBOUND on a
    stand-in `self` whose clone() returns stubs: seed_elements records what it is given, run does nothing, and
    result.lon.ffill(dim='time') forward-fills recorded float32 [trajectory, time] arrays that have trailing NaNs (elements
    deactivated before the end) and hands the result back as an object with .T, [...] and .values, the part of xarray's DataArray the
    method uses.  The stub of the backward direction holds its rows in the reference's ID order of a backward run (flipped,
    :2061-2063), which the method undoes with [::-1] (:4913); the file stores the arrays in CELL order -- trajectory k is cell k,
    the order of this project's runs in both directions.  reader = '+proj=latlong' (a proj4 string: the shim's Proj, whose
    latlong transform is the identity on both sides, so lon / lat are comparable bit for bit), domain = [3, 6.1, 59, 61],
    delta = 0.1 (31 x 20 cells), time = a list of two, duration = 3600 s.  This pins the grid, the inverse projection call, the
    forward fill, the re-ordering of the backward run and the masking.

Conditions asserted here so that the golden cannot hide a failure:
  nx != ny in every case but small22; every edge and every corner of the sheared cases has a finite value; the share of
  non-finite reference cells in the sheared cases is 0; the block case has -inf cells and no NaN; at least 5 % of the trajectories
  of (b) end in NaN columns; the file is under 1 MiB.

Also prints the error measure of the host build of csrc/odr_ftle.hip.h against (a) -- the number tests/ftle_host.py records.

    python tools/gen_golden_ftle.py
"""
import os
import sys
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from opendrift.models.basemodel import OpenDriftSimulation  # noqa: E402
from opendrift.models.physics_methods import ftle  # noqa: E402

DELTA, T = 0.02, 15.0


def sheared(ny, nx, seed):
    """displacement of a sheared, stretched and gently folded map of a DELTA grid"""
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid(np.arange(nx) * DELTA, np.arange(ny) * DELTA)
    dX = 0.8 * X + 1.7 * Y + 0.05 * np.sin(9 * X + 4 * Y) + rng.normal(0, 1e-4, X.shape)
    dY = -0.3 * X + 0.4 * Y + 0.04 * np.cos(7 * X - 5 * Y) + rng.normal(0, 1e-4, X.shape)
    return np.ascontiguousarray(dX), np.ascontiguousarray(dY)


class _Arr:
    """.T, [...] and .values of xarray's DataArray"""
    def __init__(self, a):
        self.values = a

    @property
    def T(self):
        return _Arr(self.values.T)

    def __getitem__(self, k):
        return _Arr(self.values[k])


class _Var:
    def __init__(self, a):
        self._a = a

    def ffill(self, dim):
        assert dim == 'time'
        a = self._a
        idx = np.where(np.isnan(a), 0, np.arange(a.shape[1])[None, :])
        idx = np.maximum.accumulate(idx, axis=1)
        return _Arr(np.take_along_axis(a, idx, axis=1))


class _Result:
    def __init__(self, lon, lat):
        self.lon, self.lat = _Var(lon), _Var(lat)


class _Stub:
    def __init__(self, parent):
        self.parent = parent

    def seed_elements(self, lon, lat, time, z):
        self.seeded = dict(lon=np.array(lon), lat=np.array(lat), time=time, z=z)

    def run(self, duration, time_step):
        p = self.parent
        backward = time_step < 0
        i = p.times.index(self.seeded['time'] - duration if backward else self.seeded['time'])
        assert np.array_equal(self.seeded['lon'], p.lons.ravel()) and np.array_equal(self.seeded['lat'], p.lats.ravel())
        lon, lat = p.hist['b_lon' if backward else 'f_lon'][i], p.hist['b_lat' if backward else 'f_lat'][i]
        if backward:      # the reference's backward run holds element N - 1 - k in row k
            lon, lat = lon[::-1], lat[::-1]
        self.result = _Result(lon, lat)
        p.runs.append((i, backward, duration, time_step))


class _StandIn:
    def __init__(self, times, hist, lons, lats):
        self.times, self.hist, self.lons, self.lats, self.runs = times, hist, lons, lats, []

    def clone(self):
        return _Stub(self)


def histories(rng, lons, lats, sign):
    """float32 [trajectory, time] positions of a swirl around the middle of the grid; a tenth of the trajectories end early"""
    n, nt = lons.size, 5
    lo0, la0 = lons.ravel(), lats.ravel()
    cx, cy = lo0.mean(), la0.mean()
    lon, lat = np.empty((n, nt)), np.empty((n, nt))
    for k in range(nt):
        s = sign * k / (nt - 1)
        ang = s * 0.9 * np.exp(-((lo0 - cx) ** 2 / 1.2 + (la0 - cy) ** 2 / 0.4))
        lon[:, k] = cx + (lo0 - cx) * np.cos(ang) - 2 * (la0 - cy) * np.sin(ang) + 0.15 * s
        lat[:, k] = cy + 0.5 * (lo0 - cx) * np.sin(ang) + (la0 - cy) * np.cos(ang) + 0.05 * s * np.sin(3 * lo0)
    early = rng.uniform(size=n) < 0.1
    last = np.where(early, rng.integers(0, nt - 1, n), nt - 1)      # index of the last valid time
    dead = np.arange(nt)[None, :] > last[:, None]
    lon[dead] = np.nan
    lat[dead] = np.nan
    return np.ascontiguousarray(lon, np.float32), np.ascontiguousarray(lat, np.float32)


def main():
    import ftle_host as fh
    data, worst = {}, 0.0
    # ---- (a)
    dX, dY = sheared(23, 37, 33)
    bX, bY = dX.copy(), dY.copy()
    bX[8:12, 10:15] = bX[9, 12]
    bY[8:12, 10:15] = bY[9, 12]
    cases = {'sheared': (dX, dY, T), 'block': (bX, bY, T), 'small22': sheared(2, 2, 34) + (T, ), 'small29': sheared(2, 9, 35) + (T, ),
             'negative': (dX, dY, -T)}
    for name, (x, y, dur) in cases.items():
        with np.errstate(divide='ignore'):
            ref = ftle(x, y, DELTA, dur)
        assert ref.dtype == np.float32 and ref.shape == x.shape
        ny, nx = x.shape
        assert nx != ny or name == 'small22'
        if name in ('sheared', 'negative'):
            assert np.isfinite(ref).all(), name
        if name == 'block':
            assert np.isneginf(ref).sum() == 3 * 2 and not np.isnan(ref).any() and np.isfinite(ref).sum() == ref.size - 6
            assert np.isneginf(ref[9:11, 11:14]).all()
        for edge in (ref[0], ref[-1], ref[:, 0], ref[:, -1], ref[[0, 0, -1, -1], [0, -1, 0, -1]]):
            assert np.isfinite(edge).all(), name
        data.update({'a_%s_dX' % name: x, 'a_%s_dY' % name: y, 'a_%s_duration' % name: dur, 'a_%s_ftle' % name: ref})
        m = fh.measure(fh.ftle_map(x, y, DELTA, dur), ref, dur)
        worst = max(worst, m)
        print('(a) %-9s %2d x %2d  reference min %.4g max %.4g  -inf %d | host build vs reference %.3g'
              % (name, ny, nx, ref[np.isfinite(ref)].min(), ref[np.isfinite(ref)].max(), np.isneginf(ref).sum(), m))
    data['a_delta'] = DELTA
    # ---- (b)
    proj4, domain, delta, duration = '+proj=latlong', [3.0, 6.1, 59.0, 61.0], 0.1, 3600.0
    times = [datetime(2024, 3, 1, 12), datetime(2024, 3, 1, 18)]
    xs, ys = np.arange(domain[0], domain[1], delta), np.arange(domain[2], domain[3], delta)
    X, Y = np.meshgrid(xs, ys)
    assert len(xs) != len(ys)
    rng = np.random.default_rng(36)
    hist = {k: [] for k in ('f_lon', 'f_lat', 'b_lon', 'b_lat')}
    for i in range(len(times)):
        for d, sign in (('f', 1.0 + 0.3 * i), ('b', -1.0 - 0.3 * i)):
            lo, la = histories(rng, X, Y, sign)
            assert np.isnan(lo[:, -1]).mean() >= 0.05 and not np.isnan(lo[:, 0]).any()
            hist[d + '_lon'].append(lo)
            hist[d + '_lat'].append(la)
    o = _StandIn(times, hist, X, Y)
    lcs = OpenDriftSimulation.calculate_ftle(o, reader=proj4, delta=delta, domain=domain, time=list(times), time_step=600,
                                            duration=duration)
    assert [r[:2] for r in o.runs] == [(0, False), (0, True), (1, False), (1, True)]
    assert np.array_equal(lcs['lon'], X) and np.array_equal(lcs['lat'], Y)
    for k in ('RLCS', 'ALCS'):
        assert lcs[k].shape == (2, len(ys), len(xs)) and lcs[k].dtype == np.float64
        assert not np.ma.getmaskarray(lcs[k]).any(), k
    assert not np.array_equal(lcs['RLCS'].data, lcs['ALCS'].data)
    for i in range(2):      # (the host build on what the reference differentiated, for the printed measure only)
        for d, key in (('f', 'RLCS'), ('b', 'ALCS')):
            lo = _Var(hist[d + '_lon'][i]).ffill('time').values[:, -1].reshape(X.shape)
            la = _Var(hist[d + '_lat'][i]).ffill('time').values[:, -1].reshape(X.shape)
            m = fh.measure(fh.ftle_map(lo - X, la - Y, delta, duration), lcs[key].data[i].astype(np.float32), duration)
            worst = max(worst, m)
            print('(b) time %d %s  host build vs reference %.3g' % (i, key, m))
    data.update(b_proj4=proj4, b_domain=np.array(domain), b_delta=delta, b_duration=duration, b_time_step=600.0,
                b_times=np.array([t.isoformat() for t in times]), b_lon=lcs['lon'], b_lat=lcs['lat'],
                b_RLCS=lcs['RLCS'].data, b_ALCS=lcs['ALCS'].data, b_RLCS_mask=np.ma.getmaskarray(lcs['RLCS']),
                b_ALCS_mask=np.ma.getmaskarray(lcs['ALCS']), **{'b_hist_' + k: np.stack(v) for k, v in hist.items()})
    path = os.path.join(ROOT, 'tests', 'golden', 'c33_ftle.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes; largest measure of the host build against the reference: %.3g' % worst)
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
