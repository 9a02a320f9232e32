"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c34_trajectory_lengths.npz from the REFERENCE ITSELF.

The reference's own OpenDriftSimulation.get_trajectory_lengths (opendrift/models/basemodel/__init__.py:4614-4628), imported through
oracle/refshim.py, is called UNBOUND on a stand-in `self`: a `result` whose lon / lat are [trajectory, time] float32 arrays (what the
reference's xarray Dataset hands out and what run() returns here), a `time_step_output` and the mode the decorator asks for.
pyproj.Geod.inv is the shim's (given back the shape of its arguments, as pyproj's has): the oracle's shooting inverse, which agrees
with its own direct solve to 4.7e-9 m on lines up to 5000 km between +-85 degrees.

300 trajectories, 12 output times, dt = 3600 s; a second case with dt = -3600 s (a backward run: negative speeds, nothing is cut).
  slow   drifters at 0.03 mm/s .. 0.25 m/s: intervals of 0.1 .. 900 m
  fast   3 .. 80 m/s: intervals of 10 .. 290 km
  jumps  one interval in eight of both is 400 .. 1500 km instead: faster than 100 m/s, cut to 0 in the forward case
  seam   trajectories that start just west of the +-180 seam and drift east across it (longitudes wrapped to [-180, 180])
  still  trajectories that stop (stranded): coincident pairs
  late seeding (NaN heads) and deactivation (NaN tails)

Conditions asserted here so that the golden cannot hide a failure:
  (a) NaN heads and NaN tails exist;
  (b) at least 10 % of the intervals are under 1 km, at least 10 % between 10 and 300 km, at least 5 % faster than 100 m/s and cut;
  (c) at least 5 intervals cross the seam, at least 5 are coincident pairs;
  (d) |lat| <= 85, uncut intervals of the forward case <= 360 km, all intervals <= 5000 km;
  (e) no speed within 1e-6 of 100 m/s before the cut; the cut and the NaN intervals are exactly 0;
  (f) the file is under 1 MiB.

    python tools/gen_golden_trajectory_lengths.py
"""
import os
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from opendrift.models.basemodel import Mode, OpenDriftSimulation  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import opendrift.models.basemodel as _basemodel  # noqa: E402

NTRAJ, NT, DT = 300, 12, 3600.0


class _ShapedGeod(refshim.Geod):
    """the shim's inv returns flat arrays; pyproj's keep the shape of their arguments, which the reference indexes ([-1, :])"""
    def inv(self, lons1, lats1, lons2, lats2, **kw):
        shape = np.shape(lons1)
        return tuple(np.reshape(v, shape) for v in refshim.Geod.inv(self, lons1, lats1, lons2, lats2, **kw))


_basemodel.pyproj.Geod = _ShapedGeod


class _Result:
    def __init__(self, lon, lat):
        self.lon, self.lat = lon, lat


class _StandIn:
    def __init__(self, lon, lat, dt):
        self.result = _Result(lon, lat)
        self.time_step_output = timedelta(seconds=dt)
        self.mode = Mode.Result


def population(seed):
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, NTRAJ, p=[0.4, 0.35, 0.1, 0.15])      # slow, fast, seam, still
    lon = np.empty((NTRAJ, NT))
    lat = np.empty((NTRAJ, NT))
    lon[:, 0] = rng.uniform(-170, 170, NTRAJ)
    lat[:, 0] = rng.uniform(-50, 50, NTRAJ)
    lon[kind == 2, 0] = rng.uniform(179.2, 179.98, (kind == 2).sum())
    stop_at = rng.integers(2, NT - 2, NTRAJ)
    for t in range(NT - 1):
        step = np.where(kind == 1, rng.uniform(10e3, 290e3, NTRAJ), 10 ** rng.uniform(-1, 2.95, NTRAJ))
        az = rng.uniform(0, 2 * np.pi, NTRAJ)
        az[kind == 2] = rng.uniform(np.radians(70), np.radians(110), (kind == 2).sum())
        step[kind == 2] = rng.uniform(5e3, 60e3, (kind == 2).sum())
        jump = (rng.uniform(size=NTRAJ) < 0.12) & (kind < 2)
        step[jump] = rng.uniform(400e3, 1500e3, jump.sum())
        step[(kind == 3) & (t >= stop_at)] = 0.0
        lat[:, t + 1] = lat[:, t] + step * np.cos(az) / 111.2e3
        lon[:, t + 1] = lon[:, t] + step * np.sin(az) / (111.2e3 * np.cos(np.radians(lat[:, t])))
    lon = (lon + 180.0) % 360.0 - 180.0
    steps = np.arange(NT)[None, :]
    seeded = np.where(rng.uniform(size=NTRAJ) < 0.3, rng.integers(1, 4, NTRAJ), 0)
    ended = np.where(rng.uniform(size=NTRAJ) < 0.3, rng.integers(NT - 4, NT, NTRAJ), NT)
    gone = (steps < seeded[:, None]) | (steps >= ended[:, None])
    lon[gone] = np.nan
    lat[gone] = np.nan
    return np.ascontiguousarray(lon, np.float32), np.ascontiguousarray(lat, np.float32)


def check(lon, lat, total, dist, speed):
    bad = []
    if not np.isnan(lon[:, 0]).any() or not np.isnan(lon[:, -1]).any():
        bad.append('(a)')
    lo, la = lon.T.astype(np.float64), lat.T.astype(np.float64)
    raw = orc.geod_inv(lo[:-1].ravel(), la[:-1].ravel(), lo[1:].ravel(), la[1:].ravel())[1].reshape(NT - 1, NTRAJ)
    finite = np.isfinite(raw)
    n = raw.size
    cut = finite & (raw / DT > 100)
    share = dict(short=(finite & (raw < 1e3)).sum() / n, mid=(finite & (raw >= 10e3) & (raw <= 300e3)).sum() / n, cut=cut.sum() / n)
    if share['short'] < 0.1 or share['mid'] < 0.1 or share['cut'] < 0.05:
        bad.append('(b) %s' % share)
    seam = (finite & (np.abs(lo[1:] - lo[:-1]) > 180)).sum()
    same = (finite & (lo[1:] == lo[:-1]) & (la[1:] == la[:-1])).sum()
    if seam < 5 or same < 5:
        bad.append('(c) %d seam %d coincident' % (seam, same))
    if np.nanmax(np.abs(lat)) > 85 or raw[finite & ~cut].max() > 360e3 or raw[finite].max() > 5000e3:
        bad.append('(d) lat %.2f uncut %.0f all %.0f' % (np.nanmax(np.abs(lat)), raw[finite & ~cut].max(), raw[finite].max()))
    if np.abs(raw[finite] / DT - 100).min() < 1e-6 or dist[cut | ~finite].any() or speed[cut | ~finite].any() \
            or not np.array_equal(dist[finite & ~cut], raw[finite & ~cut]):
        bad.append('(e)')
    print('%d intervals: %s, %d NaN, %d across the seam, %d coincident, longest uncut %.1f km, longest %.1f km'
          % (n, ' '.join('%s %.3f' % kv for kv in share.items()), (~finite).sum(), seam, same, raw[finite & ~cut].max() / 1e3,
             raw[finite].max() / 1e3))
    return bad


def main():
    for seed in range(34, 60):
        lon, lat = population(seed)
        total, dist, speed = OpenDriftSimulation.get_trajectory_lengths(_StandIn(lon, lat, DT))
        bad = check(lon, lat, total, dist, speed)
        print('seed %d: %s' % (seed, bad or 'all conditions hold'))
        if not bad:
            break
    else:
        raise AssertionError('no seed satisfies the conditions')
    btotal, bdist, bspeed = OpenDriftSimulation.get_trajectory_lengths(_StandIn(lon, lat, -DT))
    assert (bspeed <= 0).all() and bdist.max() > 360e3
    data = dict(lon=lon, lat=lat, dt=DT, seed=seed, total_length=total, distances=dist, speeds=speed, back_total_length=btotal,
                back_distances=bdist, back_speeds=bspeed)
    for k in ('total_length', 'distances', 'speeds', 'back_total_length', 'back_distances', 'back_speeds'):
        assert data[k].dtype == np.float64, k
    assert dist.shape == (NT - 1, NTRAJ) and total.shape == (NTRAJ, )
    path = os.path.join(ROOT, 'tests', 'golden', 'c34_trajectory_lengths.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
