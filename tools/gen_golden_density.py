"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c32_density.npz from the REFERENCE ITSELF.

The reference's own OpenDriftSimulation.get_density_array and get_residence_time (opendrift/models/basemodel/__init__.py:4091-4146,
:4247-4251), imported through oracle/refshim.py, are called UNBOUND on a stand-in `self`: a `result` whose entries have `.values`
([trajectory, time] float32 arrays, what the reference's xarray Dataset hands out and what run() returns here), a `time` of the right
length and a `status_categories`.  np.histogram2d does the binning, as it does in the reference.

300 trajectories, 6 output times, pixelsize_m = 400.  A plume: a narrow core around 4.9 E 60.1 N inside a wider cloud.  A fifth of the
entries are NaN in every variable (elements released late), about 40 % are at the surface (z = 0, some of them z = -0.0), about 10 %
are stranded (status 2, z = 0), the rest is submerged; a few entries have a NaN z at a finite position.

Cases (all on the same lon / lat / z / status):
  counts      status_categories = ['active', 'missing_data', 'stranded']: H, H_submerged, H_stranded
  nostranded  status_categories = ['active', 'missing_data']: H_stranded stays zero
  wint        weight = float32 values that are small integers (any order of summation gives the same float64 sum)
  wreal       weight = real-valued float32
  single      the fourth output time alone (edges of its own)
and get_residence_time on the counts case.  Stored: the inputs, every output, pixelsize_m, and the float32 cosine of the mid
latitude that the reference's deltalon divides by, with the float32 mid latitude itself (np.cos of a float32 differs in the last
bit between CPUs; tests/test_density_host_api.py).

Conditions asserted here so that the golden cannot hide a failure (the seed is re-drawn until they hold):
  (a) at least 10 % of the entries are in each of surface, submerged, stranded and NaN;
  (b) some z is -0.0, and some entry has a NaN z at a finite position;
  (c) len(lon_array) != len(lat_array) (a transposition cannot pass), and at least 20 bins each way;
  (d) some bin of H holds at least 3;
  (e) the file is under 1 MiB.

    python tools/gen_golden_density.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from opendrift.models.basemodel import OpenDriftSimulation  # noqa: E402

NTRAJ, NT, PIXELSIZE_M = 300, 6, 400.0
CATEGORIES = ['active', 'missing_data', 'stranded']
STRANDED = CATEGORIES.index('stranded')


class _Var:
    def __init__(self, values):
        self.values = values


class _Result(dict):
    """result.lon.values and result['mass'].values"""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


class _StandIn:
    def __init__(self, arrays, categories):
        nt = next(iter(arrays.values())).shape[1]
        self.result = _Result({k: _Var(v) for k, v in arrays.items()})
        self.result['time'] = list(range(nt))
        self.status_categories = list(categories)

    def get_density_array(self, pixelsize_m, weight=None):      # get_residence_time calls it on self
        return OpenDriftSimulation.get_density_array(self, pixelsize_m, weight=weight)


def population(seed):
    rng = np.random.default_rng(seed)
    shape = (NTRAJ, NT)
    core = rng.uniform(size=NTRAJ) < 0.5
    lon0 = np.where(core, rng.normal(4.9, 0.012, NTRAJ), rng.normal(4.9, 0.06, NTRAJ))
    lat0 = np.where(core, rng.normal(60.1, 0.006, NTRAJ), rng.normal(60.1, 0.03, NTRAJ))
    steps = np.arange(NT)[None, :]
    lon = lon0[:, None] + 0.004 * steps + rng.normal(0, 0.002, shape)
    lat = lat0[:, None] + 0.002 * steps + rng.normal(0, 0.001, shape)
    z = -rng.uniform(0.1, 30.0, shape)
    surface = rng.uniform(size=shape) < 0.4
    z[surface] = 0.0
    z[surface & (rng.uniform(size=shape) < 0.2)] = -0.0
    status = np.zeros(shape)
    strand_at = np.where(rng.uniform(size=NTRAJ) < 0.28, rng.integers(1, NT, NTRAJ), NT)      # stranded from that time on
    stranded = steps >= strand_at[:, None]
    status[stranded] = STRANDED
    z[stranded] = 0.0
    release = np.where(rng.uniform(size=NTRAJ) < 0.5, rng.integers(1, NT - 1, NTRAJ), 0)      # NaN before the release
    late = steps < release[:, None]
    odd = (rng.uniform(size=shape) < 0.01) & ~late & ~stranded      # a NaN z at a finite position
    z[odd] = np.nan
    wint = rng.integers(1, 10, shape).astype(np.float64)
    wreal = rng.uniform(0.05, 3.0, shape) * 10.0 ** rng.integers(-3, 4, shape)
    out = dict(lon=lon, lat=lat, z=z, status=status, mass_int=wint, mass=wreal)
    for v in out.values():
        v[late] = np.nan
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


def check(pop, H, Hsub, Hstr, lon_array, lat_array):
    bad = []
    z, status, lon = pop['z'], pop['status'], pop['lon']
    n = z.size
    share = dict(nan=np.isnan(lon).mean(), stranded=(status == STRANDED).mean(),
                 surface=(np.isfinite(lon) & (z >= 0) & (status != STRANDED)).mean(), submerged=(z < 0).mean())
    for k, v in share.items():
        if v < 0.1:
            bad.append('(a) %s %.3f' % (k, v))
    if not (np.signbit(z) & (z == 0)).any() or not (np.isnan(z) & np.isfinite(lon)).any():
        bad.append('(b)')
    if len(lon_array) == len(lat_array) or min(len(lon_array), len(lat_array)) < 21:
        bad.append('(c) %d x %d edges' % (len(lon_array), len(lat_array)))
    if H.max() < 3:
        bad.append('(d) %g' % H.max())
    print('%d entries: %s | %d x %d bins | sums %d surface %d submerged %d stranded | largest bin %d'
          % (n, ' '.join('%s %.3f' % kv for kv in share.items()), len(lon_array) - 1, len(lat_array) - 1, H.sum(), Hsub.sum(), Hstr.sum(),
             H.max()))
    return bad


def main():
    for seed in range(32, 52):
        pop = population(seed)
        core = {k: pop[k] for k in ('lon', 'lat', 'z', 'status')}
        o = _StandIn(pop, CATEGORIES)
        H, Hsub, Hstr, lon_array, lat_array = OpenDriftSimulation.get_density_array(o, PIXELSIZE_M)
        bad = check(pop, H, Hsub, Hstr, lon_array, lat_array)
        print('seed %d: %s' % (seed, bad or 'all conditions hold'))
        if not bad:
            break
    else:
        raise AssertionError('no seed satisfies the conditions')
    data = dict(pop, pixelsize_m=PIXELSIZE_M, seed=seed, stranded_code=STRANDED, lon_array=lon_array, lat_array=lat_array,
                counts_H=H, counts_H_submerged=Hsub, counts_H_stranded=Hstr)
    lat = pop['lat'].T
    mid = (np.nanmin(lat) + np.nanmax(lat)) / 2      # the reference's expression (:4096-4097)
    assert mid.dtype == np.float32
    data['mid_latitude_f32'] = mid
    data['cos_mid_latitude_f32'] = np.cos(np.radians(mid))
    assert data['cos_mid_latitude_f32'].dtype == np.float32
    res, rlon, rlat = OpenDriftSimulation.get_residence_time(o, PIXELSIZE_M)
    assert np.array_equal(rlon, lon_array) and np.array_equal(rlat, lat_array)
    data['residence'] = res
    o2 = _StandIn(pop, CATEGORIES[:2])
    out = OpenDriftSimulation.get_density_array(o2, PIXELSIZE_M)
    assert not out[2].any() and np.array_equal(out[0], H) and np.array_equal(out[3], lon_array)
    data.update(nostranded_H=out[0], nostranded_H_submerged=out[1], nostranded_H_stranded=out[2])
    for case, weight in (('wint', 'mass_int'), ('wreal', 'mass')):
        out = OpenDriftSimulation.get_density_array(o, PIXELSIZE_M, weight=weight)
        assert np.array_equal(out[3], lon_array) and np.array_equal(out[4], lat_array)
        data.update({case + '_H': out[0], case + '_H_submerged': out[1], case + '_H_stranded': out[2]})
    t = 3
    o3 = _StandIn({k: np.ascontiguousarray(v[:, t:t + 1]) for k, v in core.items()}, CATEGORIES)
    out = OpenDriftSimulation.get_density_array(o3, PIXELSIZE_M)
    assert out[0].shape[0] == 1 and out[0].sum() > 0
    data.update(single_time_index=t, single_H=out[0], single_H_submerged=out[1], single_H_stranded=out[2], single_lon_array=out[3],
                single_lat_array=out[4])
    for k, v in data.items():
        if k.endswith(('_H', '_H_submerged', '_H_stranded')) or k == 'residence':
            assert v.dtype == np.float64, k
    path = os.path.join(ROOT, 'tests', 'golden', 'c32_density.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes;', 'edges dtype', lon_array.dtype, lat_array.dtype)
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
