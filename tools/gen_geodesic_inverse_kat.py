"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/geodesic_inverse_kat.npz: known answers of the WGS84 INVERSE problem.

Every row (lat1, lon1, azi1, s12, lat2, lon2, azi2) is a DIRECT solve at 34 digits: exact_direct_mp of oracle/validate_geodesic.py
(the closed-form integrals of Karney 2013, eqs. 7-8, by mpmath quadrature and root finding), with lat2, lon2, azi2 rounded to float64
once.  Every s12 is at most 19 900 km, below pi b = 19 970 km, the smallest distance at which a WGS84 geodesic stops being the
shortest one: so the line of each row is THE shortest line between its end points and the inverse problem has one answer, (azi1,
s12, azi2).  Rounding the stored end point moves that answer by about 3e-9 m (half an ulp of 180 degrees is 1.6e-9 m on the ground).

Classes (column `cls`):
  0  1 mm .. 1 km            1  1 .. 1000 km            2  1000 .. 19 900 km
  3  meridional (azi1 = 0 or 180), a third of them across a pole
  4  equatorial (lat1 = 0, azi1 = +-90)
  5  point 2 within 1 degree of the antipode of point 1 (19 880 .. 19 900 km)
  6  point 1 on the +-180 seam, or the line across it

    python tools/gen_geodesic_inverse_kat.py      (about 200 rows; also prints what the host build of csrc/odr_geodinv.hip.h makes of them)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import oracle as orc  # noqa: E402
from oracle.validate_geodesic import exact_direct_mp  # noqa: E402

S_MAX = 19.9e6


def wrap(d):
    d = float(d)
    return d - 360.0 * round(d / 360.0)


def antipode_offset_deg(lat1, lon1, lat2, lon2):
    """angle between point 2 and the antipode of point 1 (spherical, good enough to classify)"""
    la, lo = np.radians(-lat1), np.radians(lon1 + 180.0)
    lb, lob = np.radians(lat2), np.radians(lon2)
    c = np.sin(la) * np.sin(lb) + np.cos(la) * np.cos(lb) * np.cos(lo - lob)
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


def cases(rng):
    out = []
    for lo_exp, hi_exp, cls, n in ((-3, 3, 0, 30), (3, 6, 1, 30)):
        for _ in range(n):
            out.append((cls, rng.uniform(-89, 89), rng.uniform(-180, 180), rng.uniform(-180, 180), 10 ** rng.uniform(lo_exp, hi_exp)))
    for _ in range(40):
        out.append((2, rng.uniform(-89, 89), rng.uniform(-180, 180), rng.uniform(-180, 180), rng.uniform(1e6, S_MAX)))
    for k in range(27):
        if k % 3 == 0:      # across a pole: from within 15 degrees of it, heading for it, 2000 .. 8000 km
            lat = rng.uniform(75, 89) * (1 if k % 2 else -1)
            out.append((3, lat, rng.uniform(-180, 180), 0.0 if lat > 0 else 180.0, rng.uniform(2e6, 8e6)))
        else:
            out.append((3, rng.uniform(-80, 80), rng.uniform(-180, 180), 0.0 if k % 2 else 180.0, 10 ** rng.uniform(-2, 6.5)))
    for k in range(20):
        out.append((4, 0.0, rng.uniform(-180, 180), 90.0 if k % 2 else -90.0, 10 ** rng.uniform(-2, np.log10(S_MAX))))
    n = 0
    while n < 30:
        lat, lon, az, s = rng.uniform(-80, 80), rng.uniform(-180, 180), rng.uniform(-180, 180), rng.uniform(19.88e6, S_MAX)
        lo2, la2, _ = orc.geod_fwd(lon, lat, az, s)
        if antipode_offset_deg(lat, lon, la2[0], lo2[0]) < 0.95:
            out.append((5, lat, lon, az, s))
            n += 1
    for k in range(25):
        lat, az, s = rng.uniform(-85, 85), rng.uniform(-180, 180), 10 ** rng.uniform(-2, 6.8)
        if k < 10:
            out.append((6, lat, 180.0, az, s))
        elif k < 20:
            out.append((6, lat, -180.0, az, s))
        else:      # a line across the seam: from just west of it, heading east, longer than the gap
            out.append((6, lat, 179.99, rng.uniform(60, 120), rng.uniform(5e3, 3e6)))
    return out


def main():
    rng = np.random.default_rng(20261019)
    rows, cls = [], []
    for c, lat1, lon1, azi1, s12 in cases(rng):
        assert s12 <= S_MAX
        lat2, lon2, azi2 = exact_direct_mp(lat1, lon1, azi1, s12)
        rows.append((lat1, lon1, azi1, s12, float(lat2), wrap(lon2), wrap(azi2)))
        cls.append(c)
    rows, cls = np.array(rows), np.array(cls, dtype=np.int32)
    near = antipode_offset_deg(rows[:, 0], rows[:, 1], rows[:, 4], rows[:, 5])
    assert (near[cls == 5] < 1.0).all(), near[cls == 5].max()
    crossing = (cls == 6) & (np.abs(rows[:, 1]) != 180.0)
    assert (rows[crossing, 5] < 0).all(), 'a seam row does not cross the seam'
    assert (np.abs(rows[cls == 3, 5] - rows[cls == 3, 1]) > 90).sum() >= 5, 'fewer than 5 rows across a pole'
    assert rows[:, 3].max() <= S_MAX and len(rows) >= 200
    path = os.path.join(ROOT, 'tests', 'golden', 'geodesic_inverse_kat.npz')
    np.savez_compressed(path, rows=rows, cls=cls)
    print(path, os.path.getsize(path), 'bytes,', len(rows), 'rows')

    import geodinv_host as gh
    a1, a2, s = gh.inverse(rows[:, 1], rows[:, 0], rows[:, 5], rows[:, 4])
    land = gh.landing_error_m(a1, s, rows[:, 2], rows[:, 3])
    for c in range(7):
        m = cls == c
        print('class %d: %3d rows, host build max |s12 - KAT| %.3g m, landing error %.3g m' % (c, m.sum(), np.abs(s - rows[:, 3])[m].max(),
                                                                                             land[m].max()))
    print('all: max |s12 - KAT| %.4g m, landing error %.4g m' % (np.abs(s - rows[:, 3]).max(), land.max()))


if __name__ == '__main__':
    main()
