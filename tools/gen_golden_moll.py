"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/proj_kat_moll.npz: known answers of +proj=moll from its DEFINITION.

Mollweide on the sphere of radius a (Snyder, USGS PP 1395, 31-1 .. 31-3): 2 th + sin 2 th = pi sin phi, x = (2 sqrt 2 / pi) a lam cos th,
y = sqrt 2 a sin th, lam the longitude from the central meridian in (-180, 180] degrees.  Solved with mpmath at 40 digits by bisection
(the left-hand side is monotone in th, so the vanishing derivative at the pole needs no care); x and y are rounded to
float64 once.  The inverse answers are the points themselves.

200 points for '+proj=moll +a=6378137 +lon_0=15 +x_0=200000 +y_0=-100000': both poles (on and off the central meridian), the equator,
+-180 degrees from the central meridian, latitudes within 1e-9 .. 1e-3 degrees of a pole, and random points.

    python tools/gen_golden_moll.py
"""
import os

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, LON0, X0, Y0 = 6378137.0, 15.0, 200000.0, -100000.0
PROJ4 = '+proj=moll +a=6378137 +lon_0=15 +x_0=200000 +y_0=-100000'
mp.mp.dps = 40


def theta(phi):
    """th in [-pi/2, pi/2] with 2 th + sin 2 th = pi sin phi (monotone in th: bisection to 40 digits)"""
    k = mp.pi * mp.sin(phi)
    lo, hi = -mp.pi / 2, mp.pi / 2
    for _ in range(150):
        mid = (lo + hi) / 2
        if 2 * mid + mp.sin(2 * mid) < k:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def forward(lon, lat):
    d = mp.mpf(lon) - mp.mpf(LON0)
    if d > 180:
        d -= 360
    if d < -180:
        d += 360
    # (at a pole th = +-pi/2 exactly; the bisection would leave it at 1e-13, the cube root of the working precision)
    th = mp.sign(lat) * mp.pi / 2 if abs(lat) == 90 else theta(mp.radians(mp.mpf(lat)))
    x = 2 * mp.sqrt(2) / mp.pi * A * mp.radians(d) * mp.cos(th) + X0
    y = mp.sqrt(2) * A * mp.sin(th) + Y0
    return float(x), float(y)


def main():
    rng = np.random.default_rng(7)
    pts = [(15.0, 90.0), (15.0, -90.0), (80.0, 90.0), (-120.0, -90.0), (15.0, 0.0), (100.0, 0.0), (-60.0, 0.0), (195.0, 0.0),
           (-165.0, 0.0), (195.0, 45.0), (-165.0, -45.0), (195.0, 89.0), (-165.0, 30.0), (15.0, 30.0), (40.0, 29.999999), (40.0, 30.000001)]
    for d in (1e-9, 1e-7, 1e-5, 1e-3, 0.1, 1.0):
        pts += [(60.0, 90.0 - d), (-100.0, -90.0 + d)]
    for d in (1e-12, 1e-9, 1e-6, 1e-3):
        pts += [(70.0, d), (-20.0, -d)]
    while len(pts) < 200:
        pts.append((float(rng.uniform(-179.0, 179.0)) + LON0, float(np.degrees(np.arcsin(rng.uniform(-1, 1))))))
    lon, lat = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    xy = np.array([forward(a, b) for a, b in zip(lon, lat)])
    path = os.path.join(ROOT, 'tests', 'golden', 'proj_kat_moll.npz')
    np.savez_compressed(path, proj4=PROJ4, a=A, lon0=LON0, x0=X0, y0=Y0, lon=lon, lat=lat, x=xy[:, 0], y=xy[:, 1])
    print(path, os.path.getsize(path), 'bytes;', len(pts), 'points')


if __name__ == '__main__':
    main()
