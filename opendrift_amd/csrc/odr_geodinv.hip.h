// WGS84 inverse geodesic on the device, and the trajectory lengths built on it (OpenDriftSimulation.get_trajectory_lengths).
//
//   get_trajectory_lengths   models/basemodel/__init__.py:4614-4628    traj_segment, k_traj_segments, k_traj_totals
//   pyproj.Geod.inv          (C. F. F. Karney, Algorithms for geodesics, J. Geodesy 87:43-55, 2013, sections 4-5)   geod_inverse
//
// geod_inverse restates the paper's inverse at order 6 for the ellipsoid of c_geod (odr_geodesic.hip.h): the end points are brought
// into the canonical order lat1 <= 0, lat1 <= lat2 <= -lat1, 0 <= lon12 <= 180; meridional and equatorial lines are closed forms;
// every other line starts from the paper's guess for alpha1 (for lines under a few decimetres the guess IS the answer; near the
// antipode it comes from the astroid equation) and solves lambda12(alpha1) = lon12 by Newton's method, with a bisection step on the
// bracket kept alongside whenever Newton leaves it, and a fixed iteration cap.
//
// The device and the host build (tests/geodinv_host.cpp) give the SAME BITS.  That rules out the math library -- its sin, cos,
// atan2 and cbrt differ between the device's and the host's in the last bit -- and every contraction the compiler chooses by itself:
// the two units are compiled with -ffp-contract=off, each fma below is written out, and gi_sincos_q / gi_atan2 / gi_cbrt are
// polynomial kernels on +, -, *, /, sqrt and fma alone (all correctly rounded on either side).  odr_geodesic.hip.h's sincosd,
// atan2d and sine series contract under `#pragma clang fp contract(fast)` and seed their reciprocals from v_rcp_f64, so they are
// restated here without either; its constants (c_geod, c_atanq, kDeg), ang_normalize and ang_round are used as they are.
//
// Rounding points of get_trajectory_lengths: float32 positions widen to float64 exactly; s12 is float64; NaN -> 0; speed = s12 / dt
// in float64 (dt with its sign); speed > 100 cuts both to 0; the total is the float64 sum in time order, one trajectory per lane.
//
// Compiled for the CPU by tests/geodinv_host.cpp: everything above the kernels is plain C++.
#pragma once
#include "odr_geodesic.hip.h"

namespace odr {

constexpr double kGiPi = 3.14159265358979323846264338327950288;
constexpr double kGiTol0 = 2.220446049250313e-16;            // 2^-52
constexpr double kGiTol1 = 200 * kGiTol0;
constexpr double kGiTol2 = 1.4901161193847656e-08;           // sqrt(tol0)
constexpr double kGiTolb = kGiTol0;
constexpr double kGiXthresh = 1000 * kGiTol2;
constexpr int kGiMaxit1 = 20, kGiMaxit2 = kGiMaxit1 + 53 + 10;      // Newton steps; the cap with the bisection steps behind them

// sin and cos on |x| <= pi/4: the fdlibm k_sin / k_cos minimax kernels, every fma written out
__host__ __device__ __forceinline__ void gi_sincos_q(double x, double &s, double &c) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double z = x * x;
  const double rs = fma(fma(fma(fma(z, S6, S5), z, S4), z, S3), z, S2);
  s = fma(z * x, fma(z, rs, S1), x);
  const double rc = z * fma(fma(fma(fma(fma(z, C6, C5), z, C4), z, C3), z, C2), z, C1);
  const double hz = 0.5 * z, w = 1.0 - hz;
  c = w + (((1.0 - w) - hz) + z * rc);
}
__host__ __device__ __forceinline__ void gi_quadrant(int q, double s, double c, double &sinx, double &cosx) {
  switch ((unsigned)q & 3U) {
    case 0U: sinx = s; cosx = c; break;
    case 1U: sinx = c; cosx = -s; break;
    case 2U: sinx = -s; cosx = -c; break;
    default: sinx = -c; cosx = s; break;
  }
  cosx += 0.0;      // no -0.0
}
// sin and cos of (x + t) degrees, |x| <= 540 and t a rounding residual: exact reduction to |r| <= 45
__host__ __device__ __forceinline__ void gi_sincosd(double x, double t, double &sinx, double &cosx) {
  const double qd = rint(x * (1.0 / 90.0));
  const double r = fma(-90.0, qd, x) + t;
  double s, c;
  gi_sincos_q(r * kDeg, s, c);
  gi_quadrant((int)qd, s, c, sinx, cosx);
}
// sin and cos of x radians, |x| <= 3.3: two-term Cody-Waite reduction by k pi/2, |k| <= 2
__host__ __device__ __forceinline__ void gi_sincos(double x, double &sinx, double &cosx) {
  const double k = rint(x * 0.63661977236758134308);
  double r = fma(-k, 1.57079632679489655800e+00, x);
  r = fma(-k, 6.12323399573676603587e-17, r);
  double s, c;
  gi_sincos_q(r, s, c);
  gi_quadrant((int)k, s, c, sinx, cosx);
}
// atan2 of finite arguments: r = min / max, atan r = r + r z q(z) with the degree-19 interpolant c_atanq, octants put back
__host__ __device__ __forceinline__ double gi_atan2(double y, double x) {
  const double ay = fabs(y), ax = fabs(x);
  const double mx = fmax(ay, ax), mn = fmin(ay, ax);
  const double r = mx > 0 ? mn / mx : 0.0;
  const double z = r * r, w = z * z;
  double qe = c_atanq[18], qo = c_atanq[19];
  for (int k = 16; k >= 0; k -= 2) { qe = fma(qe, w, c_atanq[k]); qo = fma(qo, w, c_atanq[k + 1]); }
  double a = fma(r * z, fma(qo, z, qe), r);
  a = ay > ax ? 1.57079632679489661923 - a : a;
  a = signbit(x) ? 3.14159265358979323846 - a : a;
  return copysign(a, y);
}
// in degrees, the atan taken in the octant |y| <= x so that the cardinal directions come out exactly
__host__ __device__ __forceinline__ double gi_atan2d(double y, double x) {
  int q = 0;
  if (fabs(y) > fabs(x)) { const double t = x; x = y; y = t; q = 2; }
  if (signbit(x)) { x = -x; ++q; }
  double ang = gi_atan2(y, x) * kRad2Deg;
  switch (q) {
    case 1: ang = copysign(180.0, y) - ang; break;
    case 2: ang = 90 - ang; break;
    case 3: ang = -90 + ang; break;
    default: break;
  }
  return ang;
}
// cube root: exponent / 3 on the bit pattern, then Newton steps on + * / (only the astroid's starting guess takes it)
__host__ __device__ __forceinline__ double gi_cbrt(double v) {
  const double a = fabs(v);
  if (!(a > 1e-300)) return 0.0 * v;
  unsigned long long bits;
  __builtin_memcpy(&bits, &a, 8);
  bits = bits / 3 + 0x2A9F7893782DA1CEull;
  double x;
  __builtin_memcpy(&x, &bits, 8);
  for (int k = 0; k < 6; ++k) x = x - (x * x * x - a) / (3.0 * x * x);
  return copysign(x, v);
}
__host__ __device__ __forceinline__ void gi_norm2(double &x, double &y) {
  const double r = sqrt(x * x + y * y);
  x /= r; y /= r;
}
// sum_{k=1..N} c[k] sin(2 k x) by Clenshaw's recurrence
template <int N>
__host__ __device__ __forceinline__ double gi_sin_series(double sinx, double cosx, const double *c) {
  const double ar = 2 * (cosx - sinx) * (cosx + sinx);
  double y0 = c[N], y1 = 0;
#pragma unroll
  for (int k = N - 1; k >= 1; --k) {
    const double y = fma(ar, y0, c[k] - y1);
    y1 = y0; y0 = y;
  }
  return 2 * sinx * cosx * y0;
}
__host__ __device__ __forceinline__ double gi_eps(double k2) { return k2 / (2 * (1 + sqrt(1 + k2)) + k2); }
__host__ __device__ __forceinline__ double gi_A3(double eps) {
  const double *a3 = c_geod.A3x;
  return fma(fma(fma(fma(fma(eps, a3[0], a3[1]), eps, a3[2]), eps, a3[3]), eps, a3[4]), eps, a3[5]);
}
__host__ __device__ __forceinline__ void gi_C3(double eps, double *c) {      // c[1..5]
  const double *x3 = c_geod.C3x;
  double m = eps;
  c[1] = m * fma(fma(fma(fma(eps, x3[0], x3[1]), eps, x3[2]), eps, x3[3]), eps, x3[4]);  m *= eps;
  c[2] = m * fma(fma(fma(eps, x3[5], x3[6]), eps, x3[7]), eps, x3[8]);                   m *= eps;
  c[3] = m * fma(fma(eps, x3[9], x3[10]), eps, x3[11]);                                  m *= eps;
  c[4] = m * fma(eps, x3[12], x3[13]);                                                   m *= eps;
  c[5] = m * x3[14];
}

// Distance and reduced length between sigma1 and sigma2 on the auxiliary sphere, both in units of b (eqs. 7, 40 of the paper)
template <bool WANT_S, bool WANT_M>
__host__ __device__ __forceinline__ void gi_lengths(double eps, double sig12, double ssig1, double csig1, double dn1, double ssig2,
                                                    double csig2, double dn2, double &s12b, double &m12b) {
  const double e2 = eps * eps;
  double c1[7], c2[7];
  const double A1 = (e2 * fma(e2, e2 + 4.0, 64.0) * (1.0 / 256) + eps) / (1 - eps);      // A1 - 1
  double d = eps;
  c1[1] = d * fma(e2, 6 - e2, -16.0) * (1.0 / 32);                        d *= eps;
  c1[2] = d * fma(e2, fma(e2, -9.0, 64.0), -128.0) * (1.0 / 2048);        d *= eps;
  c1[3] = d * fma(e2, 9.0, -16.0) * (1.0 / 768);                          d *= eps;
  c1[4] = d * fma(e2, 3.0, -5.0) * (1.0 / 512);                           d *= eps;
  c1[5] = d * (-7.0 / 1280);                                              d *= eps;
  c1[6] = d * (-7.0 / 2048);
  const double B1 = gi_sin_series<6>(ssig2, csig2, c1) - gi_sin_series<6>(ssig1, csig1, c1);
  if (WANT_S) s12b = (1 + A1) * (sig12 + B1);
  if (WANT_M) {
    const double A2 = (e2 * fma(e2, fma(e2, -11.0, -28.0), -192.0) * (1.0 / 256) - eps) / (1 + eps);      // A2 - 1
    d = eps;
    c2[1] = d * fma(e2, e2 + 2.0, 16.0) * (1.0 / 32);                     d *= eps;
    c2[2] = d * fma(e2, fma(e2, 35.0, 64.0), 384.0) * (1.0 / 2048);       d *= eps;
    c2[3] = d * fma(e2, 15.0, 80.0) * (1.0 / 768);                        d *= eps;
    c2[4] = d * fma(e2, 7.0, 35.0) * (1.0 / 512);                         d *= eps;
    c2[5] = d * (63.0 / 1280);                                            d *= eps;
    c2[6] = d * (77.0 / 2048);
    const double B2 = gi_sin_series<6>(ssig2, csig2, c2) - gi_sin_series<6>(ssig1, csig1, c2);
    const double J12 = (A1 - A2) * sig12 + ((1 + A1) * B1 - (1 + A2) * B2);
    m12b = dn2 * (csig1 * ssig2) - dn1 * (ssig1 * csig2) - csig1 * csig2 * J12;
  }
}

// the positive root k of k^4 + 2 k^3 - (x^2 + y^2 - 1) k^2 - 2 y^2 k - y^2 = 0 (eq. 55)
__host__ __device__ __forceinline__ double gi_astroid(double x, double y) {
  const double p = x * x, q = y * y, r = (p + q - 1) / 6;
  if (q == 0 && r <= 0) return 0;
  const double S = p * q / 4, r2 = r * r, r3 = r * r2, disc = S * (S + 2 * r3);
  double u = r;
  if (disc >= 0) {
    double T3 = S + r3;
    T3 += T3 < 0 ? -sqrt(disc) : sqrt(disc);
    const double T = gi_cbrt(T3);
    u += T + (T != 0 ? r2 / T : 0);
  } else {
    const double ang = gi_atan2(sqrt(-disc), -(S + r3));
    double sa, ca;
    gi_sincos(ang / 3, sa, ca);
    u += 2 * r * ca;
  }
  const double v = sqrt(u * u + q);
  const double uv = u < 0 ? q / (v - u) : u + v;
  const double w = (uv - q) / (2 * v);
  return uv / (sqrt(uv + w * w) + w);
}

struct GiEnds { double sbet1, cbet1, dn1, sbet2, cbet2, dn2; };

// The starting alpha1 (section 5).  Returns sigma12 >= 0 when the guess is the answer (short lines: salp2 / calp2 / dnm are set).
__host__ __device__ __forceinline__ double gi_start(const GiEnds &E, double lam12, double slam12, double clam12, double &salp1,
                                                    double &calp1, double &salp2, double &calp2, double &dnm) {
  const GeodConst &g = c_geod;
  const double sbet1 = E.sbet1, cbet1 = E.cbet1, sbet2 = E.sbet2, cbet2 = E.cbet2;
  double sig12 = -1;
  const double sbet12 = sbet2 * cbet1 - cbet2 * sbet1, cbet12 = cbet2 * cbet1 + sbet2 * sbet1;
  const double sbet12a = sbet2 * cbet1 + cbet2 * sbet1;
  const bool shortline = cbet12 >= 0 && sbet12 < 0.5 && cbet2 * lam12 < 0.5;
  double somg12, comg12;
  if (shortline) {
    double sbetm2 = (sbet1 + sbet2) * (sbet1 + sbet2);
    sbetm2 /= sbetm2 + (cbet1 + cbet2) * (cbet1 + cbet2);
    dnm = sqrt(1 + g.ep2 * sbetm2);
    gi_sincos(lam12 / (g.f1 * dnm), somg12, comg12);
  } else {
    somg12 = slam12; comg12 = clam12;
  }
  salp1 = cbet2 * somg12;
  calp1 = comg12 >= 0 ? sbet12 + cbet2 * sbet1 * (somg12 * somg12) / (1 + comg12)
                      : sbet12a - cbet2 * sbet1 * (somg12 * somg12) / (1 - comg12);
  const double ssig12 = sqrt(salp1 * salp1 + calp1 * calp1), csig12 = sbet1 * sbet2 + cbet1 * cbet2 * comg12;
  // etol2 = 0.1 tol2 / sqrt(max(0.001, f) min(1, 1 - f / 2) / 2)
  const double etol2 = 0.1 * kGiTol2 / sqrt(fmax(0.001, g.f) * fmin(1.0, 1 - g.f / 2) / 2);
  if (shortline && ssig12 < etol2) {
    salp2 = cbet1 * somg12;
    calp2 = sbet12 - cbet1 * sbet2 * (comg12 >= 0 ? (somg12 * somg12) / (1 + comg12) : 1 - comg12);
    gi_norm2(salp2, calp2);
    sig12 = gi_atan2(ssig12, csig12);
  } else if (csig12 >= 0 || ssig12 >= 6 * g.n * kGiPi * (cbet1 * cbet1)) {
    // the spherical guess is good enough
  } else {
    // near the antipode: x, y of the astroid problem (eq. 53)
    const double lam12x = gi_atan2(-slam12, -clam12);      // lam12 - pi
    const double lamscale = g.f * cbet1 * gi_A3(gi_eps(sbet1 * sbet1 * g.ep2)) * kGiPi;
    const double betscale = lamscale * cbet1;
    const double x = lam12x / lamscale, y = sbet12a / betscale;
    if (y > -kGiTol1 && x > -1 - kGiXthresh) {      // the strip next to the cut
      salp1 = fmin(1.0, -x);
      calp1 = -sqrt(1 - salp1 * salp1);
    } else {
      const double k = gi_astroid(x, y);
      const double omg12a = lamscale * (-x * k / (1 + k));
      gi_sincos(omg12a, somg12, comg12);
      comg12 = -comg12;
      salp1 = cbet2 * somg12;
      calp1 = sbet12a - cbet2 * sbet1 * (somg12 * somg12) / (1 - comg12);
    }
  }
  if (!(salp1 <= 0)) gi_norm2(salp1, calp1);
  else { salp1 = 1; calp1 = 0; }
  return sig12;
}

struct GiLine { double salp2, calp2, sig12, ssig1, csig1, ssig2, csig2, eps; };

// lambda12(alpha1) - lon12 and d lambda12 / d alpha1 (eqs. 8, 23, 46)
__host__ __device__ __forceinline__ double gi_lambda12(const GiEnds &E, double salp1, double calp1, double slam120, double clam120,
                                                       GiLine &L, double &dlam12) {
  const GeodConst &g = c_geod;
  const double sbet1 = E.sbet1, cbet1 = E.cbet1, sbet2 = E.sbet2, cbet2 = E.cbet2;
  if (sbet1 == 0 && calp1 == 0) calp1 = -kTiny;      // an equatorial line heads a hair south
  const double salp0 = salp1 * cbet1;
  const double t0 = salp1 * sbet1;
  const double calp0 = sqrt(calp1 * calp1 + t0 * t0);
  double ssig1 = sbet1, csig1 = calp1 * cbet1;
  const double somg1 = salp0 * sbet1, comg1 = csig1;
  gi_norm2(ssig1, csig1);
  const double salp2 = cbet2 != cbet1 ? salp0 / cbet2 : salp1;
  const double t1 = calp1 * cbet1;
  const double calp2 = cbet2 != cbet1 || fabs(sbet2) != -sbet1
                           ? sqrt(t1 * t1 + (cbet1 < -sbet1 ? (cbet2 - cbet1) * (cbet1 + cbet2) : (sbet1 - sbet2) * (sbet1 + sbet2))) / cbet2
                           : fabs(calp1);
  double ssig2 = sbet2, csig2 = calp2 * cbet2;
  const double somg2 = salp0 * sbet2, comg2 = csig2;
  gi_norm2(ssig2, csig2);
  const double sig12 = gi_atan2(fmax(0.0, csig1 * ssig2 - ssig1 * csig2) + 0.0, csig1 * csig2 + ssig1 * ssig2);
  const double somg12 = fmax(0.0, comg1 * somg2 - somg1 * comg2) + 0.0, comg12 = comg1 * comg2 + somg1 * somg2;
  const double eta = gi_atan2(somg12 * clam120 - comg12 * slam120, comg12 * clam120 + somg12 * slam120);
  const double eps = gi_eps(calp0 * calp0 * g.ep2);
  double c3[6];
  gi_C3(eps, c3);
  const double B312 = gi_sin_series<5>(ssig2, csig2, c3) - gi_sin_series<5>(ssig1, csig1, c3);
  const double lam12 = eta + -g.f * gi_A3(eps) * salp0 * (sig12 + B312);
  if (calp2 == 0) dlam12 = -2 * g.f1 * E.dn1 / sbet1;
  else {
    double s_unused, m12b;
    gi_lengths<false, true>(eps, sig12, ssig1, csig1, E.dn1, ssig2, csig2, E.dn2, s_unused, m12b);
    dlam12 = m12b * g.f1 / (calp2 * cbet2);
  }
  L.salp2 = salp2; L.calp2 = calp2; L.sig12 = sig12; L.ssig1 = ssig1; L.csig1 = csig1; L.ssig2 = ssig2; L.csig2 = csig2; L.eps = eps;
  return lam12;
}

// The shortest geodesic from (lat1, lon1) to (lat2, lon2), degrees: length s12 in metres, forward azimuths at both ends in degrees.
// A NaN or an infinite argument and |lat| > 90 give NaN; coincident points give 0, 0, 0.
__host__ __device__ __forceinline__ void geod_inverse(double lat1, double lon1, double lat2, double lon2, double &s12, double &azi1,
                                                      double &azi2) {
  const GeodConst &g = c_geod;
  if (!(fabs(lat1) <= 90 && fabs(lat2) <= 90 && fabs(lon1) < 1e300 && fabs(lon2) < 1e300)) {
    s12 = azi1 = azi2 = NAN;
    return;
  }
  // lon12 = lon2 - lon1 in [-180, 180] with its rounding residual (two exact sums)
  double lon12, lon12s;
  {
    const double x = ang_normalize(-lon1), y = ang_normalize(lon2);
    double s = x + y, up = s - y, vpp = s - up;
    double t = -((up - x) + (vpp - y));
    const double d = ang_normalize(s);
    s = d + t; up = s - t; vpp = s - up;
    t = -((up - d) + (vpp - t));
    lon12 = s; lon12s = t;
    if (lon12 == 0 || fabs(lon12) == 180) lon12 = copysign(lon12, lon12s == 0 ? lon2 - lon1 : -lon12s);
  }
  const bool coincident = lat1 == lat2 && lon12 == 0 && lon12s == 0;
  int lonsign = signbit(lon12) ? -1 : 1;
  lon12 *= lonsign; lon12s *= lonsign;
  const double lam12 = lon12 * kDeg;
  double slam12, clam12;
  gi_sincosd(lon12, lon12s, slam12, clam12);
  lon12s = (180 - lon12) - lon12s;      // the supplement of the longitude difference
  lat1 = ang_round(lat1); lat2 = ang_round(lat2);
  const int swapp = fabs(lat1) < fabs(lat2) ? -1 : 1;
  if (swapp < 0) { lonsign = -lonsign; const double t = lat1; lat1 = lat2; lat2 = t; }
  const int latsign = signbit(lat1) ? 1 : -1;
  lat1 *= latsign; lat2 *= latsign;
  // now lat1 <= -0 and lat1 <= lat2 <= -lat1, 0 <= lon12 <= 180

  GiEnds E;
  gi_sincosd(lat1, 0.0, E.sbet1, E.cbet1);
  E.sbet1 *= g.f1; gi_norm2(E.sbet1, E.cbet1); E.cbet1 = fmax(kTiny, E.cbet1);
  gi_sincosd(lat2, 0.0, E.sbet2, E.cbet2);
  E.sbet2 *= g.f1; gi_norm2(E.sbet2, E.cbet2); E.cbet2 = fmax(kTiny, E.cbet2);
  // equal |latitudes| must give equal reduced latitudes to the last bit: the meridional and equatorial cases test for it
  if (E.cbet1 < -E.sbet1) { if (E.cbet2 == E.cbet1) E.sbet2 = copysign(E.sbet1, E.sbet2); }
  else { if (fabs(E.sbet2) == -E.sbet1) E.cbet2 = E.cbet1; }
  E.dn1 = sqrt(1 + g.ep2 * (E.sbet1 * E.sbet1));
  E.dn2 = sqrt(1 + g.ep2 * (E.sbet2 * E.sbet2));

  double salp1 = 0, calp1 = 0, salp2 = 0, calp2 = 0, s12x = 0, m12x = 0;
  bool meridian = lat1 == -90 || slam12 == 0;
  if (meridian) {
    calp1 = clam12; salp1 = slam12;      // head to the target longitude
    calp2 = 1; salp2 = 0;                // arrive heading north
    const double ssig1 = E.sbet1, csig1 = calp1 * E.cbet1, ssig2 = E.sbet2, csig2 = calp2 * E.cbet2;
    const double sig12 = gi_atan2(fmax(0.0, csig1 * ssig2 - ssig1 * csig2) + 0.0, csig1 * csig2 + ssig1 * ssig2);
    gi_lengths<true, true>(g.n, sig12, ssig1, csig1, E.dn1, ssig2, csig2, E.dn2, s12x, m12x);
    // a meridional line is the shortest one only up to its first conjugate point (m12 >= 0)
    if (sig12 < 1 || m12x >= 0) {
      if (sig12 < 3 * kTiny || (sig12 < kGiTol0 && (s12x < 0 || m12x < 0))) s12x = 0;
      s12x *= g.b;
    } else {
      meridian = false;
    }
  }
  if (!meridian && E.sbet1 == 0 && lon12s >= g.f * 180) {
    // equatorial and short of the first conjugate point
    calp1 = calp2 = 0; salp1 = salp2 = 1;
    s12x = g.a * lam12;
  } else if (!meridian) {
    double dnm = 0;
    const double sig12 = gi_start(E, lam12, slam12, clam12, salp1, calp1, salp2, calp2, dnm);
    if (sig12 >= 0) {
      s12x = sig12 * g.b * dnm;
    } else {
      // Newton on lambda12(alpha1) = lon12; [alpha1a, alpha1b] brackets the root and takes over when Newton leaves it
      GiLine L;
      double salp1a = kTiny, calp1a = 1, salp1b = kTiny, calp1b = -1;
      bool tripn = false, tripb = false;
      for (int numit = 0;; ++numit) {
        double dv = 0;
        const double v = gi_lambda12(E, salp1, calp1, slam12, clam12, L, dv);
        if (tripb || !(fabs(v) >= (tripn ? 8 : 1) * kGiTol0) || numit == kGiMaxit2) break;
        if (v > 0 && (numit > kGiMaxit1 || calp1 / salp1 > calp1b / salp1b)) { salp1b = salp1; calp1b = calp1; }
        else if (v < 0 && (numit > kGiMaxit1 || calp1 / salp1 < calp1a / salp1a)) { salp1a = salp1; calp1a = calp1; }
        if (numit < kGiMaxit1 && dv > 0) {
          const double dalp1 = -v / dv;
          if (fabs(dalp1) < kGiPi) {
            double sdalp1, cdalp1;
            gi_sincos(dalp1, sdalp1, cdalp1);
            const double nsalp1 = salp1 * cdalp1 + calp1 * sdalp1;
            if (nsalp1 > 0) {
              calp1 = calp1 * cdalp1 - salp1 * sdalp1;
              salp1 = nsalp1;
              gi_norm2(salp1, calp1);
              tripn = fabs(v) <= 16 * kGiTol0;      // close enough: one more step and out
              continue;
            }
          }
        }
        salp1 = (salp1a + salp1b) / 2;
        calp1 = (calp1a + calp1b) / 2;
        gi_norm2(salp1, calp1);
        tripn = false;
        tripb = fabs(salp1a - salp1) + (calp1a - calp1) < kGiTolb || fabs(salp1 - salp1b) + (calp1 - calp1b) < kGiTolb;
      }
      double m_unused;
      gi_lengths<true, false>(L.eps, L.sig12, L.ssig1, L.csig1, E.dn1, L.ssig2, L.csig2, E.dn2, s12x, m_unused);
      s12x *= g.b;
      salp2 = L.salp2; calp2 = L.calp2;
    }
  }
  s12 = 0.0 + s12x;
  if (coincident) { azi1 = azi2 = 0; return; }
  if (swapp < 0) {
    double t = salp1; salp1 = salp2; salp2 = t;
    t = calp1; calp1 = calp2; calp2 = t;
  }
  salp1 *= swapp * lonsign; calp1 *= swapp * latsign;
  salp2 *= swapp * lonsign; calp2 *= swapp * latsign;
  azi1 = gi_atan2d(salp1, calp1);
  azi2 = gi_atan2d(salp2, calp2);
}

// One output interval of get_trajectory_lengths (:4619-4625): NaN -> 0, speed = distance / dt, speed > 100 -> both 0
__host__ __device__ __forceinline__ void traj_segment(float lon1, float lat1, float lon2, float lat2, double dt, double &distance,
                                                      double &speed) {
  double s12, azi1, azi2;
  geod_inverse((double)lat1, (double)lon1, (double)lat2, (double)lon2, s12, azi1, azi2);
  if (s12 != s12) s12 = 0;
  double v = s12 / dt;
  if (v > 100) { s12 = 0; v = 0; }
  distance = s12; speed = v;
}

#if !defined(ODR_GEODINV_HOST) && !defined(ODR_GEODINV_NO_KERNELS)      // odr_seed.hip.h takes the functions alone
constexpr int TRAJ_TILE = 64;                     // trajectories and output intervals of one workgroup's tile
constexpr int TRAJ_TILE_PITCH = TRAJ_TILE + 1;    // floats of a tile row: 65 times, and odd, so that a wave reading a column hits every bank once

// n pairs, one per lane; any output may be NULL
__global__ __launch_bounds__(BLOCK) void k_geod_inverse(long long n, const double *__restrict__ lon1, const double *__restrict__ lat1,
                                                        const double *__restrict__ lon2, const double *__restrict__ lat2,
                                                        double *__restrict__ azi1, double *__restrict__ azi2, double *__restrict__ s12) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double s, a1, a2;
  geod_inverse(lat1[i], lon1[i], lat2[i], lon2[i], s, a1, a2);
  if (azi1) azi1[i] = a1;
  if (azi2) azi2[i] = a2;
  if (s12) s12[i] = s;
}

// A workgroup takes 64 trajectories x 64 output intervals.  It reads the 65 positions of each of its trajectories along time (lanes
// along a row of the [trajectory][time] arrays) into LDS, then turns: a wave holds one output interval of the 64 trajectories, reads
// its two LDS columns without a bank conflict and writes 512 contiguous bytes of distances[interval][trajectory] (and of speeds).
// lon, lat: n_traj rows of n_times; dist, speed: rows of `pitch` doubles (speed may be NULL).  blockIdx.x: tile of trajectories
// first, tiles_traj of them per tile of intervals.
__global__ __launch_bounds__(BLOCK) void k_traj_segments(const float *__restrict__ lon, const float *__restrict__ lat, long long n_traj,
                                                         int n_times, unsigned tiles_traj, double dt, long long pitch,
                                                         double *__restrict__ dist, double *__restrict__ speed) {
  __shared__ float s_lon[TRAJ_TILE * TRAJ_TILE_PITCH], s_lat[TRAJ_TILE * TRAJ_TILE_PITCH];
  const unsigned tile_t = blockIdx.x / tiles_traj, tile_r = blockIdx.x - tile_t * tiles_traj;
  const long long r0 = (long long)tile_r * TRAJ_TILE;
  const int t0 = (int)tile_t * TRAJ_TILE;
  const int nt = min(TRAJ_TILE + 1, n_times - t0);               // positions of a row in this tile, >= 2
  const int nr = (int)min((long long)TRAJ_TILE, n_traj - r0);    // rows
  for (int k = threadIdx.x; k < TRAJ_TILE * TRAJ_TILE_PITCH; k += BLOCK) {
    const int row = k / TRAJ_TILE_PITCH, col = k - row * TRAJ_TILE_PITCH;
    if (row < nr && col < nt) {
      const size_t src = (size_t)(r0 + row) * (size_t)n_times + (size_t)(t0 + col);
      s_lon[k] = lon[src];
      s_lat[k] = lat[src];
    }
  }
  __syncthreads();
  const int row = threadIdx.x & (TRAJ_TILE - 1);
  if (row >= nr) return;
  for (int seg = threadIdx.x / TRAJ_TILE; seg < nt - 1; seg += BLOCK / TRAJ_TILE) {
    const int k = row * TRAJ_TILE_PITCH + seg;
    double d, v;
    traj_segment(s_lon[k], s_lat[k], s_lon[k + 1], s_lat[k + 1], dt, d, v);
    const size_t dst = (size_t)(t0 + seg) * (size_t)pitch + (size_t)(r0 + row);
    dist[dst] = d;
    if (speed) speed[dst] = v;
  }
}

// np.cumsum(distances, 0)[-1, :]: one trajectory per lane, the float64 sum in time order; a wave reads 512 contiguous bytes per row
__global__ __launch_bounds__(BLOCK) void k_traj_totals(const double *__restrict__ dist, long long n_traj, int n_segments, long long pitch,
                                                       double *__restrict__ total) {
  const long long r = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= n_traj) return;
  double sum = dist[r];
  for (int t = 1; t < n_segments; ++t) sum += dist[(size_t)t * (size_t)pitch + (size_t)r];
  total[r] = sum;
}
#endif  // kernels

}  // namespace odr
