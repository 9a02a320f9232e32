// ShipDrift: drift of a ship from wind force, wave-drift force, wave damping and form drag (Soergaard & Vada 1998).
//
//   ShipDrift.update                       models/shipdrift.py:216-343             ship_forces, k_ship_drift
//   wave_period, significant_wave_height   models/physics_methods.py:893-943       ship_forces (hs_mode, tp_mode)
//
// One thread carries one ship through the whole loop body: first move with the current, wind force, the 100-point wave spectrum
// and the two trapezoid integrals over it (running sums in registers), period factors, the four damping iterations, second
// move, stranding.
//
// The wave-force table.  The reference asks two scipy.interpolate.LinearNDInterpolator objects (a Qhull triangulation of the
// 14 x 4 x 4 grid of wforce.dat) for F and D at the 49 spectrum points below omega = 7 and at the ship's clipped ratios
// (beam / length, draft / length).  Those ratios never change and the 49 frequencies are constants of the model, so the host
// evaluates the interpolators ONCE per class (a unique pair of clipped float32 ratios) and the device reads
// double table[n_classes][49][2] (F, D) from global memory by the element's class index.
//
// Rounding contract (the dtype ladder of NumPy 2, asserted on the reference by tools/gen_golden_shipdrift.py).  Element
// properties and the environment are float32 arrays, Python scalars are weak: Tm, Hs, bl, dl, scale1, the wind force, beta1, the
// spectrum value s[i] and the period factors are float32 chains, one IEEE single operation per NumPy operation in the reference's
// order.  s is stored into a float64 array; F_wave, beta2, wave_dir and everything behind them are float64.  One quirk: from the
// 51st spectrum point on f1, f2, d1, d2 are Python floats, so 0.5 * (f1 + f2) * dom is a Python float and its product with the
// float32 array scale1 is a float32 product; up to the 50th it is float64.  No contraction (-ffp-contract=off on both sides).
// NumPy's float32 exp and power are not correctly rounded; here exp is the float64 function rounded once and the 4th / 5th power
// products in float64 rounded once: the values differ from the reference's in the last place of a float32 (DESIGN.md section 7f
// for the measured bounds).  exp, cos, sin, atan2 of the device library and of the host's libm differ in the last place too.
//
// Compiled for the CPU by tests/ship_host.cpp: includes nothing (the includer provides <cmath> and __fdiv_rn); the kernel (not
// part of the host build) takes BLOCK, PView and the moves from odr_kernels.hip.h, which the translation unit includes first.
#pragma once

namespace odr {

enum { SHIP_LENGTH = 0, SHIP_HEIGHT = 1, SHIP_DRAFT = 2, SHIP_BEAM = 3, SHIP_WIND_DRAG = 4, SHIP_WATER_DRAG = 5, SHIP_ORIENTATION = 6,
       SHIP_CLASS = 7 };   // property slots of the model
constexpr int SHIP_NSPEC = 100;     // spectrum points (NSPEC, :249)
constexpr int SHIP_NTAB = 49;       // of which below ommin3 = 7: the rows of a class table

struct ShipEnv { float u, v, xwind, ywind, sx, sy, hs, tm; };      // the float32 environment of one element
struct ShipProp { float length, height, draft, beam, cf, cd; int orientation; };
// every intermediate the golden stores (the kernel keeps vu, vv)
struct ShipForces {
  float bl, dl, Tm, Hs, F_wind_x, F_wind_y, beta1;
  double F_wave_b, beta2_b, F_wave, beta2, wave_dir, F_total, uw_tot, uw_dir, vu, vv;
};

// np.clip(x, lo, hi) = minimum(maximum(x, lo), hi)
__host__ __device__ __forceinline__ float ship_clip(float x, float lo, float hi) {
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

// The clipped ratios (:220-227) that select the class
__host__ __device__ __forceinline__ void ship_ratios(float length, float draft, float beam, float &bl, float &dl) {
  dl = __fdiv_rn(draft, length);
  bl = __fdiv_rn(beam, length);
  bl = ship_clip(bl, 0.12f, 0.18f);
  dl = ship_clip(dl, 0.025f, 0.07f);
  bl = ship_clip(bl, 0.121f, 0.179f);      // "additional clipping to avoid NaN from interpolator"
  dl = ship_clip(dl, 0.0251f, 0.069f);
}

// update() between the two update_positions calls (:218-338) for one element.  tab: the [49][2] table of the element's class.
// hs_mode: 0 wave height from the environment, 1 from the wind (0.0246 |wind|^2, float32).  tp_mode: 0 period from the
// environment, 3 from the wind (2 pi / omega in float64, omega = 5 where the wind is calm) as read back from the float32
// environment (calculate_missing_environment_variables has stored it there before update() runs, physics_methods.py:876-883).
__host__ __device__ __forceinline__ ShipForces ship_forces(const ShipEnv &e, const ShipProp &p, const double *__restrict__ tab, int hs_mode,
                                                           int tp_mode, int dir_from_stokes) {
  ShipForces r;
  const float ws = sqrtf(e.xwind * e.xwind + e.ywind * e.ywind);      // wind_speed(): np.sqrt(x**2 + y**2)
  const float ws2 = ws * ws;                                          // np.power(wind_speed(), 2)
  r.Hs = hs_mode == 0 ? e.hs : 0.0246f * ws2;
  if (tp_mode == 0) r.Tm = e.tm;
  else {
    double omega = 5;
    if (ws > 0) omega = (double)__fdiv_rn((float)(0.877 * 9.81), 1.17f * ws);
    r.Tm = (float)((2 * 3.141592653589793) / omega);
  }
  ship_ratios(p.length, p.draft, p.beam, r.bl, r.dl);

  // wind force (:234-245): 0.5 * rho_air * Cf * area_dry * |wind|^2, decomposed; calm elements get 0
  const float area_dry = p.length * (p.height - p.draft), area_wet = p.length * p.draft;
  const float F_wind = ((0.625f * p.cf) * area_dry) * ws2;
  r.F_wind_x = ws == 0 ? 0.f : __fdiv_rn(F_wind * e.xwind, ws);
  r.F_wind_y = ws == 0 ? 0.f : __fdiv_rn(F_wind * e.ywind, ws);

  // wave spectrum and the two integrals (:247-287)
  const double dom = (12.0 - 2.25) / (SHIP_NSPEC - 1);
  const float scale1 = sqrtf(__fdiv_rn(9.81f, p.length));
  // A period of exactly 0 (a reader that does not cover the ship: the fallback): the reference replaces it by the mean of the
  // other elements' periods (physics_methods.py:936-939), which is not built; such a ship gets NO waves here (spectrum 0:
  // F_wave = beta2 = 0, it drifts with current and wind force) instead of the NaN of 2 pi / 0
  const float q = r.Tm == 0.f ? 0.f : __fdiv_rn(6.283185307179586f, r.Tm);
  const double q2 = (double)q * (double)q;
  const float tmp = (float)(q2 * q2);                                  // np.power(2 pi / Tm, 4)
  const float d = __fdiv_rn((tmp * r.Hs) * r.Hs, 12.566370614359172f);
  const float b = __fdiv_rn(tmp, 3.141592653589793f);
  double F = 0.0, B = 0.0, f2 = 0.0, d2 = 0.0;
  for (int i = 0; i < SHIP_NSPEC; ++i) {
    const double om = 2.25 + i * dom;
    const float omi = (float)om * scale1;
    const double o2 = (double)omi * (double)omi, o4 = o2 * o2;
    const float p4 = (float)o4, p5 = (float)(o4 * (double)omi);       // np.power(omi, 4), np.power(omi, 5)
    const float ex = (float)exp((double)__fdiv_rn(-b, p4));
    const float sf = __fdiv_rn(d * ex, p5);
    const double s2 = (double)sf * (double)sf;                         // np.power(s[i, :], 2) on the float64 row
    const double f1 = f2, d1 = d2;
    if (i < SHIP_NTAB) { f2 = tab[2 * i]; d2 = tab[2 * i + 1]; }
    else { f2 = 0.5; d2 = (4.0 * om) * 0.5; }                          // "interval 3"
    double wf = (0.5 * (f1 + f2)) * dom, wd = (0.5 * (d1 + d2)) * dom;
    if (i <= SHIP_NTAB) { wf = wf * (double)scale1; wd = wd * (double)scale1; }      // an interpolated array is among f1, f2: float64
    else { wf = (double)((float)wf * scale1); wd = (double)((float)wd * scale1); }   // Python floats times the float32 scale1
    F = F + wf * s2;
    B = B + wd * s2;
  }
  F = ((F * 1025) * 9.81) * (double)p.length;
  B = (B * 1025) * (double)sqrtf(9.81f * p.length);
  r.F_wave_b = F; r.beta2_b = B;

  // period factors (:290-296)
  if (r.Tm > 8.55f) { F = F * .66; B = B * .60; }
  if (r.Tm >= 5.7f && r.Tm <= 8.55f) {
    const float t = r.Tm - 5.7f;
    F = F * (double)(1.0f - __fdiv_rn(0.34f * t, 2.85f));
    B = B * (double)(1.0f - __fdiv_rn(0.4f * t, 2.85f));
  }
  r.F_wave = F; r.beta2 = B;

  // form drag, wave direction = wind or Stokes direction -+ 20 degrees by orientation (:299-317)
  r.beta1 = (512.5f * p.cd) * area_wet;
  const double offset = -40 * ((double)p.orientation - 0.5);
  const float dir = dir_from_stokes ? (float)atan2((double)e.sy, (double)e.sx) : (float)atan2((double)e.ywind, (double)e.xwind);
  r.wave_dir = offset * (3.141592653589793 / 180.0) + (double)dir;
  const double cw = cos(r.wave_dir), sw = sin(r.wave_dir);
  const double Fx = (double)r.F_wind_x + F * cw, Fy = (double)r.F_wind_y + F * sw;
  r.F_total = sqrt(Fx * Fx + Fy * Fy);

  // four passes for wave damping and form drag (:321-334)
  const double b1x2 = (double)(2.f * r.beta1), b1x4 = (double)(4.f * r.beta1);
  double uw_tot = 0.0, uw_dir = 0.0;
  for (int it = 0; it < 4; ++it) {
    const double f2x = (B * uw_tot) * cw, f2y = (B * uw_tot) * sw;
    uw_dir = atan2(Fy - f2y, Fx - f2x);
    const double bet2c = B * cos(r.wave_dir - uw_dir);
    uw_tot = -bet2c / b1x2 + sqrt(bet2c * bet2c + b1x4 * r.F_total) / b1x2;
  }
  r.uw_tot = uw_tot; r.uw_dir = uw_dir;
  r.vu = uw_tot * cos(uw_dir);
  r.vv = uw_tot * sin(uw_dir);
  return r;
}

#ifndef ODR_SHIP_HOST
struct ShipSlots { const float *length, *height, *draft, *beam, *cf, *cd, *orientation, *cls; };

// ShipDrift.update of every active element: update_positions with the float32 current, the forces, update_positions with the
// float64 drift velocity from where the first move ended, stranding by the land mask sampled at the start of the step
// REPORT (an instantiation of its own, so that the plain one keeps its registers): report[10][n] gets the float64 intermediates
// of ShipForces in its order, for the tests
template <bool REPORT>
__global__ __launch_bounds__(BLOCK) void k_ship_drift(PView p, ShipSlots S, const double *__restrict__ table, int n_classes, int hs_mode,
                                                    int tp_mode, int dir_from_stokes, int stranded_code, double dt,
                                                    double *__restrict__ report) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= p.n) return;
  ShipEnv e;
  e.u = p.env[VAR_U][i]; e.v = p.env[VAR_V][i]; e.xwind = p.env[VAR_XWIND][i]; e.ywind = p.env[VAR_YWIND][i];
  e.sx = dir_from_stokes ? p.env[VAR_SX][i] : 0.f; e.sy = dir_from_stokes ? p.env[VAR_SY][i] : 0.f;
  e.hs = hs_mode == 0 ? p.env[VAR_HS][i] : 0.f; e.tm = tp_mode == 0 ? p.env[VAR_TP][i] : 0.f;
  ShipProp s;
  s.length = S.length[i]; s.height = S.height[i]; s.draft = S.draft[i]; s.beam = S.beam[i]; s.cf = S.cf[i]; s.cd = S.cd[i];
  s.orientation = (int)S.orientation[i];
  int cls = (int)S.cls[i];
  cls = cls < 0 ? 0 : (cls >= n_classes ? n_classes - 1 : cls);      // (the binding has checked the range: never read outside the table)
  const int mv = p.moving[i];
  double lon = p.lon[i], lat = p.lat[i];
  move_f32(lon, lat, e.u, e.v, mv, dt);
  const ShipForces r = ship_forces(e, s, table + (size_t)cls * (2 * SHIP_NTAB), hs_mode, tp_mode, dir_from_stokes);
  move_f64(lon, lat, r.vu, r.vv, mv, dt);
  p.lon[i] = lon; p.lat[i] = lat;
  if constexpr (REPORT) {
    const double v[10] = {r.F_wave_b, r.beta2_b, r.F_wave, r.beta2, r.wave_dir, r.F_total, r.uw_tot, r.uw_dir, r.vu, r.vv};
#pragma unroll
    for (int k = 0; k < 10; ++k) report[(size_t)k * (size_t)p.n + (size_t)i] = v[k];
  }
  if (p.env[VAR_LAND][i] == 1.0f) {      // deactivate_elements(land_binary_mask == 1, reason='ship stranded') (:342)
    if (p.status[i] == 0) p.status[i] = stranded_code;
    p.moving[i] = 0;
  }
}
#endif  // ODR_SHIP_HOST

}  // namespace odr
