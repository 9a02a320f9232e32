// OpenBerg: iceberg drift.  Roll-over, and the momentum balance of every berg integrated over the time step with SciPy's RK45.
//
//   OpenBerg.roll_over                     models/openberg.py:587-614              berg_roll_over_f32
//   OpenBerg.advect_iceberg                models/openberg.py:427-552              berg_prepare, berg_rhs, berg_attempt
//   ocean_force .. coriolis_force          models/openberg.py:104-218              berg_prepare (the factors), berg_rhs
//   solve_ivp(method='RK45')               scipy/integrate/_ivp/rk.py, common.py   berg_attempt, berg_solve
//
// (Keghouche et al. 2010 for the forces, Wagner et al. 2017 for the stability criterion, Dormand & Prince 1980 / Hairer,
// Norsett & Wanner II.4 for the integrator.)
//
// Rounding contract.  The environment and the four dimensions are float32 arrays in the reference, the six coefficients float64
// arrays (seeded as scalars: elements/elements.py:219-222), Python constants are weak (NumPy 2): a product of float32 operands
// is ONE IEEE single operation, anything that meets a coefficient or the float64 velocity vector of solve_ivp is ONE IEEE double
// operation on the widened value, in the reference's order, without contraction (the library and the host build are compiled
// with -ffp-contract=off; nothing below may be fused).  Nothing but + - * / and sqrt (correctly rounded on both sides) runs per
// element, so the device and the host build agree bit for bit; sin(radians(lat)) of the Coriolis parameter is berg_sin below
// for that reason (within an ulp of libm's).  The sine and cosine of the wave direction are formed once per call on the host
// (berg_wave_direction_f32) by NumPy's own float32 routine, restated (berg_sincosf_numpy), as is the float32 Coriolis parameter of
// a run's first step.
//
// The solver is SciPy's over the flattened velocity vector of ALL active elements: one error norm over the 2N components
// controls the step size.  Per attempt every element evaluates the six stages in registers (berg_attempt) and a fixed-order
// reduction (berg_block_sum and k_berg_fold, the same order in the host build) forms the sum of the squared scaled errors:
// two runs give the same bits.  The control flow (berg_solve) is shared by the library and the host build.
//
// Compiled for the CPU by tests/berg_host.cpp: includes nothing (the includer provides <cmath>); the kernels (not part of the
// host build) take BLOCK from odr_kernels.hip.h, which the translation unit includes first.
#pragma once

namespace odr {

enum { BERG_SAIL = 0, BERG_DRAFT = 1, BERG_LENGTH = 2, BERG_WIDTH = 3, BERG_X_VELOCITY = 4, BERG_Y_VELOCITY = 5 };   // property slots of the model
enum { BERG_ICE_FREE = 0, BERG_ICE_DRAG = 1, BERG_ICE_LOCKED = 2, BERG_ICE_MASK = 3, BERG_GROUNDED = 4 };   // BergElem::cls
constexpr double BERG_RTOL = 1e-3, BERG_ATOL = 1e-6;     // solve_ivp's defaults
constexpr int BERG_MAX_ATTEMPTS = 10000;

struct BergCoef { double weight, water_form, water_skin, wind_form, wind_skin, wave_drag; };   // float64 arrays in the reference
struct BergEnv {      // the float32 environment of one element (advect_iceberg :440-449, :469-488)
  float u, v, sx, sy, xwind, ywind, depth, ssh, hs, ice_a, ice_u, ice_v;
};
struct BergCall {     // what is the same for every element of one call
  BergCoef k;
  float wave_sin, wave_cos;     // berg_wave_direction_f32
  float ice_thickness;
  int wave_rad, stokes, coriolis, grounding;
  int lat_f32;                  // elements.lat is a float32 array (until the first update_positions of a run, elements.py:71-88)
};
// what an attempt reads of one element
struct BergElem {
  double mass, drag_o, drag_a, wave_x, wave_y, mf, ice_c;   // mf = mass * 2 Omega sin(lat); ice_c = 0.5 * (rho_ice * csi * Ai)
  float wu, wv, au, av, iu, iv;                             // water (+ Stokes), wind and ice velocity
  int cls;
};

// sin(x) for |x| <= pi/2 (a latitude in radians), from + - * only: the kernels of fdlibm / musl (k_sin.c, k_cos.c) on
// [-pi/4, pi/4], the cosine of the complement outside.  Within an ulp of the correctly rounded value.
__host__ __device__ __forceinline__ double berg_sin(double x) {
  const double ax = x < 0 ? -x : x;
  if (ax <= 0.78539816339744830962) {
    const double z = x * x, v = z * x;
    const double r = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 +
                     z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    return x + v * (-1.66666666666666324348e-01 + z * r);
  }
  const double hi = 1.57079632679489655800e+00 - ax, lo = 6.12323399573676603587e-17;   // pi/2 - |x| = hi + lo
  const double z = hi * hi, w = z * z;
  const double r = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                   (w * w) * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
  const double hz = 0.5 * z, c1 = 1.0 - hz;
  const double cc = c1 + (((1.0 - c1) - hz) + (z * r - hi * lo));     // cos(hi + lo), musl's __cos(x, y)
  return x < 0 ? -cc : cc;
}

// np.sin / np.cos of a float32 ARRAY, bit for bit: NumPy's float32 routine is not correctly rounded (it differs from the rounded
// float64 value for 5 % of the arguments), and the reference's Coriolis parameter of the first step and its wave direction go
// through it.  This is the routine of NumPy's SIMD loops (umath/loops_trigonometric, x86 with FMA, |x| < 71476): the quadrant from
// x * 2/pi rounded to nearest, a three-term Cody-Waite reduction and two polynomials, every multiply-add FUSED.  Compared with
// NumPy 2.2 on two million arguments in [-7, 7] by tests/test_berg_device_arithmetic.py: identical.  NumPy takes this route only
// where it dispatches to a SIMD loop with fused multiply-add (x86 AVX2 + FMA3 or AVX-512, the machines the golden was made on);
// on a CPU without FMA its float32 sine is another routine and the reference itself gives other bits there.
__host__ __device__ __forceinline__ void berg_sincosf_numpy(float x, float &sn, float &cs) {
  float q = x * 0x1.45f306p-1f;
  q = (q + 0x1.8p23f) - 0x1.8p23f;
  float r = fmaf(q, -0x1.921fb0p+00f, x);
  r = fmaf(q, -0x1.5110b4p-22f, r);
  r = fmaf(q, -0x1.846988p-48f, r);
  const float r2 = r * r;
  const float c = fmaf(fmaf(fmaf(fmaf(0x1.98e616p-16f, r2, -0x1.6c06dcp-10f), r2, 0x1.55553cp-05f), r2, -0x1p-1f), r2, 1.0f);
  float s = fmaf(fmaf(fmaf(0x1.7d3bbcp-19f, r2, -0x1.a06bbap-13f), r2, 0x1.11119ap-07f), r2, -0x1.555556p-03f);
  s = fmaf(s * r2, r, r);
  const int iq = (int)q, ic = iq + 1;
  sn = (iq & 1) ? c : s;
  if (iq & 2) sn = -sn;
  cs = (ic & 1) ? c : s;
  if (ic & 2) cs = -cs;
}

// roll_over (:587-614) of one element.  L, W, H are float32 arrays; crit is a NumPy float64 scalar (np.sqrt of a Python float),
// which is NOT weak: W / H is compared in float64.  alpha meets the float32 H as a Python float: cast to float32.
__host__ __device__ __forceinline__ void berg_roll_over_f32(float &length, float &width, float &sail, float &draft) {
  const double alpha = 900.0 / 1027.0;                       // rho_iceb / rho_water
  const double crit = sqrt(6 * alpha * (1 - alpha));
  float H = draft + sail;
  float W = length < width ? length : width, L = length < width ? width : length;     // np.min / np.max([L, W], axis=0)
  if ((double)__fdiv_rn(W, H) < crit) {
    const float nL = L > H ? L : H, nW = L > H ? H : L, nH = W;
    L = nL; W = nW; H = nH;
  }
  const float depthib = H * (float)alpha;
  length = L; width = W; sail = H - depthib; draft = depthib;
}

// (sea_surface_wave_from_direction + 180) % 360 (:446), np.sin / np.cos(np.deg2rad(.)) (:158-159) of the float32 value
inline void berg_wave_direction_f32(double from_direction, float &s, float &c) {
  const float a = (float)from_direction + 180.f;
  float r = fmodf(a, 360.f);
  if (r != 0.f && r < 0.f) r += 360.f;                        // np.remainder: the sign of the divisor
  const float rad = r * (3.14159274101257324f / 180.0f);
  berg_sincosf_numpy(rad, s, c);
}

// advect_iceberg up to the call of solve_ivp (:450-535) for one element: the factors of the forces, V0, the grounded flag and
// `moving` after grounding and degrounding.  lat in degrees (float64, like elements.lat).
__host__ __device__ __forceinline__ BergElem berg_prepare(const BergCall &C, const BergEnv &e, double lat, float sail, float draft, float length,
                                                          float width, int &moving, double &v0x, double &v0y) {
  BergElem E;
  const float Avo = length * draft, Aho = width * length, Ava = length * sail, Aha = width * length;
  const float Ai = C.ice_thickness * length;
  // mass = width * (Ava + Avo) * rho_iceb * weight_coef: float32 up to the float64 coefficient
  E.mass = (double)((width * (Ava + Avo)) * 900.f) * C.k.weight;
  const double k = ((1.293 * C.k.wind_form) * (double)Ava) / ((1027.0 * C.k.water_form) * (double)Avo);
  const double sk = sqrt(k), f = sk / (1 + sk);
  E.drag_o = ((513.5 * C.k.water_form) * (double)Avo) + ((1027.0 * C.k.water_skin) * (double)Aho);
  E.drag_a = (((0.5 * 1.293) * C.k.wind_form) * (double)Ava) + ((1.293 * C.k.wind_skin) * (double)Aha);
  // 0.25 * rho_water * wave_drag_coef * g * iceb_length * (wave_height / 2) ** 2 * np.sin(np.deg2rad(wave_direction))
  const float hh = e.hs / 2.f;
  const double w = (((256.75 * C.k.wave_drag) * 9.81) * (double)length) * (double)(hh * hh);
  E.wave_x = C.wave_rad ? w * (double)C.wave_sin : 0.0;
  E.wave_y = C.wave_rad ? w * (double)C.wave_cos : 0.0;
  // f = 2 * omega * np.sin(np.radians(lat)): float32 throughout while lat is a float32 array
  double f2;
  if (C.lat_f32) {
    const float rad = (float)lat * (3.14159274101257324f / 180.0f);
    float s, c;
    berg_sincosf_numpy(rad, s, c);
    f2 = (double)((float)(2 * 7.2921e-5) * s);
  } else f2 = (2 * 7.2921e-5) * berg_sin(lat * (3.14159265358979323846 / 180.0));
  E.mf = C.coriolis ? E.mass * f2 : 0.0;
  E.ice_c = (double)(0.5f * (917.f * Ai));
  E.wu = e.u + (C.stokes ? e.sx : 0.f);
  E.wv = e.v + (C.stokes ? e.sy : 0.f);
  E.au = e.xwind; E.av = e.ywind; E.iu = e.ice_u; E.iv = e.ice_v;
  E.cls = e.ice_a >= 0.9f ? BERG_ICE_LOCKED : (e.ice_a <= 0.15f ? BERG_ICE_FREE : BERG_ICE_DRAG);
  // V0 = (1 - f) * water + f * wind; the sea-ice velocity where the concentration is >= 0.9
  v0x = (1 - f) * (double)E.wu + f * (double)E.au;
  v0y = (1 - f) * (double)E.wv + f * (double)E.av;
  if (E.cls == BERG_ICE_LOCKED) { v0x = (double)E.iu; v0y = (double)E.iv; }
  const float hwall = draft - (e.depth + e.ssh);
  if (C.grounding) {
    if (hwall >= 0.f) { E.cls |= BERG_GROUNDED; moving = 0; }
    if (moving == 0 && hwall < 0.f) moving = 1;
  }
  return E;
}

// dynamic (:491-511): the acceleration of one element at the velocity (vx, vy)
__host__ __device__ __forceinline__ void berg_rhs(const BergElem &E, double vx, double vy, double &ax, double &ay) {
  const double ox = (double)E.wu - vx, oy = (double)E.wv - vy;
  const double on = sqrt(ox * ox + oy * oy);
  const double wx = (double)E.au - vx, wy = (double)E.av - vy;
  const double wn = sqrt(wx * wx + wy * wy);
  // ocean + wind + wave radiation + Coriolis (+ a sea surface slope term that is identically 0)
  const double sx = (((E.drag_o * on) * ox + (E.drag_a * wn) * wx) + E.wave_x) + E.mf * vy;
  const double sy = (((E.drag_o * on) * oy + (E.drag_a * wn) * wy) + E.wave_y) + (-E.mf) * vx;
  double fx = 0.0, fy = 0.0;
  const int cls = E.cls & BERG_ICE_MASK;
  if (cls == BERG_ICE_LOCKED) { fx = -sx; fy = -sy; }
  else if (cls == BERG_ICE_DRAG) {
    const double ix = (double)E.iu - vx, iy = (double)E.iv - vy;
    const double d = sqrt(ix * ix + iy * iy);
    fx = (E.ice_c * d) * ix;
    fy = (E.ice_c * d) * iy;
  }
  ax = (sx + fx) / E.mass;
  ay = (sy + fy) / E.mass;
}

// y / scale or f / scale of select_initial_step (common.py): the element's share of the squared norm
__host__ __device__ __forceinline__ double berg_scaled_sq(double ax, double ay, double y0x, double y0y) {
  const double qx = ax / (BERG_ATOL + fabs(y0x) * BERG_RTOL), qy = ay / (BERG_ATOL + fabs(y0y) * BERG_RTOL);
  return qx * qx + qy * qy;
}

// f1 = fun(t0 + h0, y0 + h0 * f0) of select_initial_step: returns the share of |(f1 - f0) / scale|^2
__host__ __device__ __forceinline__ double berg_probe(const BergElem &E, double h0, double yx, double yy, double fx, double fy) {
  double gx, gy;
  berg_rhs(E, yx + h0 * fx, yy + h0 * fy, gx, gy);
  return berg_scaled_sq(gx - fx, gy - fy, yx, yy);
}

// rk_step and _estimate_error_norm of one Dormand-Prince attempt (rk.py): y, f = fun(y) in (the FSAL derivative); y_new, f_new out;
// returns the element's share of |error / scale|^2.  np.dot(K[:s].T, a[:s]) is summed in ascending stage order; the terms of
// the zero coefficients (B[1], E[1]) are left out (they add +-0).
__host__ __device__ __forceinline__ double berg_attempt(const BergElem &E, double h, double yx, double yy, double k0x, double k0y, double &nx,
                                                        double &ny, double &k6x, double &k6y) {
  double k1x, k1y, k2x, k2y, k3x, k3y, k4x, k4y, k5x, k5y;
  berg_rhs(E, yx + (k0x * (1.0 / 5)) * h, yy + (k0y * (1.0 / 5)) * h, k1x, k1y);
  berg_rhs(E, yx + (k0x * (3.0 / 40) + k1x * (9.0 / 40)) * h, yy + (k0y * (3.0 / 40) + k1y * (9.0 / 40)) * h, k2x, k2y);
  berg_rhs(E, yx + ((k0x * (44.0 / 45) + k1x * (-56.0 / 15)) + k2x * (32.0 / 9)) * h,
           yy + ((k0y * (44.0 / 45) + k1y * (-56.0 / 15)) + k2y * (32.0 / 9)) * h, k3x, k3y);
  berg_rhs(E, yx + (((k0x * (19372.0 / 6561) + k1x * (-25360.0 / 2187)) + k2x * (64448.0 / 6561)) + k3x * (-212.0 / 729)) * h,
           yy + (((k0y * (19372.0 / 6561) + k1y * (-25360.0 / 2187)) + k2y * (64448.0 / 6561)) + k3y * (-212.0 / 729)) * h, k4x, k4y);
  berg_rhs(E, yx + ((((k0x * (9017.0 / 3168) + k1x * (-355.0 / 33)) + k2x * (46732.0 / 5247)) + k3x * (49.0 / 176)) + k4x * (-5103.0 / 18656)) * h,
           yy + ((((k0y * (9017.0 / 3168) + k1y * (-355.0 / 33)) + k2y * (46732.0 / 5247)) + k3y * (49.0 / 176)) + k4y * (-5103.0 / 18656)) * h, k5x, k5y);
  nx = yx + h * ((((k0x * (35.0 / 384) + k2x * (500.0 / 1113)) + k3x * (125.0 / 192)) + k4x * (-2187.0 / 6784)) + k5x * (11.0 / 84));
  ny = yy + h * ((((k0y * (35.0 / 384) + k2y * (500.0 / 1113)) + k3y * (125.0 / 192)) + k4y * (-2187.0 / 6784)) + k5y * (11.0 / 84));
  berg_rhs(E, nx, ny, k6x, k6y);
  const double ex = (((((k0x * (-71.0 / 57600) + k2x * (71.0 / 16695)) + k3x * (-71.0 / 1920)) + k4x * (17253.0 / 339200)) + k5x * (-22.0 / 525)) + k6x * (1.0 / 40)) * h;
  const double ey = (((((k0y * (-71.0 / 57600) + k2y * (71.0 / 16695)) + k3y * (-71.0 / 1920)) + k4y * (17253.0 / 339200)) + k5y * (-22.0 / 525)) + k6y * (1.0 / 40)) * h;
  const double qx = ex / (BERG_ATOL + fmax(fabs(yx), fabs(nx)) * BERG_RTOL), qy = ey / (BERG_ATOL + fmax(fabs(yy), fabs(ny)) * BERG_RTOL);
  return qx * qx + qy * qy;
}

// ---- the control flow of RK45 (rk.py: RungeKutta.__init__, _step_impl; common.py: select_initial_step; ivp.py: the loop of
// solve_ivp) over a backend B that evaluates all elements and returns sums of squares in a fixed order:
//   int norms0(double s[2])            sum (y0 / scale)^2, sum (f0 / scale)^2       (f0 = fun(y0), formed by the prepare step)
//   int probe(double h0, double &s)    sum ((fun(y0 + h0 f0) - f0) / scale)^2
//   int attempt(double h, double &s)   one Dormand-Prince attempt from (y, f) into (y_new, f_new): sum (error / scale)^2
//   void accept()                      (y, f) <- (y_new, f_new)
// each returning 0 or an error code that is handed on.  first_step, max_step, rtol and atol are SciPy's defaults.
enum { BERG_SOLVE_OK = 0, BERG_SOLVE_NOT_FINITE = 1, BERG_SOLVE_STEP_TOO_SMALL = 2, BERG_SOLVE_TOO_MANY = 3 };
struct BergSolveStat { int attempts, rejected, why; double t, h, norm; };

template <class B>
int berg_solve(B &be, long long n, double t_end, BergSolveStat &st) {
  st.attempts = st.rejected = 0; st.why = BERG_SOLVE_OK; st.t = 0; st.h = 0; st.norm = 0;
  if (n <= 0 || !(t_end > 0)) return 0;
  const double rms = pow((double)(2 * n), 0.5);          // norm(x) = np.linalg.norm(x) / x.size ** 0.5
  double s[2], s2;
  if (int rc = be.norms0(s)) return rc;
  const double d0 = sqrt(s[0]) / rms, d1 = sqrt(s[1]) / rms;
  st.norm = d1;
  if (!isfinite(d0) || !isfinite(d1)) { st.why = BERG_SOLVE_NOT_FINITE; return 0; }
  double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  if (t_end < h0) h0 = t_end;
  if (int rc = be.probe(h0, s2)) return rc;
  const double d2 = (sqrt(s2) / rms) / h0;
  st.norm = d2;
  if (!isfinite(d2)) { st.why = BERG_SOLVE_NOT_FINITE; return 0; }
  const double dm = d1 > d2 ? d1 : d2;
  const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? (1e-6 > h0 * 1e-3 ? 1e-6 : h0 * 1e-3) : pow(0.01 / dm, 1.0 / 5);
  double h_abs = 100 * h0;
  if (h1 < h_abs) h_abs = h1;
  if (t_end < h_abs) h_abs = t_end;
  double t = 0;
  while (t < t_end) {                                     // solver.step() until t reaches t_bound
    const double min_step = 10 * fabs(nextafter(t, INFINITY) - t);
    if (h_abs < min_step) h_abs = min_step;
    bool rejected = false;
    double t_new;
    for (;;) {
      st.t = t; st.h = h_abs;
      if (h_abs < min_step) { st.why = BERG_SOLVE_STEP_TOO_SMALL; return 0; }
      if (st.attempts >= BERG_MAX_ATTEMPTS) { st.why = BERG_SOLVE_TOO_MANY; return 0; }
      ++st.attempts;
      t_new = t + h_abs;
      if (t_new - t_end > 0) t_new = t_end;
      const double h = t_new - t;
      h_abs = fabs(h);
      if (int rc = be.attempt(h, s2)) return rc;
      const double err = sqrt(s2) / rms;
      st.norm = err;
      if (!isfinite(err)) { st.why = BERG_SOLVE_NOT_FINITE; return 0; }
      const double g = err == 0 ? 10.0 : 0.9 * pow(err, -0.2);
      if (err < 1) {
        double factor = g < 10.0 ? g : 10.0;
        if (rejected && factor > 1) factor = 1;
        h_abs *= factor;
        break;
      }
      h_abs *= g > 0.2 ? g : 0.2;
      rejected = true;
      ++st.rejected;
    }
    be.accept();
    t = t_new;
  }
  return 0;
}

// ---- the fixed-order sum.  Within a wave of 64 lanes: six exchange steps at lane distances 32, 16, 8, 4, 2, 1 (every lane adds
// its partner's value: both form the same sum).  Within a workgroup: the wave sums in ascending wave order.  Over the
// workgroups: BLOCK running sums over the partials j = t, t + BLOCK, ... in ascending j, then the workgroup sum of those.
// berg_block_sum_host and berg_fold_host are the same additions on the CPU.
inline double berg_block_sum_host(const double *v, int block) {
  double total = 0;
  for (int w0 = 0; w0 < block; w0 += 64) {
    double a[64], b[64];
    for (int l = 0; l < 64; ++l) a[l] = v[w0 + l];
    for (int off = 32; off; off >>= 1) {
      for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ off];
      for (int l = 0; l < 64; ++l) a[l] = b[l];
    }
    total = w0 == 0 ? a[0] : total + a[0];
  }
  return total;
}
inline double berg_fold_host(const double *part, long long nb, int block) {
  double run[1024];
  for (int t = 0; t < block; ++t) {
    double s = 0;
    for (long long j = t; j < nb; j += block) s = s + part[j];
    run[t] = s;
  }
  return berg_block_sum_host(run, block);
}

#ifndef ODR_BERG_HOST
static_assert(BLOCK % 64 == 0 && BLOCK <= 1024, "berg_block_sum: whole waves");

__device__ __forceinline__ double berg_block_sum(double v, double *lds) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int w = 1; w < BLOCK / 64; ++w) t = t + lds[w];
  return t;
}

// The scratch of one call, structure of arrays over the n active elements (odr_berg.hip lays it out)
struct BergScratch {
  double *mass, *drag_o, *drag_a, *wave_x, *wave_y, *mf, *ice_c;
  float *wu, *wv, *au, *av, *iu, *iv;
  int *cls;
  double *part;      // [2][number of workgroups]
  double *sum;       // [2]
};
struct BergState { double *yx, *yy, *fx, *fy; };

__device__ __forceinline__ BergElem berg_load(const BergScratch &S, long long i) {
  BergElem E;
  E.mass = S.mass[i]; E.drag_o = S.drag_o[i]; E.drag_a = S.drag_a[i]; E.wave_x = S.wave_x[i]; E.wave_y = S.wave_y[i];
  E.mf = S.mf[i]; E.ice_c = S.ice_c[i];
  E.wu = S.wu[i]; E.wv = S.wv[i]; E.au = S.au[i]; E.av = S.av[i]; E.iu = S.iu[i]; E.iv = S.iv[i];
  E.cls = S.cls[i];
  return E;
}

// roll_over: one element per thread, four slots in, four slots out
__global__ __launch_bounds__(BLOCK) void k_berg_roll_over(long long n, float *__restrict__ sail, float *__restrict__ draft,
                                                        float *__restrict__ length, float *__restrict__ width) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  float L = length[i], W = width[i], s = sail[i], d = draft[i];
  berg_roll_over_f32(L, W, s, d);
  length[i] = L; width[i] = W; sail[i] = s; draft[i] = d;
}

// the environment arrays of a call; a variable that was not sampled (NULL) holds the reference's fallback
struct BergEnvPtr { const float *u, *v, *sx, *sy, *xwind, *ywind, *depth, *ssh, *hs, *ice_a, *ice_u, *ice_v; };

// Prepare: the per-element factors, V0 and f0 = fun(V0) into the scratch, grounding and degrounding into `moving`, and the
// workgroup's shares of |y0 / scale|^2 and |f0 / scale|^2
__global__ __launch_bounds__(BLOCK) void k_berg_prepare(long long n, BergCall C, BergEnvPtr e, const double *__restrict__ lat,
                                                      const float *__restrict__ sail, const float *__restrict__ draft,
                                                      const float *__restrict__ length, const float *__restrict__ width,
                                                      int *__restrict__ moving, BergScratch S, BergState y) {
  __shared__ double lds[2][BLOCK / 64];
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  double s0 = 0, s1 = 0;
  if (i < n) {
    BergEnv v;
    v.u = e.u[i]; v.v = e.v[i]; v.xwind = e.xwind[i]; v.ywind = e.ywind[i];
    v.sx = e.sx ? e.sx[i] : 0.f; v.sy = e.sy ? e.sy[i] : 0.f;
    v.depth = e.depth ? e.depth[i] : 10000.f; v.ssh = e.ssh ? e.ssh[i] : 0.f; v.hs = e.hs ? e.hs[i] : 0.f;
    v.ice_a = e.ice_a ? e.ice_a[i] : 0.f; v.ice_u = e.ice_u ? e.ice_u[i] : 0.f; v.ice_v = e.ice_v ? e.ice_v[i] : 0.f;
    int mv = moving[i];
    const int mv0 = mv;
    double v0x, v0y, fx, fy;
    const BergElem E = berg_prepare(C, v, lat[i], sail[i], draft[i], length[i], width[i], mv, v0x, v0y);
    if (mv != mv0) moving[i] = mv;
    berg_rhs(E, v0x, v0y, fx, fy);
    S.mass[i] = E.mass; S.drag_o[i] = E.drag_o; S.drag_a[i] = E.drag_a; S.wave_x[i] = E.wave_x; S.wave_y[i] = E.wave_y;
    S.mf[i] = E.mf; S.ice_c[i] = E.ice_c;
    S.wu[i] = E.wu; S.wv[i] = E.wv; S.au[i] = E.au; S.av[i] = E.av; S.iu[i] = E.iu; S.iv[i] = E.iv;
    S.cls[i] = E.cls;
    y.yx[i] = v0x; y.yy[i] = v0y; y.fx[i] = fx; y.fy[i] = fy;
    s0 = berg_scaled_sq(v0x, v0y, v0x, v0y);
    s1 = berg_scaled_sq(fx, fy, v0x, v0y);
  }
  s0 = berg_block_sum(s0, lds[0]);
  s1 = berg_block_sum(s1, lds[1]);
  if (threadIdx.x == 0) { S.part[blockIdx.x] = s0; S.part[gridDim.x + blockIdx.x] = s1; }
}

__global__ __launch_bounds__(BLOCK) void k_berg_probe(long long n, double h0, BergScratch S, BergState y) {
  __shared__ double lds[BLOCK / 64];
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  double s = 0;
  if (i < n) s = berg_probe(berg_load(S, i), h0, y.yx[i], y.yy[i], y.fx[i], y.fy[i]);
  s = berg_block_sum(s, lds);
  if (threadIdx.x == 0) S.part[blockIdx.x] = s;
}

// One attempt: the six stages of every element in registers.  116 bytes read and 32 written per element.
__global__ __launch_bounds__(BLOCK) void k_berg_attempt(long long n, double h, BergScratch S, BergState y, BergState o) {
  __shared__ double lds[BLOCK / 64];
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  double s = 0;
  if (i < n) {
    double nx, ny, gx, gy;
    s = berg_attempt(berg_load(S, i), h, y.yx[i], y.yy[i], y.fx[i], y.fy[i], nx, ny, gx, gy);
    o.yx[i] = nx; o.yy[i] = ny; o.fx[i] = gx; o.fy[i] = gy;
  }
  s = berg_block_sum(s, lds);
  if (threadIdx.x == 0) S.part[blockIdx.x] = s;
}

// sum[a] <- the partials of array a (blockIdx.x = a) in the fixed order above
__global__ __launch_bounds__(BLOCK) void k_berg_fold(const double *__restrict__ part, long long nb, double *__restrict__ sum) {
  __shared__ double lds[BLOCK / 64];
  const double *p = part + (long long)blockIdx.x * nb;
  double s = 0;
  for (long long j = threadIdx.x; j < nb; j += BLOCK) s = s + p[j];
  s = berg_block_sum(s, lds);
  if (threadIdx.x == 0) sum[blockIdx.x] = s;
}

// Finish: grounded elements stand still; update_positions (basemodel/__init__.py:4631-4657) with the float64 velocities;
// iceb_x_velocity / iceb_y_velocity rounded to float32 once
__global__ __launch_bounds__(BLOCK) void k_berg_finish(PView p, double dt, const int *__restrict__ cls, BergState y, float *__restrict__ xvel,
                                                     float *__restrict__ yvel) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= p.n) return;
  double vx = y.yx[i], vy = y.yy[i];
  if (cls[i] & BERG_GROUNDED) { vx = 0.0; vy = 0.0; }
  double lon = p.lon[i], lat = p.lat[i];
  move_f64(lon, lat, vx, vy, p.moving[i], dt);
  p.lon[i] = lon; p.lat[i] = lat;
  y.yx[i] = vx; y.yy[i] = vy;      // (what odr_berg_advect reports as velocity_f64)
  xvel[i] = (float)vx; yvel[i] = (float)vy;
}
#endif  // ODR_BERG_HOST

}  // namespace odr
