// OpenOil: the NOAA oil weathering of one element and one step, from a table of pseudo-components.
//
//   OpenOil.oil_weathering_noaa                 models/openoil/openoil.py:717-790      weather_properties, weather_element
//   OpenOil.evaporation_noaa                    :822-853                               weather_element (WEATHER_EVAPORATION)
//   noaa.evap_decay_constant / mass_transport_coeff   models/openoil/noaa_oil_weathering.py:10-33   weather_mass_transport_f32
//   OpendriftOil.vapor_pressure                 models/openoil/adios/oil.py:143-169    weather_element (constants: WC_*)
//   OpenOil.emulsification_noaa                 :855-920                               weather_starts_emulsion, weather_sintef_f32, weather_element
//   OpenOil.disperse_noaa                       :792-815                               weather_dispersed_fraction
//   PhysicsMethods.wind_speed .. sea_surface_wave_breaking_fraction   models/physics_methods.py:885-966   weather_wind_speed_f32, weather_hs_f32, weather_period_f32
//   OpenOil.biodegradation_half_time / _adcroft :568-611                               weather_biodegraded_fraction
//
// Rounding contract.  The reference's element arrays are float64 when oil_weathering_noaa runs (the Oil element type declares
// them float32, but the arrays released into a run are float64; tools/gen_golden_openoil_weathering.py asserts it in front of and
// behind every step, also behind a continuous release), the environment is float32.  NumPy 2 keeps an expression of a float32
// array and Python floats in float32, so these chains are float32 here: the Kelvin conversion, wind speed, the mass transport
// coefficient (powf), gas_constant * T, the water uptake coefficient and k_emul * dt, T - 273.15 and the SINTEF weights, the
// wave height from the wind, the wave period and the breaking fraction, Adcroft's tau and fraction (powf, expf).  Everything
// that touches an element variable, the oil's two property curves (evaluated in float64 by definition),
// the vapour pressure (temp - C_2i is float32 scalar minus float64 array) and mass_components is float64.  np.sum over the
// components of a row adds in NumPy's pairwise order (weather_np_sum).  exp, pow, expf and powf are the platform's: they agree
// with NumPy's to an ulp or two, not bit for bit.
//
// Compiled for the CPU by tests/weather_host.cpp (the float rounding intrinsics are its own there): includes nothing.
#pragma once

namespace odr {

constexpr int OIL_MAXCOMP = 32;       // ODR_OIL_MAXCOMP
enum { WEATHER_PROPERTIES = 1, WEATHER_EVAPORATION = 2, WEATHER_EMULSIFICATION = 4, WEATHER_DISPERSION = 8,
       WEATHER_BIO_HALF_TIME = 16, WEATHER_BIO_ADCROFT = 32 };      // ODR_WEATHER_*
// one element's record of the side table, by element ID
enum { WS_MASS_OIL = 0, WS_MASS_EVAPORATED, WS_MASS_DISPERSED, WS_MASS_BIODEGRADED, WS_FRACTION_EVAPORATED, WS_WATER_FRACTION,
       WS_INTERFACIAL_AREA, WS_DENSITY, WS_VISCOSITY, WS_BULLTIME, WS_HALF_TIME_DROPLET, WS_HALF_TIME_SLICK, WS_FILM, WS_PAD,
       WS_N = 14 };
// what the reduction in front of a step leaves on the device (k_weather_reduce)
enum { WR_NSURF = 0,       // elements with z == 0
       WR_MIN_AGE_SURF,    // the youngest of them (:831)
       WR_MIN_YDIFF,       // min(Y_max - max_water_fraction_sintef) over the elements that start to emulsify (:888)
       WR_HS_MAX, WR_TP_MAX, WR_TP_MIN, WR_TP_SUM, WR_TP_CNT,    // provenance of wave height and period; sum and count of the periods > 0
       WR_N = 8 };

struct WeatherOil {       // launch argument
  int ncomp, stride;      // stride: ncomp rounded up to an even count (rows start on 16 bytes)
  int mwf_n, pad;         // entries of max_water_fraction: 0, 1 or 2
  double rho_ref, rho_k, rho_T, nu_ref, nu_B, nu_T;     // rho(T) = rho_ref - k (T - T_ref), nu(T) = nu_ref exp(B/T - B/T_ref)
  double bulltime, bullwinkle, y_max;
  double mwf_t[2], mwf_w[2];
  double rho_w;           // PhysicsMethods.sea_water_density() (T = 10, S = 35)
};
// per-component constants, formed on the host with the reference's NumPy expressions: [4][OIL_MAXCOMP]
enum { WC_A = 0,     // D_S * (bp - C_2i)**2 / (D_Zb * R_cal * bp)
       WC_C = 1,     // C_2i = 0.19 bp - 18
       WC_INV = 2,   // 1 / (bp - C_2i)
       WC_MW = 3 };  // molecular_weight / 1000.
struct WeatherIn {        // what one element brings besides its record and its row
  float xwind, ywind, temp, hs, tp;
  double z, age;
};

__device__ __forceinline__ float weather_wind_speed_f32(float x, float y) { return sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y))); }
// sea_water_temperature[sea_water_temperature < 100] += 273.15 on the float32 environment (:723-724)
__device__ __forceinline__ float weather_kelvin_f32(float T) { return T < 100.f ? __fadd_rn(T, (float)273.15) : T; }
// significant_wave_height (physics_methods.py:893-906): the sampled one when any is > 0, else WMO 1998 from the wind in float32
__device__ __forceinline__ float weather_hs_f32(const double *R, float hs, float ws) {
  return R[WR_HS_MAX] > 0 ? hs : __fmul_rn((float)0.0246, __fmul_rn(ws, ws));
}
// wave_period (physics_methods.py:918-943): the sampled peak period when any is > 0, a zero replaced by the mean of the others;
// else Pierson-Moskowitz from the wind, as read back from the float32 environment (:876-883, :908-916)
__device__ __forceinline__ float weather_period_f32(const double *R, float tp, float ws) {
  if (R[WR_TP_MAX] > 0) return tp == 0.f ? (float)(R[WR_TP_SUM] / R[WR_TP_CNT]) : tp;
  double omega = 5;
  if (ws > 0) omega = (double)__fdiv_rn((float)(0.877 * 9.81), __fmul_rn((float)1.17, ws));
  return (float)((2 * 3.141592653589793) / omega);
}
__device__ __forceinline__ float weather_breaking_fraction_f32(float ws, float T) {
  const float f = __fdiv_rn(__fmul_rn((float)0.032, __fsub_rn(ws, 5.f)), T);
  return f < 0.f ? 0.f : f;
}
// noaa.mass_transport_coeff
__device__ __forceinline__ float weather_mass_transport_f32(float ws) {
  if (ws >= 10.f) return __fmul_rn((float)(0.06 * 0.0025), __fmul_rn(ws, ws));
  return __fmul_rn((float)0.0025, powf(ws, (float)0.78));
}

// np.add.reduce over n contiguous float64 values: fewer than eight in a plain loop, else eight partial sums folded pairwise and
// the remainder added one by one (n <= 128: one block of NumPy's pairwise sum)
template <class F>
__device__ __forceinline__ double weather_np_sum(int n, F term) {
  if (n < 8) {
    double res = 0.;
    for (int i = 0; i < n; ++i) res = res + term(i);
    return res;
  }
  double r0 = term(0), r1 = term(1), r2 = term(2), r3 = term(3), r4 = term(4), r5 = term(5), r6 = term(6), r7 = term(7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 = r0 + term(i); r1 = r1 + term(i + 1); r2 = r2 + term(i + 2); r3 = r3 + term(i + 3);
    r4 = r4 + term(i + 4); r5 = r5 + term(i + 5); r6 = r6 + term(i + 6); r7 = r7 + term(i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res = res + term(i);
  return res;
}
// two such sums over terms that are formed together
struct WeatherPair { double a, b; };
template <class F>
__device__ __forceinline__ WeatherPair weather_np_sum2(int n, F term) {
  WeatherPair s = {0., 0.};
  if (n < 8) {
    for (int i = 0; i < n; ++i) { const WeatherPair t = term(i); s.a = s.a + t.a; s.b = s.b + t.b; }
    return s;
  }
  WeatherPair r0 = term(0), r1 = term(1), r2 = term(2), r3 = term(3), r4 = term(4), r5 = term(5), r6 = term(6), r7 = term(7);
  int i = 8;
#define ODR_WADD(r, k) { const WeatherPair t = term(k); r.a = r.a + t.a; r.b = r.b + t.b; }
  for (; i < n - (n % 8); i += 8) {
    ODR_WADD(r0, i) ODR_WADD(r1, i + 1) ODR_WADD(r2, i + 2) ODR_WADD(r3, i + 3)
    ODR_WADD(r4, i + 4) ODR_WADD(r5, i + 5) ODR_WADD(r6, i + 6) ODR_WADD(r7, i + 7)
  }
  s.a = ((r0.a + r1.a) + (r2.a + r3.a)) + ((r4.a + r5.a) + (r6.a + r7.a));
  s.b = ((r0.b + r1.b) + (r2.b + r3.b)) + ((r4.b + r5.b) + (r6.b + r7.b));
  for (; i < n; ++i) ODR_WADD(s, i)
#undef ODR_WADD
  return s;
}

// the emulsion's density and viscosity and the evaporated fraction from the state in front of the step (:741-759).  Tk: Kelvin
__device__ __forceinline__ void weather_properties(const WeatherOil &O, float Tk, double *s) {
  const double T = (double)Tk;
  const double oil_density = O.rho_ref - O.rho_k * (T - O.rho_T);
  const double oil_viscosity = O.nu_ref * exp(O.nu_B / T - O.nu_B / O.nu_T);
  const double wf = s[WS_WATER_FRACTION];
  s[WS_DENSITY] = wf * O.rho_w + (1 - wf) * oil_density;
  const double fw_d_fref = wf / 0.84;
  double kv1 = sqrt(oil_viscosity) * 1.5e3;
  if (kv1 < 1) kv1 = 1;
  if (kv1 > 10) kv1 = 10;
  const double fe = s[WS_MASS_EVAPORATED] / (s[WS_MASS_OIL] + s[WS_MASS_EVAPORATED]);
  s[WS_FRACTION_EVAPORATED] = fe;
  s[WS_VISCOSITY] = oil_viscosity * exp(kv1 * fe) * pow(1 + (fw_d_fref / (1.187 - fw_d_fref)), 2.49);
}

// start_emulsion (:866-869)
__device__ __forceinline__ bool weather_starts_emulsion(const WeatherOil &O, double age, double fraction_evaporated) {
  return (age >= O.bulltime && O.bulltime >= 0) || (fraction_evaporated >= O.bullwinkle && O.bullwinkle > 0);
}
// max_water_fraction_sintef of one element (:877-886), float32.  One entry: that value (the reference's two masks would leave
// nothing else; its own code stops on the difference of two lists there)
__device__ __forceinline__ float weather_sintef_f32(const WeatherOil &O, float Tk) {
  if (O.mwf_n == 1) return (float)O.mwf_w[0];
  const float swt = __fsub_rn(Tk, (float)273.15);
  float w = __fdiv_rn(__fsub_rn((float)O.mwf_t[1], swt), (float)(O.mwf_t[1] - O.mwf_t[0]));
  if (swt > (float)O.mwf_t[1]) w = 0.f;
  if (swt <= (float)O.mwf_t[0]) w = 1.f;
  return __fadd_rn(__fmul_rn(w, (float)O.mwf_w[0]), __fmul_rn(__fsub_rn(1.f, w), (float)O.mwf_w[1]));
}

// fraction_dispersed of disperse_noaa with the density and viscosity of the property update
__device__ __forceinline__ double weather_dispersed_fraction(const WeatherOil &O, const double *R, const WeatherIn &E, float ws, double density,
                                                             double viscosity, double dt) {
  const float hs = weather_hs_f32(R, E.hs, ws);
  const double dissipation = ((0.0034 * O.rho_w) * 9.81) * (double)__fmul_rn(hs, hs);       // wave_energy_dissipation, Delvigne and Sweeney
  const double c_disp = pow(dissipation, 0.57) * (double)weather_breaking_fraction_f32(ws, weather_period_f32(R, E.tp, ws));
  const double C_Roy = 2400.0 * exp(-73.682 * sqrt(viscosity / density));
  const double q_disp = C_Roy * c_disp * 3.9E-8 / density;
  const double f = q_disp * dt * density;
  return f >= 1 ? .99 : f;
}

// fraction_biodegraded: half_time (:568-577, float64) or Adcroft (:595-602, float32 on the float32 temperature)
__device__ __forceinline__ double weather_biodegraded_fraction(int flags, const WeatherIn &E, float Tk, const double *s, double dt) {
  const double age0 = dt / (3600 * 24);
  if (flags & WEATHER_BIO_HALF_TIME) {
    const double half_time = E.z == 0 ? s[WS_HALF_TIME_SLICK] : s[WS_HALF_TIME_DROPLET];
    return 1 - exp(-age0 / half_time);
  }
  const float swt = Tk > 100.f ? __fsub_rn(Tk, (float)273.15) : Tk;
  const float tau = __fmul_rn(12.f, powf(3.f, __fdiv_rn(__fsub_rn(20.f, swt), 10.f)));
  return (double)__fsub_rn(1.f, expf(__fdiv_rn((float)-age0, tau)));
}

// One element, one step.  s: its record [WS_N]; mc: its row of mass_components; K: the component constants [4][OIL_MAXCOMP]; R: the
// reduction in front of the step [WR_N].  Emulsification and dispersion use the evaporated fraction, density and viscosity formed
// before this step's evaporation; evaporation acts at z == 0, emulsification behind the bullwinkle test, dispersion and
// biodegradation on every element.  The row is read twice and written once under evaporation, read and written once under
// dispersion or biodegradation alone.  Returns the temperature in Kelvin.
__device__ __forceinline__ float weather_element(const WeatherOil &O, const double *K, const double *R, int flags, double dt, const WeatherIn &E,
                                                 double *s, double *mc) {
  const float Tk = weather_kelvin_f32(E.temp);
  if (flags & WEATHER_PROPERTIES) weather_properties(O, Tk, s);
  const float ws = weather_wind_speed_f32(E.xwind, E.ywind);
  const double density = s[WS_DENSITY], viscosity = s[WS_VISCOSITY], fe = s[WS_FRACTION_EVAPORATED];
  const int n = O.ncomp;
  // what scales the row behind evaporation
  const bool disperse = (flags & WEATHER_DISPERSION) != 0, biodegrade = (flags & (WEATHER_BIO_HALF_TIME | WEATHER_BIO_ADCROFT)) != 0;
  const double fd = disperse ? weather_dispersed_fraction(O, R, E, ws, density, viscosity, dt) : 0.;
  const double fb = biodegrade ? weather_biodegraded_fraction(flags, E, Tk, s, dt) : 0.;
  const double keep_d = 1 - fd;
  // biodegradation_adcroft multiplies by the float32 (1 - fraction)
  const double keep_b = (flags & WEATHER_BIO_ADCROFT) ? (double)__fsub_rn(1.f, (float)fb) : 1 - fb;
  auto scaled = [&](double m) {
    if (disperse) m = m * keep_d;
    if (biodegrade) m = m * keep_b;
    return m;
  };
  // ---- evaporation: no surface element, or the youngest older than 24 h, stops it for the whole call (:828-834)
  const bool evaporate = (flags & WEATHER_EVAPORATION) && E.z == 0 && R[WR_NSURF] > 0 && !(R[WR_MIN_AGE_SURF] > 3600 * 24);
  if (evaporate) {
    const double area = (s[WS_MASS_OIL] / density) / s[WS_FILM];
    const float Kt = weather_mass_transport_f32(ws);
    const double sum_mi_mw = weather_np_sum(n, [&](int k) { return mc[k] / K[WC_MW * OIL_MAXCOMP + k]; });
    const double T = (double)Tk;
    const double pre = -(area * 1.0 * (double)Kt) / ((double)__fmul_rn((float)8.314, Tk) * sum_mi_mw);
    const WeatherPair sums = weather_np_sum2(n, [&](int k) {
      const double var = K[WC_INV * OIL_MAXCOMP + k] - 1. / (T - K[WC_C * OIL_MAXCOMP + k]);
      const double vp = exp(K[WC_A * OIL_MAXCOMP + k] * var) * 101325.0;
      const double m0 = mc[k], remain = m0 * exp((pre * vp) * dt);
      mc[k] = scaled(remain);
      return WeatherPair{m0 - remain, remain};
    });
    s[WS_MASS_EVAPORATED] = s[WS_MASS_EVAPORATED] + sums.a;
    s[WS_MASS_OIL] = sums.b;
  } else if (disperse || biodegrade) {
    for (int k = 0; k < n; ++k) mc[k] = scaled(mc[k]);
  }
  // ---- emulsification
  if ((flags & WEATHER_EMULSIFICATION) && weather_starts_emulsion(O, E.age, fe)) {
    double Y = O.y_max;
    if (O.mwf_n > 0 && R[WR_MIN_YDIFF] > 0) {
      const double sintef = (double)weather_sintef_f32(O, Tk);
      Y = Y < sintef ? Y : sintef;
    }
    const double S_max = (6. / 1.0e-6) * (Y / (1.0 - Y));
    const double start_time = O.bulltime > 0 ? O.bulltime : (E.age >= 0 ? s[WS_BULLTIME] : E.age);
    const float k_emul = __fdiv_rn(__fmul_rn(__fmul_rn((float)(6.0 * 2.024e-06), ws), ws), (float)1.0e-5);     // noaa.water_uptake_coefficient
    double ia = s[WS_INTERFACIAL_AREA] + ((double)__fmul_rn(k_emul, (float)dt) * exp(((double)-k_emul / S_max) * (E.age - start_time)));
    ia = ia < S_max ? ia : S_max;
    s[WS_INTERFACIAL_AREA] = ia;
    const double wf = ia * 1.0e-5 / (6.0 + (ia * 1.0e-5));
    s[WS_WATER_FRACTION] = wf < Y ? wf : Y;
  }
  // ---- dispersion, then biodegradation, of the oil mass
  if (disperse) {
    const double loss = fd * s[WS_MASS_OIL];
    s[WS_MASS_OIL] = s[WS_MASS_OIL] - loss;
    s[WS_MASS_DISPERSED] = s[WS_MASS_DISPERSED] + loss;
  }
  if (biodegrade) {
    const double now = s[WS_MASS_OIL] * fb;
    s[WS_MASS_BIODEGRADED] = s[WS_MASS_BIODEGRADED] + now;
    s[WS_MASS_OIL] = s[WS_MASS_OIL] - now;
  }
  return Tk;
}

// what an element adds to the reduction in front of a step; v: [WR_N], folded with weather_fold
__device__ __forceinline__ void weather_reduce_init(double *v) {
  const double inf = __builtin_inf();
  v[WR_NSURF] = 0; v[WR_MIN_AGE_SURF] = inf; v[WR_MIN_YDIFF] = inf; v[WR_HS_MAX] = -inf; v[WR_TP_MAX] = -inf; v[WR_TP_MIN] = inf;
  v[WR_TP_SUM] = 0; v[WR_TP_CNT] = 0;
}
__device__ __forceinline__ void weather_fold(double *v, const double *w) {
  v[WR_NSURF] += w[WR_NSURF]; v[WR_TP_SUM] += w[WR_TP_SUM]; v[WR_TP_CNT] += w[WR_TP_CNT];
  v[WR_MIN_AGE_SURF] = w[WR_MIN_AGE_SURF] < v[WR_MIN_AGE_SURF] ? w[WR_MIN_AGE_SURF] : v[WR_MIN_AGE_SURF];
  v[WR_MIN_YDIFF] = w[WR_MIN_YDIFF] < v[WR_MIN_YDIFF] ? w[WR_MIN_YDIFF] : v[WR_MIN_YDIFF];
  v[WR_TP_MIN] = w[WR_TP_MIN] < v[WR_TP_MIN] ? w[WR_TP_MIN] : v[WR_TP_MIN];
  v[WR_HS_MAX] = w[WR_HS_MAX] > v[WR_HS_MAX] ? w[WR_HS_MAX] : v[WR_HS_MAX];
  v[WR_TP_MAX] = w[WR_TP_MAX] > v[WR_TP_MAX] ? w[WR_TP_MAX] : v[WR_TP_MAX];
}
__device__ __forceinline__ void weather_reduce_element(const WeatherOil &O, const WeatherIn &E, int flags, const double *s, double *v) {
  // the evaporated fraction the property update is about to form, or the stored one when the launch leaves that update out
  const double fe = (flags & WEATHER_PROPERTIES) ? s[WS_MASS_EVAPORATED] / (s[WS_MASS_OIL] + s[WS_MASS_EVAPORATED]) : s[WS_FRACTION_EVAPORATED];
  weather_reduce_init(v);
  if (E.z == 0) { v[WR_NSURF] = 1; v[WR_MIN_AGE_SURF] = E.age; }
  v[WR_HS_MAX] = (double)E.hs; v[WR_TP_MAX] = (double)E.tp; v[WR_TP_MIN] = (double)E.tp;
  if (E.tp > 0.f) { v[WR_TP_SUM] = (double)E.tp; v[WR_TP_CNT] = 1; }
  if (O.mwf_n > 0 && weather_starts_emulsion(O, E.age, fe))
    v[WR_MIN_YDIFF] = O.y_max - (double)weather_sintef_f32(O, weather_kelvin_f32(E.temp));
}

}  // namespace odr
