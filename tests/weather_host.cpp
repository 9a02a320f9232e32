// TEST INFRASTRUCTURE: the per-element code of opendrift_amd/csrc/odr_weather.hip.h (the device code of OpenOil's NOAA oil
// weathering) compiled for the CPU with g++ -ffp-contract=off, so that it can be compared with the reference's values without a
// GPU (tests/test_weather_device_arithmetic.py).  tests/hostshim stands in for <hip/hip_runtime.h>; the rounding intrinsics are IEEE
// operations; the oil arrives as the odr_oil_table of include/odrift.h.
#include <hip/hip_runtime.h>

#include "../include/odrift.h"
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
using std::exp; using std::pow; using std::sqrt;
#include "../opendrift_amd/csrc/odr_weather.hip.h"

using namespace odr;

static WeatherOil oil_of(const odr_oil_table *t) {
  WeatherOil O;
  O.ncomp = t->ncomp; O.stride = t->ncomp; O.mwf_n = t->mwf_n; O.pad = 0;
  O.rho_ref = t->density; O.rho_k = t->density_k; O.rho_T = t->density_ref_temp;
  O.nu_ref = t->viscosity; O.nu_B = t->viscosity_B; O.nu_T = t->viscosity_ref_temp;
  O.bulltime = t->bulltime; O.bullwinkle = t->bullwinkle; O.y_max = t->y_max; O.rho_w = t->sea_water_density;
  for (int k = 0; k < 2; ++k) { O.mwf_t[k] = t->mwf_t[k]; O.mwf_w[k] = t->mwf_w[k]; }
  return O;
}

// one odr_oil_weather call over n elements: rec [n][WS_N], mc [n][ncomp], red [WR_N] out; temp_k [n] out
extern "C" void weatherh_step(long long n, const odr_oil_table *t, int flags, double dt, const float *xw, const float *yw, const float *temp,
                              const float *hs, const float *tp, const double *z, const double *age, double *rec, double *mc, double *red,
                              float *temp_k) {
  const WeatherOil O = oil_of(t);
  auto in = [&](long long i) {
    WeatherIn E;
    E.xwind = xw[i]; E.ywind = yw[i]; E.temp = temp[i]; E.hs = hs[i]; E.tp = tp[i]; E.z = z[i]; E.age = age[i];
    return E;
  };
  weather_reduce_init(red);
  for (long long i = 0; i < n; ++i) {
    double v[WR_N];
    weather_reduce_element(O, in(i), flags, rec + i * WS_N, v);
    weather_fold(red, v);
  }
  for (long long i = 0; i < n; ++i) temp_k[i] = weather_element(O, t->comp, red, flags, dt, in(i), rec + i * WS_N, mc + i * O.ncomp);
}

// np.sum over the rows of a [n][m] array in the order weather_np_sum adds
extern "C" void weatherh_row_sums(long long n, int m, const double *a, double *out) {
  for (long long i = 0; i < n; ++i) out[i] = weather_np_sum(m, [&](int k) { return a[i * m + k]; });
}

// the two float32 chains whose powf / expf NumPy evaluates with its own vector code (an ulp of float32 apart from libm's on some
// arguments): the tests tell the elements on which both agree from the others
extern "C" void weatherh_mass_transport(long long n, const float *ws, float *out) {
  for (long long i = 0; i < n; ++i) out[i] = weather_mass_transport_f32(ws[i]);
}
extern "C" void weatherh_adcroft_fraction(long long n, const float *temp_k, double dt, float *out) {
  WeatherIn E = {};
  double s[WS_N] = {};
  for (long long i = 0; i < n; ++i) out[i] = (float)weather_biodegraded_fraction(WEATHER_BIO_ADCROFT, E, temp_k[i], s, dt);
}
