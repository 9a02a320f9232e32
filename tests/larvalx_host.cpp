// TEST INFRASTRUCTURE: the per-element arithmetic of opendrift_amd/csrc/odr_larvalx.hip.h and odr_solar.hip.h (the device code
// of LarvalFishExtended.update_fish_larvae, LarvalFishExtended._apply_vertical_behavior and OceanDrift.solar_elevation) compiled
// for the CPU with g++ -ffp-contract=off, so that it can be compared with the reference's values without a GPU
// (tests/test_larvalx_device_arithmetic.py).  tests/hostshim stands in for <hip/hip_runtime.h>; the rounding intrinsics are IEEE
// operations; the kernels themselves are excluded by ODR_LARVALX_HOST.  The loops do what the kernels do with an element, store
// for store, and what the entry points do with their scalars.
#include <hip/hip_runtime.h>

#define ODR_LARVALX_HOST 1
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline double __ddiv_rn(double a, double b) { volatile double r = a / b; return r; }
#include "../opendrift_amd/csrc/odr_larvalx.hip.h"

extern "C" void larvxh_elevation(long long n, const double *lon, const double *lat, double declination_rad, double eqtime,
                                 double day_minutes, double *out) {
  const double sin_d = std::sin(declination_rad), cos_d = std::cos(declination_rad);
  for (long long i = 0; i < n; ++i) out[i] = odr::solar_elevation_deg(lon[i], lat[i], sin_d, cos_d, eqtime, day_minutes);
}

extern "C" void larvxh_hatch(long long n, double increment, float *stage, float *hatched) {
  for (long long i = 0; i < n; ++i) {
    if (hatched[i] != 0.f) continue;
    float s = stage[i];
    const bool h = odr::larvalx_hatch_f32(s, (float)increment);
    stage[i] = s;
    if (h) hatched[i] = 1.f;
  }
}

// day[i]: the flag the element used (0 for an element that does not move, and in mode depth)
extern "C" void larvxh_behave(long long n, const float *hatched, const float *depth, const double *lon, const double *lat, int mode,
                              int only_hatched, int z_f32, double c0, double hw0, double c1, double hw1, double w_active, double dt,
                              double declination_rad, double eqtime, double day_minutes, double *z, unsigned char *day) {
  for (long long i = 0; i < n; ++i) day[i] = 0;
  if (!(w_active > 0.0) || !(dt > 0.0)) return;
  odr::LarvalxBehave B;
  B.band_min[0] = c0 - hw0; B.band_max[0] = c0 + hw0;
  B.band_min[1] = c1 - hw1; B.band_max[1] = c1 + hw1;
  B.max_step = w_active * dt;
  B.sin_d = std::sin(declination_rad); B.cos_d = std::cos(declination_rad);
  B.eqtime = eqtime; B.day_minutes = day_minutes;
  B.mode = mode; B.z_f32 = z_f32 != 0; B.only_hatched = only_hatched != 0;
  for (long long i = 0; i < n; ++i) {
    if (B.only_hatched && hatched[i] != 1.f) continue;
    bool d = false;
    if (B.mode == odr::LARVALX_MODE_DVM) d = odr::solar_elevation_deg(lon[i], lat[i], B.sin_d, B.cos_d, B.eqtime, B.day_minutes) > 0.0;
    day[i] = d;
    z[i] = odr::larvalx_behave(z[i], depth[i], d, B);
  }
}
