// TEST INFRASTRUCTURE: the per-element arithmetic of opendrift_amd/csrc/odr_larval.hip.h (the device code of
// LarvalFish.update_fish_larvae and LarvalFish.larvae_vertical_migration) compiled for the CPU with g++ -ffp-contract=off, so
// that it can be compared with the reference's values without a GPU (tests/test_larval_device_arithmetic.py).  tests/hostshim
// stands in for <hip/hip_runtime.h>; the single-precision rounding intrinsics are IEEE single operations; the kernels
// themselves are excluded by ODR_LARVAL_HOST.  The loops do what the kernels do with an element, store for store.
#include <hip/hip_runtime.h>

#define ODR_LARVAL_HOST 1
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
#include "../opendrift_amd/csrc/odr_larval.hip.h"

// written[i]: bit 0 stage_fraction, bit 1 hatched, bit 2 weight and length were stored
extern "C" void larvh_update(long long n, const float *temp, double dt_seconds, float *stage, float *hatched, float *weight,
                             float *length, unsigned char *written) {
  const float days_f = odr::larval_days_in_timestep_f32(dt_seconds), dt_f = (float)dt_seconds;
  for (long long i = 0; i < n; ++i) {
    written[i] = 0;
    const float h0 = hatched[i];
    if (h0 != 0.f && h0 != 1.f) continue;
    float h = h0, s = h0 == 0.f ? stage[i] : 1.f, w = weight[i], L = 0.f;
    if (odr::larval_update_f32(temp[i], days_f, dt_f, s, h, w, L)) { weight[i] = w; length[i] = L; written[i] |= 4; }
    if (h0 == 0.f) {
      stage[i] = s; written[i] |= 1;
      if (h != h0) { hatched[i] = h; written[i] |= 2; }
    }
  }
}

extern "C" void larvh_migrate(long long n, const float *hatched, const float *length, double fraction_swimming, double dt_seconds,
                              int direction, double *z, float *displacement) {
  for (long long i = 0; i < n; ++i) {
    displacement[i] = 0.f;
    if (hatched[i] != 1.f) continue;
    const float reach = __fmul_rn(__fmul_rn((float)fraction_swimming, odr::larval_swim_f32(length[i])), (float)dt_seconds);
    displacement[i] = __fmul_rn((float)direction, reach);      // (what larval_migrate adds, for the test's ulp measure)
    z[i] = odr::larval_migrate(z[i], length[i], (float)fraction_swimming, (float)dt_seconds, (float)direction);
  }
}
