// TEST INFRASTRUCTURE: the per-element arithmetic of opendrift_amd/csrc/odr_egg.hip.h (the device code of
// PelagicEggDrift.update_terminal_velocity) compiled for the CPU with g++ -ffp-contract=off, so that it can be compared with
// the reference's values without a GPU (tests/test_egg_device_arithmetic.py).  tests/hostshim stands in for
// <hip/hip_runtime.h>; the single-precision rounding intrinsics are IEEE single operations; the kernel itself is excluded
// by ODR_EGG_HOST.
#include <hip/hip_runtime.h>

#define ODR_EGG_HOST 1
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
#include "../opendrift_amd/csrc/odr_egg.hip.h"

extern "C" void eggh_terminal_velocity(long long n, const float *temp, const float *salt, const float *diameter,
                                       const float *neutral_salinity, float *w, unsigned char *high_re) {
  for (long long i = 0; i < n; ++i) {
    bool hr;
    w[i] = odr::egg_terminal_velocity_f32(temp[i], salt[i], diameter[i], neutral_salinity[i], hr);
    high_re[i] = hr ? 1 : 0;
  }
}
