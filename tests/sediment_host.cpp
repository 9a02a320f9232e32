// TEST INFRASTRUCTURE: the per-element arithmetic of opendrift_amd/csrc/odr_sediment.hip.h (the device code of
// SedimentDrift.resuspension) compiled for the CPU with g++ -ffp-contract=off, so that it can be compared with the
// reference's values without a GPU (tests/test_sediment_device_arithmetic.py).  tests/hostshim stands in for
// <hip/hip_runtime.h> (it has the float64 rounding intrinsics); the float32 ones are IEEE single operations; the kernel itself is excluded by ODR_SEDIMENT_HOST.
#include <hip/hip_runtime.h>
#include <cmath>

#define ODR_SEDIMENT_HOST 1
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
#include "../opendrift_amd/csrc/odr_sediment.hip.h"

// moving / z in place; returns the number of resuspended elements
extern "C" long long sedh_resuspend(long long n, const float *u, const float *v, float threshold, int *moving, double *z) {
  long long count = 0;
  for (long long i = 0; i < n; ++i) count += odr::sediment_resuspend(u[i], v[i], threshold, moving[i], z[i]) ? 1 : 0;
  return count;
}
