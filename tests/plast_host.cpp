// TEST INFRASTRUCTURE: the per-element arithmetic of opendrift_amd/csrc/odr_plast.hip.h (the device code of
// drift:use_tabularised_stokes_drift and of PlastDrift.update_particle_depth) compiled for the CPU with g++ -ffp-contract=off, so
// that it can be compared with the reference's values without a GPU (tests/test_plast_device_arithmetic.py).  tests/hostshim
// stands in for <hip/hip_runtime.h>; the rounding intrinsics are IEEE operations; the kernels are excluded by ODR_PLAST_HOST.
#include <hip/hip_runtime.h>

#define ODR_PLAST_HOST 1
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
static inline double __dsqrt_rn(double a) { volatile double r = std::sqrt(a); return r; }
#include "../opendrift_amd/csrc/odr_plast.hip.h"

extern "C" void plasth_stokes_from_wind(long long n, const float *xw, const float *yw, const double *stokes, int n_stokes,
                                        const double *hs_coeff, float *sx, float *sy, float *hs) {
  odr::PlastCoeff C = {};
  for (int k = 0; k < n_stokes && k < odr::PLAST_MAX_COEFF; ++k) C.stokes[k] = stokes[k];
  C.n_stokes = n_stokes;
  C.hs[0] = hs_coeff[0]; C.hs[1] = hs_coeff[1];
  for (long long i = 0; i < n; ++i) {
    odr::plast_stokes_from_wind(C, xw[i], yw[i], sx[i], sy[i]);
    hs[i] = odr::plast_hs_from_wind(C, xw[i], yw[i]);
  }
}

// z[i] = -(K[i] / w[i]) E[i]; returns whether some scale is one NumPy refuses (z is then left as it was)
extern "C" int plasth_depth(long long n, const float *K, const float *w, const double *E, double *z) {
  for (long long i = 0; i < n; ++i)
    if (odr::plast_scale_refused(odr::plast_scale(K[i], w[i]))) return 1;
  for (long long i = 0; i < n; ++i) z[i] = odr::plast_depth(odr::plast_scale(K[i], w[i]), E[i]);
  return 0;
}
