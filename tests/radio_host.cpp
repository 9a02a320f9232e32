// TEST INFRASTRUCTURE: the per-element code of opendrift_amd/csrc/odr_radio.hip.h (the device code of RadionuclideDrift's
// speciation, terminal velocity and resuspension) compiled for the CPU with g++ -ffp-contract=off, so that it can be compared
// with the reference's values without a GPU (tests/test_radio_device_arithmetic.py).  tests/hostshim stands in for
// <hip/hip_runtime.h>; the rounding intrinsics are IEEE operations; the kernels themselves are excluded by ODR_RADIO_HOST.
#include <hip/hip_runtime.h>

#define ODR_RADIO_HOST 1
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
static inline double __ddiv_rn(double a, double b) { volatile double r = a / b; return r; }
using std::exp;
#include "../opendrift_amd/csrc/odr_radio.hip.h"

using namespace odr;

struct HostDraws {
  const double *a[4];
  long long i;
  double operator()(int which) { return a[which][i]; }
};

// setup: the members of odr::RadioSetup in their order (7 doubles, 3 floats as doubles, 13 ints as doubles), see radio_host.py
static RadioSetup setup_of(const double *s) {
  RadioSetup S;
  S.dt = s[0]; S.layer_thick = s[1]; S.dia_part = s[2]; S.dia_diss = s[3]; S.dia_uncert = s[4]; S.desorb_std = s[5]; S.resusp_std = s[6];
  S.desorb_depth = (float)s[7]; S.resusp_depth = (float)s[8]; S.critvel = (float)s[9];
  S.nspecies = (int)s[10]; S.nsal = (int)s[11]; S.lognormal = (int)s[12];
  S.lmm = (int)s[13]; S.lmmcation = (int)s[14]; S.lmmanion = (int)s[15]; S.polymer = (int)s[16]; S.prev = (int)s[17]; S.srev = (int)s[18];
  S.psrev = (int)s[19]; S.ssrev = (int)s[20]; S.pirrev = (int)s[21]; S.sirrev = (int)s[22];
  return S;
}

// counts: [50], added to.  noise_is_final: the draws are the reference's values (else standard normals, as the device RNG's)
extern "C" void radioh_speciation(long long n, const double *setup, const double *table, float *specie, float *diameter, int *moving,
                                  double *z, const float *sal, const float *depth, const float *conc3, const double *u1,
                                  const double *u2, const double *diam_noise, const double *depth_noise, int noise_is_final,
                                  long long *counts) {
  const RadioSetup S = setup_of(setup);
  const RadioView V = {specie, diameter, moving, z, sal, depth, conc3, nullptr, nullptr};
  for (long long i = 0; i < n; ++i) {
    HostDraws D = {{u1, u2, diam_noise, depth_noise}, i};
    const int bin = radio_speciate_at(S, table, V, i, noise_is_final != 0, D);
    if (bin >= 0) counts[bin]++;
  }
}

extern "C" void radioh_probabilities(long long n, const double *setup, const double *table, const float *specie, const double *z,
                                     const float *sal, const float *depth, const float *conc3, double *p7, double *psum) {
  const RadioSetup S = setup_of(setup);
  for (long long i = 0; i < n; ++i) {
    double p[RADIO_MAXSP];
    psum[i] = radio_probabilities(S, table, (int)specie[i], sal[i], depth[i], conc3[i], z[i], p);
    for (int j = 0; j < RADIO_MAXSP; ++j) p7[i * RADIO_MAXSP + j] = p[j];
  }
}

extern "C" void radioh_terminal_velocity(long long n, const float *temp, const float *salt, const float *diameter, const float *density,
                                         const int *moving, float *w) {
  for (long long i = 0; i < n; ++i) w[i] = radio_terminal_velocity_f32(temp[i], salt[i], diameter[i], density[i], moving[i]);
}

extern "C" void radioh_resuspend(long long n, const double *setup, float *specie, float *diameter, int *moving, double *z, const float *u,
                                 const float *v, const float *depth, const double *diam_noise, const double *depth_noise,
                                 int noise_is_final, long long *counts) {
  const RadioSetup S = setup_of(setup);
  const RadioView V = {specie, diameter, moving, z, nullptr, depth, nullptr, u, v};
  for (long long i = 0; i < n; ++i) {
    HostDraws D = {{nullptr, nullptr, diam_noise, depth_noise}, i};
    int bins[2];
    if (!radio_resuspend_at(S, V, i, noise_is_final != 0, D, bins)) counts[RADIO_BAD_SPECIES]++;
    for (int b : bins)
      if (b >= 0) counts[b]++;
  }
}
