// TEST INFRASTRUCTURE: the per-element arithmetic, the fixed-order sums and the solver control flow of
// opendrift_amd/csrc/odr_berg.hip.h (the device code of OpenBerg.roll_over and OpenBerg.advect_iceberg) compiled for the CPU with
// g++ -ffp-contract=off, so that they can be compared with the reference's values without a GPU
// (tests/test_berg_device_arithmetic.py) and with the device bit for bit (tests/test_gpu_openberg.py).  tests/hostshim stands in for
// <hip/hip_runtime.h>; the kernels themselves are excluded by ODR_BERG_HOST.  The loops do what the kernels do with an element,
// store for store, and sum the workgroups' shares in the kernels' order (`block` = the library's workgroup size).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#define ODR_BERG_HOST 1
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
#include "../opendrift_amd/csrc/odr_berg.hip.h"

using namespace odr;

extern "C" void bergh_roll_over(long long n, float *sail, float *draft, float *length, float *width) {
  for (long long i = 0; i < n; ++i) berg_roll_over_f32(length[i], width[i], sail[i], draft[i]);
}

extern "C" double bergh_sin(double x) { return berg_sin(x); }
extern "C" void bergh_sincosf(long long n, const float *x, float *s, float *c) {
  for (long long i = 0; i < n; ++i) berg_sincosf_numpy(x[i], s[i], c[i]);
}

namespace {
struct BergHost {
  long long n;
  int block;
  long long nb;
  std::vector<BergElem> E;
  std::vector<double> yx, yy, fx, fy, ox, oy, gx, gy, part0, part1, v;
  // the workgroups' shares of element values val(i), then the fold over the workgroups
  template <class F> double sum(F val, std::vector<double> &part) {
    for (long long b = 0; b < nb; ++b) {
      for (int t = 0; t < block; ++t) { const long long i = b * block + t; v[t] = i < n ? val(i) : 0.0; }
      part[b] = berg_block_sum_host(v.data(), block);
    }
    return berg_fold_host(part.data(), nb, block);
  }
  int norms0(double s[2]) {
    s[0] = sum([&](long long i) { return berg_scaled_sq(yx[i], yy[i], yx[i], yy[i]); }, part0);
    s[1] = sum([&](long long i) { return berg_scaled_sq(fx[i], fy[i], yx[i], yy[i]); }, part1);
    return 0;
  }
  int probe(double h0, double &s) {
    s = sum([&](long long i) { return berg_probe(E[i], h0, yx[i], yy[i], fx[i], fy[i]); }, part0);
    return 0;
  }
  int attempt(double h, double &s) {
    s = sum([&](long long i) { return berg_attempt(E[i], h, yx[i], yy[i], fx[i], fy[i], ox[i], oy[i], gx[i], gy[i]); }, part0);
    return 0;
  }
  void accept() { yx.swap(ox); yy.swap(oy); fx.swap(gx); fy.swap(gy); }
};
}  // namespace

// env: 12 arrays in the order of BergEnv; coef: the six coefficients in the order of BergCoef; flags: wave_rad, stokes_drift,
// coriolis, grounding, lat_is_float32.  Returns the BERG_SOLVE_* code.  stat: attempts, rejected.
extern "C" int bergh_advect(long long n, const float *const *env, const double *lat, const float *sail, const float *draft, const float *length,
                            const float *width, int32_t *moving, const double *coef, double wave_from_direction, double sea_ice_thickness,
                            const int *flags, double dt, int block, double *v0x, double *v0y, double *vx, double *vy, float *xvel, float *yvel,
                            signed char *grounded, int32_t *stat) {
  BergCall C;
  C.k = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
  berg_wave_direction_f32(wave_from_direction, C.wave_sin, C.wave_cos);
  C.ice_thickness = (float)sea_ice_thickness;
  C.wave_rad = flags[0] != 0; C.stokes = flags[1] != 0; C.coriolis = flags[2] != 0; C.grounding = flags[3] != 0; C.lat_f32 = flags[4] != 0;
  BergHost be;
  be.n = n; be.block = block; be.nb = (n + block - 1) / block;
  be.E.resize(n);
  for (auto *a : {&be.yx, &be.yy, &be.fx, &be.fy, &be.ox, &be.oy, &be.gx, &be.gy}) a->assign(n, 0.0);
  be.part0.assign(be.nb, 0.0); be.part1.assign(be.nb, 0.0); be.v.assign(block, 0.0);
  for (long long i = 0; i < n; ++i) {
    const BergEnv e = {env[0][i], env[1][i], env[2][i], env[3][i], env[4][i], env[5][i], env[6][i], env[7][i], env[8][i], env[9][i], env[10][i], env[11][i]};
    int mv = moving[i];
    be.E[i] = berg_prepare(C, e, lat[i], sail[i], draft[i], length[i], width[i], mv, be.yx[i], be.yy[i]);
    moving[i] = mv;
    berg_rhs(be.E[i], be.yx[i], be.yy[i], be.fx[i], be.fy[i]);
    v0x[i] = be.yx[i]; v0y[i] = be.yy[i];
    grounded[i] = (be.E[i].cls & BERG_GROUNDED) != 0;
  }
  BergSolveStat st;
  berg_solve(be, n, dt, st);
  stat[0] = st.attempts; stat[1] = st.rejected;
  if (st.why != BERG_SOLVE_OK) return st.why;
  for (long long i = 0; i < n; ++i) {
    double x = be.yx[i], y = be.yy[i];
    if (be.E[i].cls & BERG_GROUNDED) { x = 0.0; y = 0.0; }
    vx[i] = x; vy[i] = y; xvel[i] = (float)x; yvel[i] = (float)y;
  }
  return 0;
}
