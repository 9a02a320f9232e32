// TEST INFRASTRUCTURE: the per-element arithmetic of opendrift_amd/csrc/odr_ship.hip.h (the device code of ShipDrift.update)
// compiled for the CPU with g++ -ffp-contract=off, so that it can be compared with the reference's values without a GPU
// (tests/test_ship_device_arithmetic.py) and with the device (tests/test_gpu_shipdrift.py).  tests/hostshim stands in for
// <hip/hip_runtime.h>; the kernel itself is excluded by ODR_SHIP_HOST.
#include <hip/hip_runtime.h>

#include <cstdint>

#define ODR_SHIP_HOST 1
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }
#include "../opendrift_amd/csrc/odr_ship.hip.h"

using namespace odr;

extern "C" int shiph_rows() { return SHIP_NTAB; }

extern "C" void shiph_ratios(long long n, const float *length, const float *draft, const float *beam, float *bl, float *dl) {
  for (long long i = 0; i < n; ++i) ship_ratios(length[i], draft[i], beam[i], bl[i], dl[i]);
}

// env: 8 arrays in the order of ShipEnv; prop: 6 arrays in the order of ShipProp's floats; table[n_classes][49][2];
// f32out: 7 arrays in the order of ShipForces' floats; f64out: 10 arrays in the order of its doubles
extern "C" void shiph_forces(long long n, const float *const *env, const float *const *prop, const int32_t *orientation, const int32_t *cls,
                             const double *table, int hs_mode, int tp_mode, int dir_from_stokes, float *const *f32out, double *const *f64out) {
  for (long long i = 0; i < n; ++i) {
    const ShipEnv e = {env[0][i], env[1][i], env[2][i], env[3][i], env[4][i], env[5][i], env[6][i], env[7][i]};
    const ShipProp p = {prop[0][i], prop[1][i], prop[2][i], prop[3][i], prop[4][i], prop[5][i], orientation[i]};
    const ShipForces r = ship_forces(e, p, table + (size_t)cls[i] * (2 * SHIP_NTAB), hs_mode, tp_mode, dir_from_stokes);
    const float f[7] = {r.bl, r.dl, r.Tm, r.Hs, r.F_wind_x, r.F_wind_y, r.beta1};
    const double d[10] = {r.F_wave_b, r.beta2_b, r.F_wave, r.beta2, r.wave_dir, r.F_total, r.uw_tot, r.uw_dir, r.vu, r.vv};
    for (int k = 0; k < 7; ++k) f32out[k][i] = f[k];
    for (int k = 0; k < 10; ++k) f64out[k][i] = d[k];
  }
}
