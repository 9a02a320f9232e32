// PelagicEggDrift: the buoyancy of a pelagic fish egg from the temperature and salinity of the water around it.
//
//   PelagicEggDrift.update_terminal_velocity    models/pelagicegg.py:100-179           egg_terminal_velocity_f32
//
// (Sundby 1983, Deep Sea Research 30; the LADIM formulation of Vikebo et al. 2007.)  The egg has the temperature of the water and
// the salinity it is neutrally buoyant at: the density difference comes from the equation of state (odr_seawater.hip.h).
//
// Rounding contract.  The reference works on float32 arrays (environment, diameter, neutral_buoyancy_salinity) and Python
// float constants, which NumPy 2 casts to float32: every + - * / below is ONE IEEE single operation, in the reference's order,
// without contraction.  The Stokes velocity and the regime test W*1000*d/mu > 0.5 use nothing else, so they -- and the choice
// of the branch -- are reproduced bit for bit.  The high-Reynolds branch (Dallavalle's empirical form, cgs units) has an exp
// and three fractional powers, which NumPy evaluates with float32 routines that are not correctly rounded: here each is
// evaluated in float64 (the exponent being the float32 value NumPy uses) and rounded once.  Only the selected branch is
// evaluated; the reference forms both and stores the selected one (its unused high-Reynolds value is NaN for a sinking egg).
//
// Compiled for the CPU by tests/egg_host.cpp (the rounding intrinsics are its own there): includes nothing but the chains.
#pragma once
#include "odr_seawater.hip.h"

namespace odr {

enum { EGG_DIAMETER = 0, EGG_NEUTRAL_SALINITY = 1, EGG_DENSITY = 2, EGG_HATCHED = 3 };   // property slots of the model

#define EF(x) ((float)(x))
// x ** e of a float32 array and a Python float: float32 result, the exponent cast to float32
__device__ __forceinline__ float egg_pow_f32(float x, float e) { return (float)pow((double)x, (double)e); }

// T [deg C], S: the water at the element; d [m]: egg diameter; s_egg: salinity of neutral buoyancy.  Returns the terminal
// velocity [m/s, positive upwards]; high_re: the regime the value was taken from
__device__ __forceinline__ float egg_terminal_velocity_f32(float T, float S, float d, float s_egg, bool &high_re) {
  const float g = EF(9.81);
  const float rho_w = oil_sea_water_density_f32(T, S);
  const float dr = __fsub_rn(rho_w, oil_sea_water_density_f32(T, s_egg));   // DENSw - DENSegg
  const float mu = oil_water_viscosity_f32(T, S);
  // W = (1.0/my_w)*(1.0/18.0)*g*eggsize**2 * dr                      (Stokes; left to right)
  float W = __fmul_rn(__fdiv_rn(1.0f, mu), EF(1.0 / 18.0));
  W = __fmul_rn(W, g);
  W = __fmul_rn(W, __fmul_rn(d, d));
  W = __fmul_rn(W, dr);
  high_re = __fdiv_rn(__fmul_rn(__fmul_rn(W, 1000.f), d), mu) > 0.5f;       // Re > 0.5
  if (!high_re) return W;
  // lengths in cm from here on.  my_w = 0.01854 * exp(-0.02783 * T)  [cm2/s]
  const float nu = __fmul_rn(EF(0.01854), (float)exp((double)__fmul_rn(EF(-0.02783), T)));
  // d0 = (eggsize * 100) - 0.4 * (9.0 * my_w**2 / (100 * g) * DENSw / dr)**(1.0 / 3.0)
  float x = __fmul_rn(9.0f, __fmul_rn(nu, nu));
  x = __fdiv_rn(x, EF(100 * 9.81));
  x = __fdiv_rn(__fmul_rn(x, rho_w), dr);
  const float d0 = __fsub_rn(__fmul_rn(d, 100.f), __fmul_rn(EF(0.4), egg_pow_f32(x, EF(1.0 / 3.0))));
  // W2 = 19.0*d0*(0.001*dr)**(2.0/3.0)*(my_w*0.001*DENSw)**(-1.0/3.0)  [cm/s], / 100
  float W2 = __fmul_rn(19.0f, d0);
  W2 = __fmul_rn(W2, egg_pow_f32(__fmul_rn(EF(0.001), dr), EF(2.0 / 3.0)));
  W2 = __fmul_rn(W2, egg_pow_f32(__fmul_rn(__fmul_rn(nu, EF(0.001)), rho_w), EF(-1.0 / 3.0)));
  return __fdiv_rn(W2, 100.f);
}
#undef EF

#ifndef ODR_EGG_HOST
// one element per thread: T, S and the two properties in, the terminal velocity out (20 B per element, coalesced)
__global__ __launch_bounds__(256) void k_egg_terminal_velocity(long long n, const float *__restrict__ T, const float *__restrict__ S,
                                                               const float *__restrict__ diameter,
                                                               const float *__restrict__ neutral_salinity,
                                                               float *__restrict__ terminal_velocity) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool high_re;
  terminal_velocity[i] = egg_terminal_velocity_f32(T[i], S[i], diameter[i], neutral_salinity[i], high_re);
}
#endif  // ODR_EGG_HOST

}  // namespace odr
