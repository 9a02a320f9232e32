// Sea-water density and dynamic viscosity as the reference's models evaluate them on the float32 environment:
//
//   PhysicsMethods.sea_water_density            models/physics_methods.py:574-608      oil_sea_water_density_f32
//   seawater_dynamic_viscosity_sharqawy         models/physics_methods.py:159-178      oil_water_viscosity_f32
//
// float32 arrays times Python float constants stay float32 under NumPy 2: every operation is one IEEE single operation in the
// reference's order, the constants are cast to float32, nothing is contracted.  Shared by the oil physics of the mixing loop
// (odr_oil.hip.h) and the pelagic egg model (odr_egg.hip.h); tests/oil_host.cpp and tests/egg_host.cpp compile it for the
// CPU (the rounding intrinsics are theirs there), so it includes nothing.
#pragma once

namespace odr {

#define OF(x) ((float)(x))
__device__ __forceinline__ float oil_sea_water_density_f32(float T, float S) {
  float R1 = __fsub_rn(__fmul_rn(OF(6.536332E-09), T), OF(1.120083E-06));
  R1 = __fadd_rn(__fmul_rn(R1, T), OF(1.001685E-04));
  R1 = __fsub_rn(__fmul_rn(R1, T), OF(9.095290E-03));
  R1 = __fadd_rn(__fmul_rn(R1, T), OF(6.793952E-02));
  R1 = __fsub_rn(__fmul_rn(R1, T), OF(28.263737));
  float R2 = __fsub_rn(__fmul_rn(OF(5.3875E-09), T), OF(8.2467E-07));
  R2 = __fadd_rn(__fmul_rn(R2, T), OF(7.6438E-05));
  R2 = __fsub_rn(__fmul_rn(R2, T), OF(4.0899E-03));
  R2 = __fadd_rn(__fmul_rn(R2, T), OF(8.24493E-01));
  float R3 = __fadd_rn(__fmul_rn(OF(-1.6546E-06), T), OF(1.0227E-04));
  R3 = __fsub_rn(__fmul_rn(R3, T), OF(5.72466E-03));
  const float in = __fadd_rn(__fadd_rn(__fmul_rn(OF(4.8314E-04), S), __fmul_rn(R3, sqrtf(S))), R2);
  const float SIG = __fadd_rn(R1, __fmul_rn(in, S));
  return __fadd_rn(__fadd_rn(SIG, OF(28.106331)), 1000.f);
}

__device__ __forceinline__ float oil_water_viscosity_f32(float T, float S) {
  const float t1 = __fadd_rn(T, OF(64.993));
  const float mu_w = __fadd_rn(OF(4.2844e-5), __fdiv_rn(1.0f, __fsub_rn(__fmul_rn(OF(0.157), __fmul_rn(t1, t1)), OF(91.296))));
  const float T2 = __fmul_rn(T, T);
  const float A = __fsub_rn(__fadd_rn(OF(1.541), __fmul_rn(OF(1.998e-2), T)), __fmul_rn(OF(9.52e-5), T2));
  const float B = __fadd_rn(__fsub_rn(OF(7.974), __fmul_rn(OF(7.561e-2), T)), __fmul_rn(OF(4.724e-4), T2));
  const float s = __fdiv_rn(S, 1000.f);
  return __fmul_rn(mu_w, __fadd_rn(__fadd_rn(1.f, __fmul_rn(A, s)), __fmul_rn(B, __fmul_rn(s, s))));
}
#undef OF

}  // namespace odr
