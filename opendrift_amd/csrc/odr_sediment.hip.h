// SedimentDrift: a settled element (moving == 0) is set moving again where the current is fast enough.
//
//   SedimentDrift.resuspension          models/sedimentdrift.py:118-126         sediment_resuspend
//   PhysicsMethods.current_speed        models/physics_methods.py:889-891       sediment_current_speed_f32
//
// (The settling itself -- SedimentDrift.bottom_interaction, sedimentdrift.py:108-116 -- is the sea-floor action
// ODR_SEAFLOOR_SETTLE inside the mixing sub-steps and odr_vertical_buoyancy, odr_kernels.hip.h.)
//
// Rounding contract.  current_speed() is np.sqrt(u**2 + v**2) on the float32 environment arrays: two IEEE single products,
// one sum, one correctly rounded single square root, without contraction.  NumPy 2 compares that float32 array with the
// Python float of the configuration cast to float32 (the caller hands the cast value in).  z is a float64 array:
// z + .01 is ONE IEEE double addition of the double nearest to 0.01.
//
// Compiled for the CPU by tests/sediment_host.cpp (the rounding intrinsics are its own there): includes nothing.
#pragma once

namespace odr {

__device__ __forceinline__ float sediment_current_speed_f32(float u, float v) {
  return sqrtf(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)));   // IEEE sqrt (-O3 without fast-math: correctly rounded)
}

// one element: true when it was resuspended (moving 0 -> 1, z one centimetre up)
__device__ __forceinline__ bool sediment_resuspend(float u, float v, float threshold, int &moving, double &z) {
  if (!(sediment_current_speed_f32(u, v) > threshold && moving == 0)) return false;
  moving = 1;                     // allow moving again
  z = __dadd_rn(z, 0.01);         // suspend 1 cm above where it lay
  return true;
}

#ifndef ODR_SEDIMENT_HOST
// one element per thread: u, v, moving, z in (20 B), moving and z out for the resuspended ones only (12 B); the count by a
// ballot per wave, the waves' counts summed in LDS, one atomicAdd per workgroup (n_out == nullptr: nothing is counted)
__global__ __launch_bounds__(256) void k_resuspend(long long n, const float *__restrict__ u, const float *__restrict__ v,
                                                   float threshold, int *__restrict__ moving, double *__restrict__ z,
                                                   unsigned long long *__restrict__ n_out) {
  __shared__ unsigned wave_n[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (i < n) {
    int m = moving[i];
    if (m == 0) {     // (a moving element reads nothing else)
      double zz = z[i];
      hit = sediment_resuspend(u[i], v[i], threshold, m, zz);
      if (hit) { moving[i] = m; z[i] = zz; }
    }
  }
  if (!n_out) return;    // (uniform over the grid)
  const unsigned long long b = __ballot(hit);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (unsigned)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    if (t) atomicAdd(n_out, (unsigned long long)t);
  }
}
#endif  // ODR_SEDIMENT_HOST

}  // namespace odr
