// PlastDrift, and the parameterisation of absent waves from the wind that its defaults turn on.
//
//   wave_stokes_drift_parameterised          models/physics_methods.py:488-527          plast_stokes_from_wind / k_stokes_from_wind
//   wave_significant_height_parameterised    models/physics_methods.py:530-568          plast_hs_from_wind     / k_stokes_from_wind
//   PlastDrift.update_particle_depth         models/plastdrift.py:94-107 ('analytical') plast_depth           / k_plast_depth
//
// Rounding contract (asserted against the reference by tools/gen_golden_plastdrift.py).
// Environment.get_environment hands the two functions MASKED float32 arrays.  A masked array ** 2 is float64 (np.ma.power takes
// the exponent as a 0-d integer array, which NumPy does not treat as a weak scalar), so the wind speed is formed in float64 from
// the widened components: two exact squares, one rounded sum, one correctly rounded square root, capped at 30 (a NaN stays).
// np.polyval is a float64 Horner chain y = y * x + c from y = 0 with the leading coefficient first, every product and sum
// rounded on its own; the Stokes components are the widened wind components times the factor, float64; the assignment into the
// float32 environment rounds ONCE.  The coefficients are np.polyfit's over the reference's tables: data of the reference, handed
// in by the caller (at most 7 for the drift factor, 2 for the wave height), never held here.
// The depth: environment.ocean_vertical_diffusivity / elements.terminal_velocity is ONE float32 division, widened by
// np.random.exponential, which returns scale * standard_exponential: z = -(scale * E), float64, one product.  NumPy refuses a
// scale whose sign bit is set and that is not NaN (ValueError 'scale < 0': -0.0 too); a NaN scale gives NaN.
//
// Compiled for the CPU by tests/plast_host.cpp (the rounding intrinsics are its own there): this header includes nothing.
#pragma once

namespace odr {

enum { PLAST_STOKES = 1, PLAST_HS = 2 };      // which group k_stokes_from_wind writes (ODR_PLAST_* of include/odrift.h)
constexpr int PLAST_MAX_COEFF = 7, PLAST_HS_COEFF = 2;
struct PlastCoeff {                            // a launch argument: read through scalar loads, never indexed at run time
  double stokes[PLAST_MAX_COEFF], hs[PLAST_HS_COEFF];
  int n_stokes;
};

__device__ __forceinline__ double plast_wind_speed(float xw, float yw) {
  const double x = (double)xw, y = (double)yw;
  const double s = __dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
  return s > 30.0 ? 30.0 : s;                 // windspeed[windspeed > 30] = 30
}
template <int N>
__device__ __forceinline__ double plast_polyval(const double *c, int n, double x) {
  double y = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (k < n) y = __dadd_rn(__dmul_rn(y, x), c[k]);
  return y;
}
// the float32 values the environment holds behind the assignment
__device__ __forceinline__ void plast_stokes_from_wind(const PlastCoeff &C, float xw, float yw, float &sx, float &sy) {
  const double wf = plast_polyval<PLAST_MAX_COEFF>(C.stokes, C.n_stokes, plast_wind_speed(xw, yw));
  sx = (float)__dmul_rn((double)xw, wf);
  sy = (float)__dmul_rn((double)yw, wf);
}
__device__ __forceinline__ float plast_hs_from_wind(const PlastCoeff &C, float xw, float yw) {
  return (float)plast_polyval<PLAST_HS_COEFF>(C.hs, PLAST_HS_COEFF, plast_wind_speed(xw, yw));
}

__device__ __forceinline__ double plast_scale(float K, float w) { return (double)__fdiv_rn(K, w); }
__device__ __forceinline__ bool plast_scale_refused(double scale) { return scale == scale && __builtin_signbit(scale); }
__device__ __forceinline__ double plast_depth(double scale, double E) { return -__dmul_rn(scale, E); }

#ifndef ODR_PLAST_HOST
// One element per thread, active elements only; 8 B read and 4 B of status, 8 / 4 / 12 B written per element by `flags`.
__global__ __launch_bounds__(256) void k_stokes_from_wind(long long n, const int *__restrict__ status, const float *__restrict__ xw,
                                                          const float *__restrict__ yw, float *__restrict__ sx, float *__restrict__ sy,
                                                          float *__restrict__ hs, PlastCoeff C, int flags) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || status[i] != 0) return;
  const float x = xw[i], y = yw[i];
  if (flags & PLAST_STOKES) {
    float a, b;
    plast_stokes_from_wind(C, x, y, a, b);
    sx[i] = a;
    sy[i] = b;
  }
  if (flags & PLAST_HS) hs[i] = plast_hs_from_wind(C, x, y);
}

// *refused = 1 when some active element has a scale NumPy refuses; k_plast_depth, enqueued behind it, then writes nothing
__global__ __launch_bounds__(256) void k_plast_check(long long n, const int *__restrict__ status, const float *__restrict__ K,
                                                     const float *__restrict__ w, unsigned long long *refused) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || status[i] != 0) return;
  if (plast_scale_refused(plast_scale(K[i], w[i]))) *refused = 1ull;
}

// The standard exponential of the device generator: the element's Philox block of this step at RNG_OFF_PLAST (the keying of
// the other device draws, rng_block), its first 53 bits v as u = v 2^-53 in [0, 1) -- NumPy's own range -- and E = -log1p(-u),
// finite.  1 - u = (2^53 - v) 2^-53 is exact in float64, so log1p(-u) is the logarithm of a positive normal number: log_pos, the
// routine the normal draws take theirs with (odr_geodesic.hip.h: ~25 instructions, <= 3 ulp).
// The offset lies behind every other consumer's range of a step (the oil's sub-step blocks end at 8000, its diameter block is
// 8000 .. 8003) and below RNG_STEP_STRIDE: the streams stay disjoint whatever models share a seed.
constexpr unsigned long long RNG_OFF_PLAST = 8100;
static_assert(RNG_OFF_PLAST % 4 == 0 && RNG_OFF_PLAST + 4 <= RNG_STEP_STRIDE, "one Philox block inside the step's stride");
__device__ __forceinline__ double plast_device_exponential(unsigned long long seed, int id, unsigned long long step) {
  const uint4 b = rng_block(seed, id, step, RNG_OFF_PLAST);
  const unsigned long long v = (unsigned long long)b.x | ((unsigned long long)(b.y >> 11) << 32);
  return -log_pos(__dmul_rn((double)(0x20000000000000ull - v), 0x1p-53));
}

// One element per thread, active elements only: z = -(K / w) * E.  draws: one standard exponential per element of the set, in its
// order (rng_mode ODR_RNG_HOST), else the device generator.  8 B read and 4 B of status (+ 8 B of draws), 8 B written per element.
__global__ __launch_bounds__(256) void k_plast_depth(long long n, const int *__restrict__ status, const int *__restrict__ id,
                                                     const float *__restrict__ K, const float *__restrict__ w, double *__restrict__ z,
                                                     int rng_mode, const double *__restrict__ draws, unsigned long long seed,
                                                     unsigned long long step, const unsigned long long *__restrict__ refused) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || status[i] != 0 || *refused) return;
  const double E = rng_mode == 1 ? draws[i] : plast_device_exponential(seed, id[i], step);
  z[i] = plast_depth(plast_scale(K[i], w[i]), E);
}
#endif  // ODR_PLAST_HOST

}  // namespace odr
