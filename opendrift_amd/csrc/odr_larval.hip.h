// LarvalFish: eggs hatch, larvae grow and swim up and down with the time of day.
//
//   LarvalFish.update_fish_larvae          models/larvalfish.py:200-231            larval_update_f32
//   LarvalFish.fish_growth                 models/larvalfish.py:185-198            larval_growth_f32
//   LarvalFish.larvae_vertical_migration   models/larvalfish.py:233-253            larval_swim_f32, larval_migrate
//
// (Ellertsen et al. 1988 for the egg stage, Folkvord 2005 for growth and length, Peck et al. 2006 for the swimming speed,
// after Kvile et al. 2018.  The terminal velocity of the model is PelagicEggDrift's, line for line: odr_egg.hip.h.)
//
// Rounding contract.  The reference works on float32 arrays (sea_water_temperature, stage_fraction, weight, length -- the
// dtypes the element type declares) and Python float constants, which NumPy 2 casts to float32: every + - * / and **2 below
// is ONE IEEE single operation, in the reference's order, without contraction.  `**3` is NOT a product there: NumPy has a
// fast path for the exponents -1, 0, 0.5, 1 and 2 only, and x**3 is np.power(x, float32(3)) bit for bit.  NumPy's float32
// exp, log, log10 and power are not correctly rounded: here each is evaluated in float64 on the float32 argument NumPy uses
// (float32(-0.08) is not -0.08) and rounded once.  The live z is a float64 array when the larvae swim (it is one after the
// vertical mixing) and direction * max_migration_per_timestep a float32 array: their sum is ONE IEEE double addition of the
// widened float32 displacement, and min(0, .) a float64 comparison.  Only the selected branch is evaluated: an egg never
// goes through the larval formulas (its length of 0 would give 5.289 / 0), and nothing of an egg but stage_fraction and
// hatched is written.
//
// Compiled for the CPU by tests/larval_host.cpp (the rounding intrinsics are its own there): includes nothing; the kernels
// (not part of the host build) take BLOCK from odr_kernels.hip.h, which the translation unit includes first.
#pragma once

namespace odr {

enum { LARVA_DIAMETER = 0, LARVA_NEUTRAL_SALINITY = 1, LARVA_STAGE_FRACTION = 2, LARVA_HATCHED = 3, LARVA_LENGTH = 4,
       LARVA_WEIGHT = 5, LARVA_SURVIVAL = 6 };   // property slots of the model

#define LF(x) ((float)(x))
__host__ __device__ __forceinline__ float larval_exp_f32(float x) { return (float)exp((double)x); }
__host__ __device__ __forceinline__ float larval_log_f32(float x) { return (float)log((double)x); }
__host__ __device__ __forceinline__ float larval_log10_f32(float x) { return (float)log10((double)x); }
// x ** e with a float32 exponent (an array, or a Python float cast to float32): float32 result
__host__ __device__ __forceinline__ float larval_pow_f32(float x, float e) { return (float)pow((double)x, (double)e); }

// days_in_timestep = self.time_step.total_seconds()/(60*60*24) (:206): a Python float, cast to float32 where it meets the array
inline float larval_days_in_timestep_f32(double dt_seconds) { return (float)(dt_seconds / 86400.0); }

// fish_growth (:185-198): the weight gained in one time step [mg]; T [deg C], dt_f = float32(time_step.total_seconds())
__host__ __device__ __forceinline__ float larval_growth_f32(float w, float T, float dt_f) {
  const float lw = larval_log_f32(w);
  // GR = 1.08 + 1.79*T - 0.074*T*log(w) - 0.0965*T*log(w)**2 + 0.0112*T*log(w)**3      (daily growth rate in percent)
  float GR = __fadd_rn(LF(1.08), __fmul_rn(LF(1.79), T));
  GR = __fsub_rn(GR, __fmul_rn(__fmul_rn(LF(0.074), T), lw));
  GR = __fsub_rn(GR, __fmul_rn(__fmul_rn(LF(0.0965), T), __fmul_rn(lw, lw)));
  GR = __fadd_rn(GR, __fmul_rn(__fmul_rn(LF(0.0112), T), larval_pow_f32(lw, 3.0f)));
  // g = (np.log(GR / 100. + 1)) * self.time_step.total_seconds()/86400
  float g = larval_log_f32(__fadd_rn(__fdiv_rn(GR, 100.f), 1.f));
  g = __fdiv_rn(__fmul_rn(g, dt_f), 86400.f);
  return __fmul_rn(w, __fsub_rn(larval_exp_f32(g), 1.f));       // weight * (np.exp(g) - 1.)
}

// length [mm] of a larva of weight w [mg] (:230-231): np.exp(2.296 + 0.277 * np.log(w) - 0.005128 * np.log10(w)**2)
__host__ __device__ __forceinline__ float larval_length_f32(float w) {
  const float l10 = larval_log10_f32(w);
  float x = __fadd_rn(LF(2.296), __fmul_rn(LF(0.277), larval_log_f32(w)));
  x = __fsub_rn(x, __fmul_rn(LF(0.005128), __fmul_rn(l10, l10)));
  return larval_exp_f32(x);
}

// update_fish_larvae (:200-231) of one element.  days_f = float32(time_step.total_seconds() / 86400).  stage and hatched are
// always current on return; weight and length are changed for a larva only (an egg hatched in this call included).
// Returns true when weight and length have to be stored.
__host__ __device__ __forceinline__ bool larval_update_f32(float T, float days_f, float dt_f, float &stage, float &hatched, float &weight,
                                                  float &length) {
  if (hatched == 0.f) {
    // amb_duration = np.exp(3.65 - 0.145*T): total egg development time [days]; stage_fraction += days_in_timestep / amb_duration
    const float duration = larval_exp_f32(__fsub_rn(LF(3.65), __fmul_rn(LF(0.145), T)));
    stage = __fadd_rn(stage, __fdiv_rn(days_f, duration));
    if (stage >= 1.f) hatched = 1.f;
  }
  if (hatched != 1.f) return false;
  weight = __fadd_rn(weight, larval_growth_f32(weight, T, dt_f));
  length = larval_length_f32(weight);
  return true;
}

// (0.261*(L**(1.552*L**(-0.08))) - 5.289/L) / 1000: swimming speed [m/s] of a larva of length L [mm] (:242)
__host__ __device__ __forceinline__ float larval_swim_f32(float L) {
  const float e = __fmul_rn(LF(1.552), larval_pow_f32(L, LF(-0.08)));
  const float s = __fsub_rn(__fmul_rn(LF(0.261), larval_pow_f32(L, e)), __fdiv_rn(LF(5.289), L));
  return __fdiv_rn(s, 1000.f);
}

// larvae_vertical_migration (:233-253) of one larva: the new z.  f = float32(IBM:fraction_of_timestep_swimming),
// direction = -1 (down, hour < 12) or +1
__host__ __device__ __forceinline__ double larval_migrate(double z, float L, float f, float dt_f, float direction) {
  // max_migration_per_timestep = f*swim_speed*self.time_step.total_seconds()
  const float reach = __fmul_rn(__fmul_rn(f, larval_swim_f32(L)), dt_f);
  const double zn = __dadd_rn(z, (double)__fmul_rn(direction, reach));
  return zn < 0.0 ? zn : (zn != zn ? zn : 0.0);       // np.minimum(0, zn): NaN propagates
}
#undef LF

#ifndef ODR_LARVAL_HOST
// one element per thread.  An egg: T, stage_fraction, hatched in, stage_fraction (and hatched when it hatches) out; a larva:
// weight in, weight and length out
__global__ __launch_bounds__(BLOCK) void k_larval_update(long long n, const float *__restrict__ T, float days_f, float dt_f,
                                                       float *__restrict__ stage, float *__restrict__ hatched,
                                                       float *__restrict__ weight, float *__restrict__ length) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float h0 = hatched[i];
  if (h0 != 0.f && h0 != 1.f) return;   // (neither egg nor larva: the reference selects neither)
  float h = h0, s = h0 == 0.f ? stage[i] : 1.f, w = weight[i], L = 0.f;
  if (larval_update_f32(T[i], days_f, dt_f, s, h, w, L)) { weight[i] = w; length[i] = L; }
  if (h0 == 0.f) {
    stage[i] = s;
    if (h != h0) hatched[i] = h;
  }
}

// one element per thread: hatched in; a larva: length and z in, z out
__global__ __launch_bounds__(BLOCK) void k_larval_migrate(long long n, const float *__restrict__ hatched, const float *__restrict__ length,
                                                        float f, float dt_f, float direction, double *__restrict__ z) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (hatched[i] != 1.f) return;
  z[i] = larval_migrate(z[i], length[i], f, dt_f, direction);
}
#endif  // ODR_LARVAL_HOST

}  // namespace odr
