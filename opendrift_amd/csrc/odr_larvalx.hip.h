// LarvalFishExtended: eggs hatch after a fixed time; larvae or phytoplankton keep a depth band, or migrate between a day band and
// a night band chosen per element by the solar elevation at its own position.
//
//   LarvalFishExtended.update_fish_larvae          models/larvalfish_extended.py:292-318    larvalx_hatch_f32
//   LarvalFishExtended._compute_band_half_width    models/larvalfish_extended.py:177-186    host, once per band (float64)
//   LarvalFishExtended._target_into_band           models/larvalfish_extended.py:188-200    larvalx_target
//   LarvalFishExtended._apply_vertical_behavior    models/larvalfish_extended.py:206-290    larvalx_behave
//
// Rounding contract.  stage_fraction is a float32 array and days_in_timestep / hatch_time_days a Python float, which NumPy 2
// casts to float32 where it meets the array: stage_fraction += increment is ONE IEEE single addition of float32(increment).
//
// The band centre and its half-width are Python / NumPy float64 scalars, so band_min = centre - half_w and band_max = centre +
// half_w are float64, the comparisons of _target_into_band are float64 comparisons of the widened z, and its result is a float64
// array: z itself inside the band, else the nearer edge.  What follows depends on the dtype z has in the reference, and on the
// mode.  z is a float64 array once the vertical mixing has run, and the float32 the element type declares until then; the
// caller says which (z_f32), as for OpenBerg's latitude.  This file reproduces both:
//   float64 z, either mode: dz = target - z, clip(dz, -max_step, max_step), z + dz_step, min(., 0), max(., -(double)depth) -- one
//     IEEE double operation each (`target_z.astype(z.dtype)` changes nothing);
//   float32 z, mode dvm: `np.where(is_day, ...).astype(z.dtype)` rounds the target to float32; dz, the clip against
//     float32(max_step) and the sum are IEEE single operations;
//   float32 z, mode depth: there is no astype: dz and the clip are float64, `z[idx] += dz_step` rounds the float64 sum to float32
//     once;
//   float32 z, then: min(., 0) and max(., -depth) are float32 comparisons with the float32 sea-floor depth.
// With z_f32 the z of the particle set (always float64 here) is rounded to float32 when it is read -- exact where the run held
// float32 values from the start -- and the float32 result is stored widened.  Day is solar_elevation > 0 with the elevation of
// odr_solar.hip.h.  NaN: np.clip, np.minimum and np.maximum propagate a NaN z, and so does this code; a NaN depth gives NaN.
//
// Only elements that move are written: with active_only_hatched every element whose hatched slot is not 1 keeps its z bits.
//
// Compiled for the CPU by tests/larvalx_host.cpp (the rounding intrinsics are its own there): includes nothing but
// odr_solar.hip.h; the kernels (not part of the host build) take BLOCK from odr_kernels.hip.h, which the translation unit
// includes first.
#pragma once

#include "odr_solar.hip.h"

namespace odr {

enum { LARVALX_STAGE_FRACTION = 0, LARVALX_HATCHED = 1 };   // property slots of the model
enum { LARVALX_MODE_DEPTH = 1, LARVALX_MODE_DVM = 2 };

// What a behaviour launch needs besides the arrays.  Band 0: the depth band (mode depth) or the NIGHT band (mode dvm); band 1: the
// DAY band.  min / max: centre -+ half-width, formed by the host in float64 as the reference forms them.
struct LarvalxBehave {
  double band_min[2], band_max[2];
  double max_step;                          // w_active * dt
  double sin_d, cos_d, eqtime, day_minutes; // odr_solar.hip.h
  int mode, z_f32, only_hatched;
};

// update_fish_larvae (:292-318) of one egg: stage_fraction += float32(increment); returns true when it hatches
__host__ __device__ __forceinline__ bool larvalx_hatch_f32(float &stage, float increment_f) {
  stage = __fadd_rn(stage, increment_f);
  return stage >= 1.f;
}

// _target_into_band (:188-200): float64
__host__ __device__ __forceinline__ double larvalx_target(double z, double band_min, double band_max) {
  return (z >= band_min && z <= band_max) ? z : (z < band_min ? band_min : band_max);
}

__host__ __device__ __forceinline__ double larvalx_clip_f64(double x, double lo, double hi) {   // np.clip: NaN propagates
  return x < lo ? lo : (x > hi ? hi : x);
}
__host__ __device__ __forceinline__ float larvalx_clip_f32(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// _apply_vertical_behavior (:206-290) of one moving element: the new z.  day: solar_elevation > 0 (mode dvm only)
__host__ __device__ __forceinline__ double larvalx_behave(double z, float depth, bool day, const LarvalxBehave &B) {
  const int b = (B.mode == LARVALX_MODE_DVM && day) ? 1 : 0;
  if (!B.z_f32) {
    const double dz = __dsub_rn(larvalx_target(z, B.band_min[b], B.band_max[b]), z);
    double zn = __dadd_rn(z, larvalx_clip_f64(dz, -B.max_step, B.max_step));
    zn = zn > 0.0 ? 0.0 : zn;                                       // np.minimum(z, 0.0)
    const double bottom = -(double)depth;
    return (zn < bottom || bottom != bottom) ? bottom : zn;         // np.maximum(z, bottom)
  }
  const float zf = (float)z;
  const double target = larvalx_target((double)zf, B.band_min[b], B.band_max[b]);
  float zn;
  if (B.mode == LARVALX_MODE_DVM) {
    const float m = (float)B.max_step;
    zn = __fadd_rn(zf, larvalx_clip_f32(__fsub_rn((float)target, zf), -m, m));
  } else {
    zn = (float)__dadd_rn((double)zf, larvalx_clip_f64(__dsub_rn(target, (double)zf), -B.max_step, B.max_step));
  }
  zn = zn > 0.f ? 0.f : zn;
  const float bottom = -depth;
  return (double)((zn < bottom || bottom != bottom) ? bottom : zn);
}

#ifndef ODR_LARVALX_HOST
// one element per thread: hatched in; an egg: stage_fraction in and out, hatched out when it hatches
__global__ __launch_bounds__(BLOCK) void k_larvalx_hatch(long long n, float increment_f, float *__restrict__ stage, float *__restrict__ hatched) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (hatched[i] != 0.f) return;
  float s = stage[i];
  const bool h = larvalx_hatch_f32(s, increment_f);
  stage[i] = s;
  if (h) hatched[i] = 1.f;
}

// one element per thread: hatched (larva case), z and depth in, with mode dvm lon and lat too; z out
__global__ __launch_bounds__(BLOCK) void k_larvalx_behave(long long n, LarvalxBehave B, const float *__restrict__ hatched,
                                                         const float *__restrict__ depth, const double *__restrict__ lon,
                                                         const double *__restrict__ lat, double *__restrict__ z) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (B.only_hatched && hatched[i] != 1.f) return;
  bool day = false;
  if (B.mode == LARVALX_MODE_DVM) day = solar_elevation_deg(lon[i], lat[i], B.sin_d, B.cos_d, B.eqtime, B.day_minutes) > 0.0;
  z[i] = larvalx_behave(z[i], depth[i], day, B);
}

// one element per thread: lon and lat in, the elevation [deg] out
__global__ __launch_bounds__(BLOCK) void k_solar_elevation(long long n, double sin_d, double cos_d, double eqtime, double day_minutes,
                                                          const double *__restrict__ lon, const double *__restrict__ lat,
                                                          double *__restrict__ out) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = solar_elevation_deg(lon[i], lat[i], sin_d, cos_d, eqtime, day_minutes);
}
#endif  // ODR_LARVALX_HOST

}  // namespace odr
