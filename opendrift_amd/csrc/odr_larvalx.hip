// libodrift_hip.so, a translation unit of its own: the extended larval fish model's own physics
// (LarvalFishExtended.update_fish_larvae, LarvalFishExtended._apply_vertical_behavior) and the solar elevation of the active
// set (OceanDrift.solar_elevation).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_larvalx.hip.h"

// Solar elevation [deg] of every active element into out_host[0 .. n) (models/physics_methods.py:977-979, :1036-1043;
// odr_solar.hip.h).  Waits for the context's stream: the values are in out_host on return.
int odr_solar_elevation(odr_ctx *c, odr_particles *p, double declination_rad, double time_offset_minutes, double day_minutes,
                        double *out_host) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(declination_rad == declination_rad && time_offset_minutes == time_offset_minutes && day_minutes == day_minutes, "NaN argument");
  if (p->n == 0) return 0;
  REQUIRE(out_host, "NULL argument");
  void *buf;
  if (int rc = scratch(c, p, sizeof(double) * (size_t)p->n, &buf)) return rc;
  hipLaunchKernelGGL(k_solar_elevation, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, std::sin(declination_rad),
                     std::cos(declination_rad), time_offset_minutes, day_minutes, p->d64[0], p->d64[1], (double *)buf);
  HIPCHK(hipGetLastError());
  D2H(out_host, buf, sizeof(double) * (size_t)p->n);
  return 0;
}

// Fixed-time hatching of every egg of the active set (models/larvalfish_extended.py:292-318; odr_larvalx.hip.h).  Enqueued on the
// context's stream, no host synchronisation.
int odr_larvalx_hatch(odr_ctx *c, odr_particles *p, int stage_fraction_slot, int hatched_slot, double increment) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(increment == increment, "increment is NaN");
  if (int rc = property_slots(p, {stage_fraction_slot, hatched_slot})) return rc;
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_larvalx_hatch, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, (float)increment,
                     p->aux[stage_fraction_slot], p->aux[hatched_slot]);
  HIPCHK(hipGetLastError());
  return 0;
}

// z of every moving element of the active set after the behaviour step (models/larvalfish_extended.py:206-290;
// odr_larvalx.hip.h).  No host synchronisation.
int odr_larvalx_behave(odr_ctx *c, odr_particles *p, int hatched_slot, int mode, int active_only_hatched, int z_is_float32,
                       double band0_centre, double band0_half_width, double band1_centre, double band1_half_width, double w_active,
                       double dt_seconds, double declination_rad, double time_offset_minutes, double day_minutes) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(mode == ODR_LARVALX_DEPTH || mode == ODR_LARVALX_DVM, "mode is %d, not ODR_LARVALX_DEPTH or ODR_LARVALX_DVM", mode);
  REQUIRE(band0_centre == band0_centre && band0_half_width >= 0.0 && w_active == w_active && dt_seconds == dt_seconds,
          "NaN argument or negative half-width");
  if (mode == ODR_LARVALX_DVM)
    REQUIRE(band1_centre == band1_centre && band1_half_width >= 0.0 && declination_rad == declination_rad &&
            time_offset_minutes == time_offset_minutes && day_minutes == day_minutes, "NaN argument or negative half-width");
  if (!p->env[VAR_DEPTH]) return fail(ODR_ERR_STATE, "sea_floor_depth_below_sea_level has not been sampled");
  if (active_only_hatched)
    if (int rc = property_slots(p, {hatched_slot})) return rc;
  if (!(w_active > 0.0) || !(dt_seconds > 0.0)) return 0;     // :246-247: nothing moves, nothing is clipped
  p->epoch++;  // z changes
  if (p->n == 0) return 0;
  LarvalxBehave B;
  B.band_min[0] = band0_centre - band0_half_width; B.band_max[0] = band0_centre + band0_half_width;
  B.band_min[1] = band1_centre - band1_half_width; B.band_max[1] = band1_centre + band1_half_width;
  B.max_step = w_active * dt_seconds;
  B.sin_d = std::sin(declination_rad); B.cos_d = std::cos(declination_rad);
  B.eqtime = time_offset_minutes; B.day_minutes = day_minutes;
  B.mode = mode == ODR_LARVALX_DVM ? LARVALX_MODE_DVM : LARVALX_MODE_DEPTH;
  B.z_f32 = z_is_float32 != 0; B.only_hatched = active_only_hatched != 0;
  hipLaunchKernelGGL(k_larvalx_behave, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, B,
                     active_only_hatched ? p->aux[hatched_slot] : (const float *)nullptr, p->env[VAR_DEPTH], p->d64[0], p->d64[1], p->d64[2]);
  HIPCHK(hipGetLastError());
  return 0;
}
