// libodrift_hip.so, a translation unit of its own: the larval fish model's own physics (LarvalFish.update_fish_larvae,
// LarvalFish.larvae_vertical_migration).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_larval.hip.h"

// Hatching, growth and length of every active element from the sampled temperature and four property slots
// (models/larvalfish.py:185-231; odr_larval.hip.h).  Enqueued on the context's stream, no host synchronisation.
int odr_larval_update(odr_ctx *c, odr_particles *p, int stage_fraction_slot, int hatched_slot, int weight_slot, int length_slot,
                      double dt_seconds) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(dt_seconds == dt_seconds, "dt_seconds is NaN");
  if (!p->env[VAR_TEMP]) return fail(ODR_ERR_STATE, "sea_water_temperature must have been sampled");
  if (int rc = property_slots(p, {stage_fraction_slot, hatched_slot, weight_slot, length_slot})) return rc;
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_larval_update, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->env[VAR_TEMP],
                     larval_days_in_timestep_f32(dt_seconds), (float)dt_seconds, p->aux[stage_fraction_slot], p->aux[hatched_slot],
                     p->aux[weight_slot], p->aux[length_slot]);
  HIPCHK(hipGetLastError());
  return 0;
}

// z of every larva (hatched == 1) of the active set after swimming for fraction_swimming of the time step, up (direction +1)
// or down (-1), not above the surface (models/larvalfish.py:233-253; odr_larval.hip.h).  No host synchronisation.
int odr_larval_migrate(odr_ctx *c, odr_particles *p, int hatched_slot, int length_slot, double fraction_swimming, double dt_seconds,
                       int direction) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(dt_seconds == dt_seconds && fraction_swimming == fraction_swimming, "NaN argument");
  REQUIRE(direction == 1 || direction == -1, "direction is %d, not +1 or -1", direction);
  if (int rc = property_slots(p, {hatched_slot, length_slot})) return rc;
  p->epoch++;  // z changes
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_larval_migrate, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->aux[hatched_slot],
                     p->aux[length_slot], (float)fraction_swimming, (float)dt_seconds, (float)direction, p->d64[2]);
  HIPCHK(hipGetLastError());
  return 0;
}
