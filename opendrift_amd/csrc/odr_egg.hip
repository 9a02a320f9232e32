// libodrift_hip.so, translation unit 10: the pelagic egg model's own physics (PelagicEggDrift.update_terminal_velocity).
// See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_egg.hip.h"

// elements.terminal_velocity of every active element from the sampled temperature and salinity and two property slots
// (models/pelagicegg.py:100-179; odr_egg.hip.h).  Enqueued on the context's stream, no host synchronisation.
int odr_egg_terminal_velocity(odr_ctx *c, odr_particles *p, int diameter_slot, int salinity_slot) {
  REQUIRE(c && p, "NULL argument");
  if (int rc = property_slots(p, {diameter_slot, salinity_slot})) return rc;
  if (!p->env[VAR_TEMP] || !p->env[VAR_SALT])
    return fail(ODR_ERR_STATE, "sea_water_temperature and sea_water_salinity must have been sampled");
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_egg_terminal_velocity, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->env[VAR_TEMP],
                     p->env[VAR_SALT], p->aux[diameter_slot], p->aux[salinity_slot], p->f32[2]);
  HIPCHK(hipGetLastError());
  return 0;
}
