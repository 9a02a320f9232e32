// libodrift_hip.so, translation unit 11: the sediment model's own step (SedimentDrift.resuspension).
// See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_sediment.hip.h"

// Settled elements (moving == 0) of the active set whose sampled current speed exceeds `threshold` move again, 1 cm above
// where they lay (models/sedimentdrift.py:118-126; odr_sediment.hip.h).  Enqueued on the context's stream; the host waits
// only when it asks for the count (n_resuspended != NULL).
int odr_resuspend(odr_ctx *c, odr_particles *p, float threshold, int64_t *n_resuspended) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(threshold == threshold, "threshold is NaN");
  if (n_resuspended) *n_resuspended = 0;
  if (!p->env[VAR_U] || !p->env[VAR_V])
    return fail(ODR_ERR_STATE, "x_sea_water_velocity and y_sea_water_velocity must have been sampled");
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  if (n_resuspended) HIPCHK(hipMemsetAsync(c->counter, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_resuspend, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->env[VAR_U], p->env[VAR_V],
                     threshold, p->i32[2], p->d64[2], n_resuspended ? c->counter : nullptr);
  HIPCHK(hipGetLastError());
  return read_counter(c, n_resuspended);
}
