// libodrift_hip.so, a translation unit of its own: the iceberg model's own physics (OpenBerg.roll_over, OpenBerg.advect_iceberg
// with SciPy's RK45 over the active set).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_berg.hip.h"

// length, width, sail and draft of every active element after the stability test of Wagner et al. (models/openberg.py:587-614;
// odr_berg.hip.h).  Enqueued on the context's stream, no host synchronisation.
int odr_berg_roll_over(odr_ctx *c, odr_particles *p, int sail_slot, int draft_slot, int length_slot, int width_slot) {
  REQUIRE(c && p, "NULL argument");
  if (int rc = property_slots(p, {sail_slot, draft_slot, length_slot, width_slot}, 4)) return rc;
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_berg_roll_over, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->aux[sail_slot], p->aux[draft_slot],
                     p->aux[length_slot], p->aux[width_slot]);
  HIPCHK(hipGetLastError());
  return 0;
}

namespace {
// berg_solve's backend on the device: one launch per evaluation of all elements, one fold launch, one value read back
struct BergDevice {
  odr_ctx *c;
  long long n;
  unsigned nb;
  BergScratch S;
  BergState y, o;
  int read(int m, double *out) {
    hipLaunchKernelGGL(k_berg_fold, dim3(m), dim3(BLOCK), 0, c->stream, S.part, (long long)nb, S.sum);
    HIPCHK(hipGetLastError());
    D2H(out, S.sum, sizeof(double) * (size_t)m);
    return 0;
  }
  int norms0(double s[2]) { return read(2, s); }      // the prepare launch left both sets of partials
  int probe(double h0, double &s) {
    hipLaunchKernelGGL(k_berg_probe, dim3(nb), dim3(BLOCK), 0, c->stream, n, h0, S, y);
    HIPCHK(hipGetLastError());
    return read(1, &s);
  }
  int attempt(double h, double &s) {
    hipLaunchKernelGGL(k_berg_attempt, dim3(nb), dim3(BLOCK), 0, c->stream, n, h, S, y, o);
    HIPCHK(hipGetLastError());
    return read(1, &s);
  }
  void accept() { std::swap(y, o); }
};
}  // namespace

// OpenBerg.advect_iceberg with surface currents (models/openberg.py:427-552, the forces :104-218): prepare, SciPy's RK45 over the
// velocity vector of the whole active set (one read-back of the error norm per attempt), finish.  Synchronises with the host.
// A failed solve leaves the call partly applied: `moving` is grounded / degrounded by the prepare launch and the epoch is bumped;
// positions and the velocity slots are untouched.
int odr_berg_advect(odr_ctx *c, odr_particles *p, int sail_slot, int draft_slot, int length_slot, int width_slot, int x_velocity_slot,
                    int y_velocity_slot, double weight_coef, double water_form_drag_coef, double water_skin_drag_coef,
                    double wind_form_drag_coef, double wind_skin_drag_coef, double wave_drag_coef, double wave_from_direction,
                    double sea_ice_thickness, int wave_rad, int stokes_drift, int coriolis, int grounding, int lat_is_float32,
                    double dt_seconds, int32_t *n_attempts, int32_t *n_rejected, double *velocity_f64) {
  REQUIRE(c && p, "NULL argument");
  const double scalars[] = {weight_coef, water_form_drag_coef, water_skin_drag_coef, wind_form_drag_coef, wind_skin_drag_coef, wave_drag_coef,
                            wave_from_direction, sea_ice_thickness, dt_seconds};
  for (double s : scalars) REQUIRE(s == s, "NaN argument");
  REQUIRE(dt_seconds > 0, "dt_seconds is %g, not positive", dt_seconds);
  if (!p->env[VAR_U] || !p->env[VAR_V]) return fail(ODR_ERR_STATE, "the current (x_sea_water_velocity, y_sea_water_velocity) must have been sampled");
  if (!p->env[VAR_XWIND] || !p->env[VAR_YWIND]) return fail(ODR_ERR_STATE, "the wind (x_wind, y_wind) must have been sampled");
  if (stokes_drift && (!p->env[VAR_SX] || !p->env[VAR_SY])) return fail(ODR_ERR_STATE, "the Stokes drift must have been sampled when stokes_drift is set");
  if (int rc = property_slots(p, {sail_slot, draft_slot, length_slot, width_slot, x_velocity_slot, y_velocity_slot}, 4)) return rc;
  if (n_attempts) *n_attempts = 0;
  if (n_rejected) *n_rejected = 0;
  p->epoch++;  // positions, moving and two properties change
  if (p->n == 0) return 0;
  for (int k : {x_velocity_slot, y_velocity_slot})
    if (!p->aux[k]) {
      HIPCHK(hipMalloc((void **)&p->aux[k], sizeof(float) * (size_t)p->cap));
      HIPCHK(hipMemsetAsync(p->aux[k], 0, sizeof(float) * (size_t)p->cap, c->stream));
      p->aux_user |= 1u << k;
    }

  // the scratch of the call: 7 + 8 float64 arrays, 6 float32 arrays and one int32 array over the elements, 2 x nb partials, 2 sums
  const size_t n = (size_t)p->n, n8 = (n + 1) & ~(size_t)1;      // (float / int arrays padded to 8 bytes)
  const unsigned nb = nblk(p->n);
  void *base;
  if (int rc = scratch(c, p, sizeof(double) * (15 * n + 2 * (size_t)nb + 2) + 4 * 7 * n8, &base)) return rc;
  BergDevice be;
  be.c = c; be.n = p->n; be.nb = nb;
  double *d = (double *)base;
  BergScratch &S = be.S;
  S.mass = d; S.drag_o = d + n; S.drag_a = d + 2 * n; S.wave_x = d + 3 * n; S.wave_y = d + 4 * n; S.mf = d + 5 * n; S.ice_c = d + 6 * n;
  be.y = {d + 7 * n, d + 8 * n, d + 9 * n, d + 10 * n};
  be.o = {d + 11 * n, d + 12 * n, d + 13 * n, d + 14 * n};
  S.part = d + 15 * n; S.sum = S.part + 2 * (size_t)nb;
  float *f = (float *)(S.sum + 2);
  S.wu = f; S.wv = f + n8; S.au = f + 2 * n8; S.av = f + 3 * n8; S.iu = f + 4 * n8; S.iv = f + 5 * n8;
  S.cls = (int *)(f + 6 * n8);

  BergCall C;
  C.k = {weight_coef, water_form_drag_coef, water_skin_drag_coef, wind_form_drag_coef, wind_skin_drag_coef, wave_drag_coef};
  berg_wave_direction_f32(wave_from_direction, C.wave_sin, C.wave_cos);
  C.ice_thickness = (float)sea_ice_thickness;
  C.wave_rad = wave_rad != 0; C.stokes = stokes_drift != 0; C.coriolis = coriolis != 0; C.grounding = grounding != 0;
  C.lat_f32 = lat_is_float32 != 0;
  const BergEnvPtr e = {p->env[VAR_U], p->env[VAR_V], p->env[VAR_SX], p->env[VAR_SY], p->env[VAR_XWIND], p->env[VAR_YWIND], p->env[VAR_DEPTH],
                        p->env[VAR_SSH], p->env[VAR_HS], p->env[VAR_ICE_A], p->env[VAR_ICE_U], p->env[VAR_ICE_V]};
  hipLaunchKernelGGL(k_berg_prepare, dim3(nb), dim3(BLOCK), 0, c->stream, (long long)p->n, C, e, p->d64[1], p->aux[sail_slot], p->aux[draft_slot],
                     p->aux[length_slot], p->aux[width_slot], p->i32[2], S, be.y);
  HIPCHK(hipGetLastError());

  BergSolveStat st;
  if (int rc = berg_solve(be, (long long)p->n, dt_seconds, st)) return rc;
  if (n_attempts) *n_attempts = st.attempts;
  if (n_rejected) *n_rejected = st.rejected;
  if (st.why == BERG_SOLVE_NOT_FINITE)
    return fail(ODR_ERR_STATE, "iceberg velocities: the error norm is not finite (%g) at t = %g s after %d attempts", st.norm, st.t, st.attempts);
  if (st.why == BERG_SOLVE_STEP_TOO_SMALL)
    return fail(ODR_ERR_STATE, "iceberg velocities: the step size %g s fell below the smallest step at t = %g s after %d attempts", st.h, st.t,
                st.attempts);
  if (st.why == BERG_SOLVE_TOO_MANY)
    return fail(ODR_ERR_STATE, "iceberg velocities: more than %d attempts (t = %g s of %g s, step size %g s)", BERG_MAX_ATTEMPTS, st.t, dt_seconds,
                st.h);

  hipLaunchKernelGGL(k_berg_finish, dim3(nb), dim3(BLOCK), 0, c->stream, view(p), dt_seconds, S.cls, be.y, p->aux[x_velocity_slot],
                     p->aux[y_velocity_slot]);
  HIPCHK(hipGetLastError());
  if (velocity_f64) {      // (the finish launch wrote the velocities it moved with back into y)
    D2H(velocity_f64, be.y.yx, sizeof(double) * n);
    D2H(velocity_f64 + n, be.y.yy, sizeof(double) * n);
  }
  return 0;
}
