// libodrift_hip.so: PlastDrift's submersion by wind and the parameterisation of absent waves from the wind (Stokes drift and
// significant wave height of Environment.get_environment).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_plast.hip.h"

// Stokes drift and / or wave height of every active element from the sampled wind (models/basemodel/environment.py:844-863,
// models/physics_methods.py:488-568; odr_plast.hip.h).  One launch on the context's stream, no host synchronisation.
int odr_stokes_from_wind(odr_ctx *c, odr_particles *p, const double *stokes_coeff, int n_stokes, const double *hs_coeff, int flags) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(flags > 0 && !(flags & ~(PLAST_STOKES | PLAST_HS)), "flags must be ODR_PLAST_STOKES, ODR_PLAST_HS or both, not %d", flags);
  PlastCoeff C;
  memset(&C, 0, sizeof C);
  if (flags & PLAST_STOKES) {
    REQUIRE(stokes_coeff && n_stokes >= 1 && n_stokes <= PLAST_MAX_COEFF, "1 .. %d coefficients of the drift factor, not %d", PLAST_MAX_COEFF, n_stokes);
    for (int k = 0; k < n_stokes; ++k) C.stokes[k] = stokes_coeff[k];
    C.n_stokes = n_stokes;
  }
  if (flags & PLAST_HS) {
    REQUIRE(hs_coeff, "the two coefficients of the wave height are missing");
    for (int k = 0; k < PLAST_HS_COEFF; ++k) C.hs[k] = hs_coeff[k];
  }
  if (!p->env[VAR_XWIND] || !p->env[VAR_YWIND]) return fail(ODR_ERR_STATE, "x_wind and y_wind must have been sampled");
  int rc;
  if (flags & PLAST_STOKES) {
    if ((rc = ensure_env(c, p, VAR_SX)) || (rc = ensure_env(c, p, VAR_SY))) return rc;
    p->env_cok[VAR_SX] = p->env_cok[VAR_SY] = false;
  }
  if (flags & PLAST_HS) {
    if ((rc = ensure_env(c, p, VAR_HS))) return rc;
    p->env_cok[VAR_HS] = false;
  }
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_stokes_from_wind, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->i32[1], p->env[VAR_XWIND],
                     p->env[VAR_YWIND], p->env[VAR_SX], p->env[VAR_SY], p->env[VAR_HS], C, flags);
  HIPCHK(hipGetLastError());
  return 0;
}

// The plain maxima over the active elements that environment.py:847-858 asks about: out3 = {Stokes x, Stokes y, wave height},
// -inf for a variable that has not been sampled and for a set without active elements.  They are slots of the movers' reduction.
int odr_reduce_wave_maxima(odr_ctx *c, odr_particles *p, double *out3) {
  REQUIRE(c && p && out3, "NULL argument");
  REQUIRE(!c->red_pinned, "a reduction installed over the ranks of a sharded run does not hold the Stokes components");
  int rc = reduce(c, p, 0.1, 0, false, false, false);
  if (rc) return rc;
  double r[R_N];
  D2H(r, c->red, sizeof r);
  out3[0] = r[R_SXMAX]; out3[1] = r[R_SYMAX]; out3[2] = r[R_HSMAX];
  return 0;
}

// PlastDrift.update_particle_depth with vertical_mixing:mixingmodel = 'analytical' (models/plastdrift.py:102-107): z of every
// active element drawn anew, -(K / terminal_velocity) E.  draws (ODR_RNG_HOST): one standard exponential per element of the set.
// Two launches and the read-back of the flag the first one raises: ODR_ERR_INVALID, and no z changed, for a scale NumPy refuses.
int odr_plast_depth(odr_ctx *c, odr_particles *p, int rng_mode, const double *draws, uint64_t step) {
  REQUIRE(c && p, "NULL argument");
  REQUIRE(rng_mode == ODR_RNG_DEVICE || rng_mode == ODR_RNG_HOST, "bad rng_mode %d", rng_mode);
  if (!p->env[VAR_KZ]) return fail(ODR_ERR_STATE, "ocean_vertical_diffusivity must have been sampled");
  if (p->n == 0) return 0;
  double *dd = nullptr;
  if (rng_mode == ODR_RNG_HOST) {
    REQUIRE(draws, "host draws required in ODR_RNG_HOST mode");
    void *s;
    int rc = scratch(c, p, sizeof(double) * (size_t)p->n, &s);
    if (rc) return rc;
    dd = (double *)s;
    H2D(dd, draws, sizeof(double) * (size_t)p->n);
  }
  p->epoch++;  // z changes: invalidates the cached reductions (reduce()) and the step launch's keep ballots
  HIPCHK(hipMemsetAsync(c->counter, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_plast_check, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->i32[1], p->env[VAR_KZ], p->f32[2],
                     c->counter);
  hipLaunchKernelGGL(k_plast_depth, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->i32[1], p->i32[0], p->env[VAR_KZ],
                     p->f32[2], p->d64[2], rng_mode, dd, c->seed, (unsigned long long)step, c->counter);
  HIPCHK(hipGetLastError());
  int64_t refused = 0;
  int rc = read_counter(c, &refused);
  if (rc) return rc;
  if (refused) return fail(ODR_ERR_INVALID, "scale < 0: ocean_vertical_diffusivity / terminal_velocity is negative for an active element");
  return 0;
}
