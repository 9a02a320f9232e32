// libodrift_hip.so, a translation unit of its own: the radionuclide model's own physics (RadionuclideDrift.update_speciation,
// update_terminal_velocity, resuspension).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_radio.hip.h"

struct odr_radio {
  RadioSetup S;
  double *table;                 // device: [4][7][7] transfer rates, zero where the setup has none
  unsigned long long *counts;    // device: [7][7] transformations in -> out, [49] elements whose species number is outside the table
};

static int radio_species_ok(int v, int nspecies, bool required, const char *name) {
  if (v == -1 && !required) return 0;
  REQUIRE(v >= 0 && v < nspecies, "species number of '%s' is %d, outside 0 .. %d", name, v, nspecies - 1);
  return 0;
}

int odr_radio_create(odr_ctx *c, const odr_radio_setup *s, odr_radio **out) {
  REQUIRE(c && s && out, "NULL argument");
  REQUIRE(s->nspecies >= 1 && s->nspecies <= RADIO_MAXSP, "nspecies is %d, not 1 .. %d", s->nspecies, RADIO_MAXSP);
  REQUIRE(s->nsalinity == 1 || s->nsalinity == RADIO_MAXSAL, "nsalinity is %d, not 1 or %d", s->nsalinity, RADIO_MAXSAL);
  REQUIRE((s->lmm >= 0) != (s->lmmcation >= 0), "a setup has either LMM or LMMcation");
  REQUIRE(s->lmm < 0 || s->nsalinity == 1, "the salinity intervals belong to the LMMcation setup");
  const bool al = s->lmmcation >= 0;
  int rc = 0;
  if ((rc = radio_species_ok(s->lmm, s->nspecies, !al, "LMM")) || (rc = radio_species_ok(s->lmmcation, s->nspecies, al, "LMMcation")) ||
      (rc = radio_species_ok(s->lmmanion, s->nspecies, al, "LMManion")) || (rc = radio_species_ok(s->polymer, s->nspecies, al, "Polymer")) ||
      (rc = radio_species_ok(s->particle_rev, s->nspecies, true, "Particle reversible")) ||
      (rc = radio_species_ok(s->sediment_rev, s->nspecies, true, "Sediment reversible")) ||
      (rc = radio_species_ok(s->particle_slow, s->nspecies, false, "Particle slowly reversible")) ||
      (rc = radio_species_ok(s->sediment_slow, s->nspecies, s->particle_slow >= 0, "Sediment slowly reversible")) ||
      (rc = radio_species_ok(s->particle_irrev, s->nspecies, false, "Particle irreversible")) ||
      (rc = radio_species_ok(s->sediment_irrev, s->nspecies, s->particle_irrev >= 0, "Sediment irreversible")))
    return rc;
  std::vector<double> t((size_t)RADIO_MAXSAL * RADIO_NBINS, 0.0);
  for (int a = 0; a < s->nsalinity; ++a)
    for (int i = 0; i < s->nspecies; ++i)
      for (int j = 0; j < s->nspecies; ++j) {
        const double k = s->rates[(a * RADIO_MAXSP + i) * RADIO_MAXSP + j];
        REQUIRE(k >= 0 && std::isfinite(k), "transfer rate [%d][%d][%d] is not a finite number >= 0", a, i, j);
        t[(size_t)(a * RADIO_MAXSP + i) * RADIO_MAXSP + j] = k;
      }
  for (double v : {s->layer_thick, s->particle_diameter, s->dissolved_diameter, s->diameter_uncertainty, s->desorption_depth,
                   s->desorption_depth_uncert, s->resuspension_depth, s->resuspension_depth_uncert, s->resuspension_critvel})
    REQUIRE(v == v, "NaN in the setup");
  odr_radio *r = new odr_radio();
  RadioSetup &S = r->S;
  S.dt = 0.0;
  S.layer_thick = s->layer_thick; S.dia_part = s->particle_diameter; S.dia_diss = s->dissolved_diameter;
  S.dia_uncert = s->diameter_uncertainty; S.desorb_std = s->desorption_depth_uncert; S.resusp_std = s->resuspension_depth_uncert;
  S.desorb_depth = (float)s->desorption_depth; S.resusp_depth = (float)s->resuspension_depth; S.critvel = (float)s->resuspension_critvel;
  S.nspecies = s->nspecies; S.nsal = s->nsalinity; S.lognormal = s->lognormal ? 1 : 0;
  S.lmm = s->lmm; S.lmmcation = s->lmmcation; S.lmmanion = s->lmmanion; S.polymer = s->polymer;
  S.prev = s->particle_rev; S.srev = s->sediment_rev; S.psrev = s->particle_slow; S.ssrev = s->sediment_slow;
  S.pirrev = s->particle_irrev; S.sirrev = s->sediment_irrev;
  r->table = nullptr; r->counts = nullptr;
  auto drop = [&](int code) { (void)hipFree(r->table); (void)hipFree(r->counts); delete r; return code; };
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc((void **)&r->table, sizeof(double) * t.size()) != hipSuccess ||
      hipMalloc((void **)&r->counts, sizeof(unsigned long long) * (RADIO_NBINS + 1)) != hipSuccess)
    return drop(fail(ODR_ERR_HIP, "allocating the radionuclide tables failed"));
  if (int rc2 = odr_i_h2d(c, r->table, t.data(), sizeof(double) * t.size(), c->stream)) return drop(rc2);
  if (hipMemsetAsync(r->counts, 0, sizeof(unsigned long long) * (RADIO_NBINS + 1), c->stream) != hipSuccess)
    return drop(fail(ODR_ERR_HIP, "clearing the radionuclide counters failed"));
  *out = r;
  return 0;
}

int odr_radio_destroy(odr_ctx *c, odr_radio *r) {
  REQUIRE(c, "NULL argument");
  if (!r) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));      // a launch that reads it may be in flight
  HIPCHK(hipFree(r->table));
  HIPCHK(hipFree(r->counts));
  delete r;
  return 0;
}

// counts[in * 7 + out] since odr_radio_create (or the last reset).  Waits for the context's stream.
int odr_radio_counts(odr_ctx *c, odr_radio *r, int64_t *counts49, int reset) {
  REQUIRE(c && r && counts49, "NULL argument");
  unsigned long long h[RADIO_NBINS + 1];
  D2H(h, r->counts, sizeof h);
  if (reset) HIPCHK(hipMemsetAsync(r->counts, 0, sizeof h, c->stream));
  for (int k = 0; k < RADIO_NBINS; ++k) counts49[k] = (int64_t)h[k];
  if (h[RADIO_NBINS])
    return fail(ODR_ERR_STATE, "%llu element-launches met a species number outside the table of %d species (they were left unchanged)",
                h[RADIO_NBINS], r->S.nspecies);
  return 0;
}

// the caller's draws (ODR_RNG_HOST) behind each other in the particle set's scratch buffer
static int radio_draws(odr_ctx *c, odr_particles *p, std::initializer_list<const double *> host, RadioDraws &H) {
  const size_t n = (size_t)p->n;
  void *s;
  if (int rc = scratch(c, p, sizeof(double) * n * host.size(), &s)) return rc;
  double *d = (double *)s;
  const double **dst[4] = {&H.u1, &H.u2, &H.diam, &H.depth};
  int k = 4 - (int)host.size();     // (two arrays: the two normals)
  for (const double *h : host) {
    REQUIRE(h, "host draws required in ODR_RNG_HOST mode");
    H2D(d, h, sizeof(double) * n);
    *dst[k++] = d;
    d += n;
  }
  return 0;
}

// update_transfer_rates + update_speciation with the diameter, sorption and desorption updates (models/radionuclides.py:728-860,
// :866-902; odr_radio.hip.h).  Enqueued on the context's stream; no host synchronisation in ODR_RNG_DEVICE mode.
int odr_radio_speciation(odr_ctx *c, odr_particles *p, odr_radio *r, int specie_slot, int diameter_slot, int32_t conc3_var,
                         double dt_seconds, int rng_mode, const double *u1, const double *u2, const double *diameter_noise,
                         const double *depth_noise, uint64_t step) {
  REQUIRE(c && p && r, "NULL argument");
  REQUIRE(dt_seconds == dt_seconds, "dt_seconds is NaN");
  REQUIRE(rng_mode == ODR_RNG_DEVICE || rng_mode == ODR_RNG_HOST, "unknown rng_mode %d", rng_mode);
  REQUIRE(conc3_var >= 0 && conc3_var < NVAR, "bad variable id %d for conc3", (int)conc3_var);
  if (int rc = property_slots(p, {specie_slot, diameter_slot})) return rc;
  if (!p->env[VAR_DEPTH]) return fail(ODR_ERR_STATE, "sea_floor_depth_below_sea_level must have been sampled");
  if (r->S.lmm >= 0 && !p->env[conc3_var]) return fail(ODR_ERR_STATE, "conc3 (variable slot %d) must have been sampled", (int)conc3_var);
  if (r->S.nsal > 1 && !p->env[VAR_SALT]) return fail(ODR_ERR_STATE, "sea_water_salinity must have been sampled");
  p->epoch++;  // z and properties change
  if (p->n == 0) return 0;
  RadioDraws H = {nullptr, nullptr, nullptr, nullptr};
  if (rng_mode == ODR_RNG_HOST)
    if (int rc = radio_draws(c, p, {u1, u2, diameter_noise, depth_noise}, H)) return rc;
  RadioSetup S = r->S;
  S.dt = dt_seconds;
  const RadioView V = {p->aux[specie_slot], p->aux[diameter_slot], p->i32[2], p->d64[2], p->env[VAR_SALT], p->env[VAR_DEPTH],
                       p->env[conc3_var], p->env[VAR_U], p->env[VAR_V]};
  hipLaunchKernelGGL(k_radio_speciation, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, S, r->table, V, p->i32[0], rng_mode,
                     H, c->seed, (unsigned long long)step, r->counts);
  HIPCHK(hipGetLastError());
  return 0;
}

// elements.terminal_velocity of every active element: Stokes' law from the sampled temperature and salinity and the element's
// diameter and density, times moving (models/radionuclides.py:665-721 without profiles).  No host synchronisation.
int odr_radio_terminal_velocity(odr_ctx *c, odr_particles *p, int diameter_slot, int density_slot) {
  REQUIRE(c && p, "NULL argument");
  if (int rc = property_slots(p, {diameter_slot, density_slot})) return rc;
  if (!p->env[VAR_TEMP] || !p->env[VAR_SALT])
    return fail(ODR_ERR_STATE, "sea_water_temperature and sea_water_salinity must have been sampled");
  p->epoch++;  // invalidates the cached reductions (reduce())
  if (p->n == 0) return 0;
  hipLaunchKernelGGL(k_radio_terminal_velocity, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, p->env[VAR_TEMP],
                     p->env[VAR_SALT], p->aux[diameter_slot], p->aux[density_slot], p->i32[2], p->f32[2]);
  HIPCHK(hipGetLastError());
  return 0;
}

// bottom_interaction's change of species for the elements the sea-floor action settled, then resuspension
// (models/radionuclides.py:912-942, :946-997).  No host synchronisation in ODR_RNG_DEVICE mode.
int odr_radio_resuspend(odr_ctx *c, odr_particles *p, odr_radio *r, int specie_slot, int diameter_slot, int rng_mode,
                        const double *diameter_noise, const double *depth_noise, uint64_t step) {
  REQUIRE(c && p && r, "NULL argument");
  REQUIRE(rng_mode == ODR_RNG_DEVICE || rng_mode == ODR_RNG_HOST, "unknown rng_mode %d", rng_mode);
  if (int rc = property_slots(p, {specie_slot, diameter_slot})) return rc;
  if (!p->env[VAR_U] || !p->env[VAR_V])
    return fail(ODR_ERR_STATE, "x_sea_water_velocity and y_sea_water_velocity must have been sampled");
  if (!p->env[VAR_DEPTH]) return fail(ODR_ERR_STATE, "sea_floor_depth_below_sea_level must have been sampled");
  p->epoch++;  // z, moving and properties change
  if (p->n == 0) return 0;
  RadioDraws H = {nullptr, nullptr, nullptr, nullptr};
  if (rng_mode == ODR_RNG_HOST)
    if (int rc = radio_draws(c, p, {diameter_noise, depth_noise}, H)) return rc;
  const RadioView V = {p->aux[specie_slot], p->aux[diameter_slot], p->i32[2], p->d64[2], nullptr, p->env[VAR_DEPTH], nullptr,
                       p->env[VAR_U], p->env[VAR_V]};
  hipLaunchKernelGGL(k_radio_resuspend, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, (long long)p->n, r->S, V, p->i32[0], rng_mode, H,
                     c->seed, (unsigned long long)step, r->counts);
  HIPCHK(hipGetLastError());
  return 0;
}
