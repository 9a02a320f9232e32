// libodrift_hip.so, a translation unit of its own: OpenOil's NOAA oil weathering (odr_weather.hip.h) on a side table the particle
// set owns.  The table is indexed by element ID through the set's id array, like the reference's noaa_mass_balance
// ['mass_components'] (openoil.py:682-693): compaction, the spatial re-sort and the property slots never see it.
#include "odr_host.h"
#include "odr_weather.hip.h"

struct odr_weather {
  WeatherOil O;
  long long n_total;
  double *K;         // device [4][OIL_MAXCOMP]: the component constants
  double *rec;       // device [n_total][WS_N]: the element records
  double *mc;        // device [n_total][O.stride]: mass_components
  double *red;       // device [WR_N]: the reduction in front of the last step; behind it [8]: the last budget
  double *part;      // device [nblk(cap + dead_cap)][8]: per-workgroup partials of either fold
};

static const char *const WS_NAMES[WS_N] = {"mass_oil", "mass_evaporated", "mass_dispersed", "mass_biodegraded", "fraction_evaporated",
                                           "water_fraction", "interfacial_area", "density", "viscosity", "bulltime",
                                           "biodegradation_half_time_droplet", "biodegradation_half_time_slick", "oil_film_thickness", nullptr};

void odr_i_weather_release(odr_particles *p) {
  odr_weather *w = p->weather;
  if (!w) return;
  (void)hipFree(w->K); (void)hipFree(w->rec); (void)hipFree(w->mc); (void)hipFree(w->red); (void)hipFree(w->part);
  delete w;
  p->weather = nullptr;
}

// ------------------------------------------------------------------ kernels
// folds the BLOCK vectors of a workgroup in a fixed order (a tree over the thread index); thread 0 ends with the result in sh[0]
template <class Fold>
__device__ __forceinline__ void weather_block_fold(double (*sh)[8], const double *v, Fold fold) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[t][k] = v[k];
  __syncthreads();
  for (int h = BLOCK / 2; h > 0; h >>= 1) {
    if (t < h) fold(sh[t], sh[t + h]);
    __syncthreads();
  }
}
struct WeatherSum8 {
  __device__ __forceinline__ void operator()(double *a, const double *b) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += b[k];
  }
};
struct WeatherFlagFold {
  __device__ __forceinline__ void operator()(double *a, const double *b) const { weather_fold(a, b); }
};

__device__ __forceinline__ WeatherIn weather_in(long long i, const double *z, const float *age, const float *xw, const float *yw,
                                                const float *temp, const float *hs, const float *tp) {
  WeatherIn E;
  E.xwind = xw[i]; E.ywind = yw[i]; E.temp = temp[i]; E.hs = hs ? hs[i] : 0.f; E.tp = tp ? tp[i] : 0.f;
  E.z = z[i]; E.age = (double)age[i];
  return E;
}

// the call-wide decisions of one step from the state in front of it: per-workgroup partials ...
__global__ __launch_bounds__(BLOCK) void k_weather_reduce(long long n, long long n_total, WeatherOil O, int flags, const int *id, const double *z,
                                                          const float *age, const float *xw, const float *yw, const float *temp,
                                                          const float *hs, const float *tp, const double *rec, double *part) {
  __shared__ double sh[BLOCK][8];
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  double v[WR_N];
  weather_reduce_init(v);
  if (i < n) {
    const long long e = id[i];
    if (e >= 0 && e < n_total) {
      const double *r = rec + e * WS_N;
      double s[WS_N];
#pragma unroll
      for (int k = 0; k < WS_N; ++k) s[k] = k == WS_MASS_OIL || k == WS_MASS_EVAPORATED || k == WS_FRACTION_EVAPORATED ? r[k] : 0.;
      weather_reduce_element(O, weather_in(i, z, age, xw, yw, temp, hs, tp), flags, s, v);
    }
  }
  weather_block_fold(sh, v, WeatherFlagFold());
  if (threadIdx.x < 8) part[(size_t)blockIdx.x * 8 + threadIdx.x] = sh[0][threadIdx.x];
}
// ... folded by one workgroup, partial after partial in index order per thread, then the tree
template <class Fold, bool FLAGS>
__global__ __launch_bounds__(BLOCK) void k_weather_fold(int nparts, const double *part, double *out) {
  __shared__ double sh[BLOCK][8];
  double v[8];
  if (FLAGS) weather_reduce_init(v);
  else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.;
  }
  for (int b = threadIdx.x; b < nparts; b += BLOCK) Fold()(v, part + (size_t)b * 8);
  weather_block_fold(sh, v, Fold());
  if (threadIdx.x < 8) out[threadIdx.x] = sh[0][threadIdx.x];
}

// one step of every active element: Kelvin conversion, property update, evaporation, emulsification, dispersion, biodegradation
__global__ __launch_bounds__(BLOCK) void k_weather(long long n, long long n_total, WeatherOil O, const double *Kg, const double *Rg, int flags,
                                                   double dt, const int *id, const double *z, const float *age, const float *xw,
                                                   const float *yw, const float *temp, const float *hs, const float *tp, double *rec,
                                                   double *mc, float *aux_density, float *aux_viscosity) {
  __shared__ double K[4 * OIL_MAXCOMP];
  __shared__ double R[WR_N];
  for (int t = threadIdx.x; t < 4 * OIL_MAXCOMP; t += BLOCK) K[t] = Kg[t];
  if (threadIdx.x < WR_N) R[threadIdx.x] = Rg[threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const long long e = id[i];
  if (e < 0 || e >= n_total) return;       // an element without a row: left alone (odr_oil_weather has checked the IDs it can)
  double *r = rec + e * WS_N;
  double s[WS_N];
#pragma unroll
  for (int k = 0; k < WS_N; ++k) s[k] = r[k];
  weather_element(O, K, R, flags, dt, weather_in(i, z, age, xw, yw, temp, hs, tp), s, mc + e * O.stride);
#pragma unroll
  for (int k = 0; k <= WS_VISCOSITY; ++k) r[k] = s[k];
  // the mixing kernels read density and viscosity as float32 properties
  aux_density[i] = (float)s[WS_DENSITY];
  aux_viscosity[i] = (float)s[WS_VISCOSITY];
}

// get_oil_budget's sums over the active elements [0, n) and the deactivated store [n, n + ndead):
// surface, submerged, stranded, evaporated, dispersed, biodegraded, (unused), elements counted
__global__ __launch_bounds__(BLOCK) void k_weather_budget(long long n, long long ndead, long long n_total, int stranded_code, const int *id,
                                                          const int *status, const double *z, const int *dead_id, const int *dead_status,
                                                          const double *dead_z, const double *rec, double *part) {
  __shared__ double sh[BLOCK][8];
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  double v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = 0.;
  if (i < n + ndead) {
    const bool live = i < n;
    const long long j = live ? i : i - n;
    const long long e = live ? id[j] : dead_id[j];
    if (e >= 0 && e < n_total) {
      const int st = live ? status[j] : dead_status[j];
      const double zz = live ? z[j] : dead_z[j];
      const double *r = rec + e * WS_N;
      const double m = r[WS_MASS_OIL];
      const bool stranded = st == stranded_code;
      v[0] = !stranded && zz == 0 ? m : 0.;
      v[1] = !stranded && zz != 0 ? m : 0.;
      v[2] = stranded ? m : 0.;
      v[3] = r[WS_MASS_EVAPORATED]; v[4] = r[WS_MASS_DISPERSED]; v[5] = r[WS_MASS_BIODEGRADED];
      v[7] = 1.;
    }
  }
  weather_block_fold(sh, v, WeatherSum8());
  if (threadIdx.x < 8) part[(size_t)blockIdx.x * 8 + threadIdx.x] = sh[0][threadIdx.x];
}

__global__ __launch_bounds__(BLOCK) void k_weather_pad_rows(long long n, int ncomp, int stride, const double *rows, double *mc) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n * stride) return;
  const long long e = i / stride;
  const int k = (int)(i - e * stride);
  mc[i] = k < ncomp ? rows[e * ncomp + k] : 0.;
}
__global__ __launch_bounds__(BLOCK) void k_weather_unpad_rows(long long n, int ncomp, int stride, const double *mc, double *rows) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n * ncomp) return;
  const long long e = i / ncomp;
  rows[i] = mc[e * stride + (i - e * ncomp)];
}
__global__ __launch_bounds__(BLOCK) void k_weather_column(long long n, int k, int to_table, double *rec, double *col) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (to_table) rec[i * WS_N + k] = col[i];
  else col[i] = rec[i * WS_N + k];
}

// ------------------------------------------------------------------ entry points
// The oil as a table and the side table for n_total elements (openoil.py:682-693 prepare_run: one row of mass_components per
// scheduled element, indexed by ID).  Replaces an earlier table of the particle set.
int odr_oil_weathering_setup(odr_ctx *c, odr_particles *p, const odr_oil_table *t, int64_t n_total) {
  REQUIRE(c && p && t, "NULL argument");
  REQUIRE(t->ncomp >= 1 && t->ncomp <= OIL_MAXCOMP, "an oil of %d pseudo-components: the table holds 1 .. %d (ODR_OIL_MAXCOMP)", t->ncomp,
          OIL_MAXCOMP);
  REQUIRE(t->mwf_n >= 0 && t->mwf_n <= 2, "max_water_fraction has %d entries, not 0, 1 or 2", t->mwf_n);
  REQUIRE(n_total > 0, "n_total must be positive");
  for (int k = 0; k < 4 * OIL_MAXCOMP; ++k) REQUIRE(t->comp[k] == t->comp[k], "NaN in the component constants");
  for (double v : {t->density, t->density_ref_temp, t->density_k, t->viscosity, t->viscosity_ref_temp, t->viscosity_B, t->bulltime,
                   t->bullwinkle, t->y_max, t->sea_water_density})
    REQUIRE(v == v, "NaN in the oil table");
  REQUIRE(t->mwf_n < 2 || t->mwf_t[1] != t->mwf_t[0], "the two temperatures of max_water_fraction are equal");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));      // a launch that reads an earlier table may be in flight
  odr_i_weather_release(p);
  odr_weather *w = new odr_weather();
  memset(w, 0, sizeof *w);
  WeatherOil &O = w->O;
  O.ncomp = t->ncomp; O.stride = (t->ncomp + 1) & ~1; O.mwf_n = t->mwf_n; O.pad = 0;
  O.rho_ref = t->density; O.rho_k = t->density_k; O.rho_T = t->density_ref_temp;
  O.nu_ref = t->viscosity; O.nu_B = t->viscosity_B; O.nu_T = t->viscosity_ref_temp;
  O.bulltime = t->bulltime; O.bullwinkle = t->bullwinkle; O.y_max = t->y_max; O.rho_w = t->sea_water_density;
  for (int k = 0; k < 2; ++k) { O.mwf_t[k] = t->mwf_t[k]; O.mwf_w[k] = t->mwf_w[k]; }
  w->n_total = n_total;
  p->weather = w;
  const size_t nparts = (size_t)nblk(p->cap + p->dead_cap) + 1;
  auto drop = [&](int code) { odr_i_weather_release(p); return code; };
  if (hipMalloc((void **)&w->K, sizeof(double) * 4 * OIL_MAXCOMP) != hipSuccess ||
      hipMalloc((void **)&w->rec, sizeof(double) * WS_N * (size_t)n_total) != hipSuccess ||
      hipMalloc((void **)&w->mc, sizeof(double) * (size_t)O.stride * (size_t)n_total) != hipSuccess ||
      hipMalloc((void **)&w->red, sizeof(double) * (WR_N + 8)) != hipSuccess || hipMalloc((void **)&w->part, sizeof(double) * 8 * nparts) != hipSuccess)
    return drop(fail(ODR_ERR_HIP, "allocating the weathering table for %lld elements of %d components failed", (long long)n_total, t->ncomp));
  if (int rc = odr_i_h2d(c, w->K, t->comp, sizeof(double) * 4 * OIL_MAXCOMP, c->stream)) return drop(rc);
  if (hipMemsetAsync(w->rec, 0, sizeof(double) * WS_N * (size_t)n_total, c->stream) != hipSuccess ||
      hipMemsetAsync(w->mc, 0, sizeof(double) * (size_t)O.stride * (size_t)n_total, c->stream) != hipSuccess ||
      hipMemsetAsync(w->red, 0, sizeof(double) * (WR_N + 8), c->stream) != hipSuccess)
    return drop(fail(ODR_ERR_HIP, "clearing the weathering table failed"));
  return 0;
}

static int weather_of(odr_particles *p, odr_weather **w) {
  if (!p->weather) return fail(ODR_ERR_STATE, "the particle set has no weathering table (odr_oil_weathering_setup)");
  *w = p->weather;
  return 0;
}

// The rows [id0, id0 + n) as seed_elements and prepare_run leave them (openoil.py:1726-1755, :686-693): records[n][14] in the order
// of odr_oil_weathering_get's names (the 14th value unused), rows[n][ncomp] = mass_fraction * mass_oil.
int odr_oil_weathering_seed(odr_ctx *c, odr_particles *p, int64_t id0, int64_t n, const double *records, const double *rows) {
  REQUIRE(c && p && records && rows, "NULL argument");
  odr_weather *w;
  if (int rc = weather_of(p, &w)) return rc;
  REQUIRE(id0 >= 0 && n >= 0 && id0 + n <= w->n_total, "rows %lld .. %lld of a table of %lld", (long long)id0, (long long)(id0 + n),
          (long long)w->n_total);
  if (n == 0) return 0;
  const int nc = w->O.ncomp, st = w->O.stride;
  H2D(w->rec + id0 * WS_N, records, sizeof(double) * WS_N * (size_t)n);
  void *s;
  if (int rc = scratch(c, p, sizeof(double) * (size_t)n * nc, &s)) return rc;
  H2D(s, rows, sizeof(double) * (size_t)n * nc);
  hipLaunchKernelGGL(k_weather_pad_rows, dim3(nblk(n * st)), dim3(BLOCK), 0, c->stream, (long long)n, nc, st, (const double *)s, w->mc + id0 * st);
  HIPCHK(hipGetLastError());
  return 0;
}

static int weather_column(const char *name) {
  for (int k = 0; k < WS_N; ++k)
    if (WS_NAMES[k] && !strcmp(name, WS_NAMES[k])) return k;
  return -1;
}

// One variable of the table by element ID: out[n_total] for a name of the record ("mass_oil", "mass_evaporated", "mass_dispersed",
// "mass_biodegraded", "fraction_evaporated", "water_fraction", "interfacial_area", "density", "viscosity", "bulltime",
// "biodegradation_half_time_droplet", "biodegradation_half_time_slick", "oil_film_thickness"), out[n_total][ncomp] for
// "mass_components", out[8] for "reduction" (the call-wide values the last odr_oil_weather formed).  Waits for the stream.
int odr_oil_weathering_get(odr_ctx *c, odr_particles *p, const char *name, double *out) {
  REQUIRE(c && p && name && out, "NULL argument");
  odr_weather *w;
  if (int rc = weather_of(p, &w)) return rc;
  const long long n = w->n_total;
  if (!strcmp(name, "reduction")) { D2H(out, w->red, sizeof(double) * WR_N); return 0; }
  void *s;
  if (!strcmp(name, "mass_components")) {
    const int nc = w->O.ncomp;
    if (int rc = scratch(c, p, sizeof(double) * (size_t)n * nc, &s)) return rc;
    hipLaunchKernelGGL(k_weather_unpad_rows, dim3(nblk(n * nc)), dim3(BLOCK), 0, c->stream, n, nc, w->O.stride, (const double *)w->mc, (double *)s);
    HIPCHK(hipGetLastError());
    D2H(out, s, sizeof(double) * (size_t)n * nc);
    return 0;
  }
  const int k = weather_column(name);
  REQUIRE(k >= 0, "no weathering variable '%s'", name);
  if (int rc = scratch(c, p, sizeof(double) * (size_t)n, &s)) return rc;
  hipLaunchKernelGGL(k_weather_column, dim3(nblk(n)), dim3(BLOCK), 0, c->stream, n, k, 0, w->rec, (double *)s);
  HIPCHK(hipGetLastError());
  D2H(out, s, sizeof(double) * (size_t)n);
  return 0;
}

// the reverse, for the names of the record and "mass_components"
int odr_oil_weathering_set(odr_ctx *c, odr_particles *p, const char *name, const double *in) {
  REQUIRE(c && p && name && in, "NULL argument");
  odr_weather *w;
  if (int rc = weather_of(p, &w)) return rc;
  const long long n = w->n_total;
  void *s;
  if (!strcmp(name, "mass_components")) {
    const int nc = w->O.ncomp, st = w->O.stride;
    if (int rc = scratch(c, p, sizeof(double) * (size_t)n * nc, &s)) return rc;
    H2D(s, in, sizeof(double) * (size_t)n * nc);
    hipLaunchKernelGGL(k_weather_pad_rows, dim3(nblk(n * st)), dim3(BLOCK), 0, c->stream, n, nc, st, (const double *)s, w->mc);
    HIPCHK(hipGetLastError());
    return 0;
  }
  const int k = weather_column(name);
  REQUIRE(k >= 0, "no weathering variable '%s'", name);
  if (int rc = scratch(c, p, sizeof(double) * (size_t)n, &s)) return rc;
  H2D(s, in, sizeof(double) * (size_t)n);
  hipLaunchKernelGGL(k_weather_column, dim3(nblk(n)), dim3(BLOCK), 0, c->stream, n, k, 1, w->rec, (double *)s);
  HIPCHK(hipGetLastError());
  return 0;
}

// oil_weathering_noaa over the active set (openoil.py:717-790): a reduction for the call-wide decisions, whose results stay on the
// device, then one launch for every element.  Enqueued on the context's stream; no host synchronisation.
int odr_oil_weather(odr_ctx *c, odr_particles *p, double dt_seconds, int flags) {
  REQUIRE(c && p, "NULL argument");
  odr_weather *w;
  if (int rc = weather_of(p, &w)) return rc;
  REQUIRE(dt_seconds == dt_seconds, "dt_seconds is NaN");
  const int all = WEATHER_PROPERTIES | WEATHER_EVAPORATION | WEATHER_EMULSIFICATION | WEATHER_DISPERSION | WEATHER_BIO_HALF_TIME | WEATHER_BIO_ADCROFT;
  REQUIRE(flags >= 0 && !(flags & ~all), "unknown process flags %d", flags);
  REQUIRE((flags & (WEATHER_BIO_HALF_TIME | WEATHER_BIO_ADCROFT)) != (WEATHER_BIO_HALF_TIME | WEATHER_BIO_ADCROFT), "two biodegradation methods");
  if (!p->env[VAR_XWIND] || !p->env[VAR_YWIND] || !p->env[VAR_TEMP])
    return fail(ODR_ERR_STATE, "x_wind, y_wind and sea_water_temperature must have been sampled");
  if (int rc = property_slots(p, {OIL_DENSITY, OIL_VISCOSITY})) return rc;
  if (p->id_max >= w->n_total) return fail(ODR_ERR_STATE, "element ID %lld has no row in a table of %lld", p->id_max, (long long)w->n_total);
  p->epoch++;  // properties change
  if (p->n == 0) return 0;
  const unsigned nb = nblk(p->n);
  hipLaunchKernelGGL(k_weather_reduce, dim3(nb), dim3(BLOCK), 0, c->stream, (long long)p->n, w->n_total, w->O, flags, p->i32[0], p->d64[2], p->f32[3],
                     p->env[VAR_XWIND], p->env[VAR_YWIND], p->env[VAR_TEMP], p->env[VAR_HS], p->env[VAR_TP], (const double *)w->rec, w->part);
  hipLaunchKernelGGL((k_weather_fold<WeatherFlagFold, true>), dim3(1), dim3(BLOCK), 0, c->stream, (int)nb, (const double *)w->part, w->red);
  hipLaunchKernelGGL(k_weather, dim3(nb), dim3(BLOCK), 0, c->stream, (long long)p->n, w->n_total, w->O, (const double *)w->K, (const double *)w->red,
                     flags, dt_seconds, p->i32[0], p->d64[2], p->f32[3], p->env[VAR_XWIND], p->env[VAR_YWIND], p->env[VAR_TEMP], p->env[VAR_HS],
                     p->env[VAR_TP], w->rec, w->mc, p->aux[OIL_DENSITY], p->aux[OIL_VISCOSITY]);
  HIPCHK(hipGetLastError());
  return 0;
}

// get_oil_budget's sums now (openoil.py:1241-1306): out[8] = mass_surface, mass_submerged, mass_stranded, mass_evaporated,
// mass_dispersed, mass_biodegraded, mass_total, elements counted.  Active and deactivated elements are counted, the latter with
// the masses, depth and status they left with (the reference forward-fills them).  One reduction with a fixed fold order.
int odr_oil_budget(odr_ctx *c, odr_particles *p, int32_t stranded_code, double *out) {
  REQUIRE(c && p && out, "NULL argument");
  odr_weather *w;
  if (int rc = weather_of(p, &w)) return rc;
  const long long m = p->n + p->ndead;
  if (m == 0) { memset(out, 0, sizeof(double) * 8); return 0; }
  const unsigned nb = nblk(m);
  hipLaunchKernelGGL(k_weather_budget, dim3(nb), dim3(BLOCK), 0, c->stream, (long long)p->n, (long long)p->ndead, w->n_total, (int)stranded_code,
                     p->i32[0], p->i32[1], p->d64[2], p->deadi32[0], p->deadi32[1], p->dead64[2], (const double *)w->rec, w->part);
  hipLaunchKernelGGL((k_weather_fold<WeatherSum8, false>), dim3(1), dim3(BLOCK), 0, c->stream, (int)nb, (const double *)w->part, w->red + WR_N);
  HIPCHK(hipGetLastError());
  D2H(out, w->red + WR_N, sizeof(double) * 8);
  out[6] = out[4] + out[1] + out[0] + out[2] + out[3] + out[5];      // the reference's order (:1302-1303)
  return 0;
}
