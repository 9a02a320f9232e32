// libodrift_hip.so, a translation unit of its own: density maps on a grid regular in a projection and the radionuclide
// concentration maps of a finished run (OpenDriftSimulation.get_density_array_proj, models/basemodel/__init__.py:4148-4245;
// RadionuclideDrift.get_radionuclide_density_array and horizontal_smooth, models/radionuclides.py:1425-1492, :1518-1551).
#include "odr_host.h"
#include "odr_conc.hip.h"

namespace {

constexpr size_t CONC_SLAB_BYTES = 256u << 20;         // device memory of one slab of host inputs (ODR_CONC_SLAB_BYTES overrides)
constexpr long long CONC_LAUNCH_ENTRIES = 1ll << 30;   // entries of one launch
constexpr size_t CONC_HIST_BYTES = 8ull << 30;         // device memory of the whole histogram: refused beyond
constexpr int CONC_EXTENT_BLOCKS = 1024;               // partial records of one k_conc_extent launch
constexpr long long CONC_GRID_CHUNK = 1ll << 20;       // grid points of one k_conc_grid launch
constexpr size_t CONC_BOX_CELLS = 1u << 24;            // cells of one odr_box_smooth pass, unless one plane is larger

int increasing(const double *e, int n, const char *what) {
  REQUIRE(n >= 2, "%s: %d values, fewer than two", what, n);
  for (int k = 0; k < n; ++k) REQUIRE(std::isfinite(e[k]), "%s[%d] is not finite", what, k);
  for (int k = 1; k < n; ++k) REQUIRE(e[k] > e[k - 1], "%s is not strictly increasing at %d", what, k);
  return 0;
}

// the projections a map grid can be regular in: what odr_umesh / odr_shape take, and Mollweide
int proj_ok(const odr_proj_desc *proj) {
  if (!proj) return 0;
  switch (proj->kind) {
    case ODR_PROJ_LATLONG: return 0;
    case ODR_PROJ_STERE_EQUIT_SPHERE: case ODR_PROJ_STERE_POLAR: case ODR_PROJ_MERC: case ODR_PROJ_LCC: case ODR_PROJ_TMERC:
    case ODR_PROJ_LAEA: case ODR_PROJ_STERE_OBLIQUE: case ODR_PROJ_MOLL:
      REQUIRE(std::isfinite(proj->a) && proj->a > 0, "projection: a = %g", proj->a);
      return 0;
    default: return fail(ODR_ERR_INVALID, "projection kind %d does not serve a map grid", (int)proj->kind);
  }
}

// [trajectory][time] float32 inputs, each in host or device memory (NULL: absent), handed to `launch` slab by slab of whole
// trajectories: launch(ptr, entries) with device pointers.  The host arrays share a device buffer within the byte budget.
// clock: starts a measurement that brackets every slab's launches (NULL: they are not timed).
template <int NIN, class F>
int for_slabs(odr_ctx *c, DevScope &B, KernelClock *clock, const float *const (&in)[NIN], long long n_trajectories, long long n_times,
              F &&launch) {
  bool dev[NIN];
  int n_host = 0;
  for (int k = 0; k < NIN; ++k) {
    dev[k] = in[k] ? odr_i_on_device(in[k]) : true;
    if (!dev[k]) ++n_host;
  }
  long long slab_traj = std::max<long long>(1, CONC_LAUNCH_ENTRIES / n_times);
  if (n_host) {
    size_t budget = CONC_SLAB_BYTES;
    if (const char *s = getenv("ODR_CONC_SLAB_BYTES")) {
      const long long v = atoll(s);
      REQUIRE(v > 0, "ODR_CONC_SLAB_BYTES=%s", s);
      budget = (size_t)v;
    }
    const size_t row = sizeof(float) * (size_t)n_times * (size_t)n_host;
    slab_traj = std::min<long long>(slab_traj, std::max<long long>(1, (long long)(budget / row)));
  }
  slab_traj = std::min<long long>(slab_traj, n_trajectories);
  const size_t slab_floats = (size_t)slab_traj * (size_t)n_times;
  float *slab = nullptr;
  if (n_host) if (int rc = B.alloc((void **)&slab, sizeof(float) * slab_floats * (size_t)n_host)) return rc;
  if (clock) clock->reset();
  for (long long t0 = 0; t0 < n_trajectories; t0 += slab_traj) {
    const long long nt = std::min(slab_traj, n_trajectories - t0);
    const size_t off = (size_t)t0 * (size_t)n_times, count = (size_t)nt * (size_t)n_times;
    const float *ptr[NIN];
    int h = 0;
    for (int k = 0; k < NIN; ++k) {
      if (!in[k]) { ptr[k] = nullptr; continue; }
      if (dev[k]) { ptr[k] = in[k] + off; continue; }
      float *d = slab + slab_floats * (size_t)h++;
      H2D(d, in[k] + off, sizeof(float) * count);      // waits for the stream: the launch of the slab before has read `d`
      ptr[k] = d;
    }
    if (clock) if (int rc = clock->start(c->stream)) return rc;
    if (int rc = launch(ptr, (long long)count)) return rc;
    HIPCHK(hipGetLastError());
    if (clock) if (int rc = clock->stop(c->stream)) return rc;
  }
  return 0;
}

template <int MODE, typename T>
void launch_bin(odr_ctx *c, const ConcArgs &A, const DevProj &P, bool lds, T *H) {
  const size_t shm = sizeof(double) * ((lds ? (size_t)(A.ax.n + A.ay.n) : 0) + (MODE == CONC_SPECIES ? (size_t)A.n_bounds : 0));
  if (lds) hipLaunchKernelGGL((k_conc_bin<MODE, true, T>), dim3(nblk(A.n)), dim3(BLOCK), shm, c->stream, A, P, H);
  else hipLaunchKernelGGL((k_conc_bin<MODE, false, T>), dim3(nblk(A.n)), dim3(BLOCK), shm, c->stream, A, P, H);
}

// device histogram of `cells` cells -> float64 host arrays out[0 .. n_out) of cells / n_out each, through the bounce buffer
int fetch_hist(odr_ctx *c, const void *hist, size_t cells_each, int n_out, double *const *out, bool f64) {
  void *b;
  if (int rc = odr_i_bounce(c, 0, &b)) return rc;
  const size_t cell_bytes = f64 ? sizeof(double) : sizeof(unsigned), chunk = ODR_BOUNCE_BYTES / cell_bytes;
  for (int k = 0; k < n_out; ++k) {
    for (size_t o = 0; o < cells_each; o += chunk) {
      const size_t m = std::min(chunk, cells_each - o);
      HIPCHK(hipMemcpyAsync(b, (const char *)hist + ((size_t)k * cells_each + o) * cell_bytes, m * cell_bytes, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      if (f64) memcpy(out[k] + o, b, m * sizeof(double));
      else for (size_t i = 0; i < m; ++i) out[k][o + i] = (double)((const unsigned *)b)[i];
    }
  }
  return 0;
}

// edges (and z bounds) on the device, the axes of the bin search
int upload_axes(odr_ctx *c, DevScope &B, ConcArgs &A, int nx, const double *xe, int ny, const double *ye, int nz, const double *zb) {
  double *edges;
  if (int rc = B.alloc((void **)&edges, sizeof(double) * (size_t)(nx + ny + nz))) return rc;
  H2D(edges, xe, sizeof(double) * (size_t)nx);
  H2D(edges + nx, ye, sizeof(double) * (size_t)ny);
  if (nz) H2D(edges + nx + ny, zb, sizeof(double) * (size_t)nz);
  A.x_edges = edges; A.y_edges = edges + nx; A.z_bounds = nz ? edges + nx + ny : nullptr;
  A.ax = density_axis(xe, nx); A.ay = density_axis(ye, ny);
  return 0;
}

}  // namespace

// get_density_array_proj (models/basemodel/__init__.py:4148-4245) for given edges in projection units: H, H_submerged, H_stranded of
// every output time, the entries a map does not want counted in outside_bin when there is one.  Synchronous.
int odr_density_map_proj(odr_ctx *c, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, const float *z,
                         const float *status, const float *weight, int32_t stranded_code, const odr_proj_desc *proj, int32_t n_x_edges,
                         const double *x_edges, int32_t n_y_edges, const double *y_edges, int64_t outside_bin, double *H,
                         double *H_submerged, double *H_stranded) {
  REQUIRE(c && lon && lat && z && status && x_edges && y_edges && H && H_submerged, "NULL argument");
  REQUIRE(H_stranded || stranded_code < 0, "NULL H_stranded with a stranded category");
  REQUIRE(n_trajectories >= 0 && n_times >= 0, "negative size");
  REQUIRE((unsigned long long)n_trajectories < (1ull << 32), "%lld trajectories: the counts are 32-bit", (long long)n_trajectories);
  if (int rc = proj_ok(proj)) return rc;
  if (int rc = increasing(x_edges, n_x_edges, "x_edges")) return rc;
  if (int rc = increasing(y_edges, n_y_edges, "y_edges")) return rc;
  const unsigned long long plane = (unsigned long long)(n_x_edges - 1) * (unsigned long long)(n_y_edges - 1);
  REQUIRE(plane <= (1ull << 28), "%llu bins per output time, more than 2^28", plane);
  REQUIRE(outside_bin >= -1 && outside_bin < (long long)plane, "outside_bin %lld of %llu bins", (long long)outside_bin, plane);
  const bool weighted = weight != nullptr;
  const size_t cell_bytes = weighted ? sizeof(double) : sizeof(unsigned);
  const size_t cells = (size_t)n_times * plane;
  REQUIRE(3 * cells <= CONC_HIST_BYTES / cell_bytes, "%d output times of %llu bins: the three maps take more than %llu bytes on the device",
          (int)n_times, plane, (unsigned long long)CONC_HIST_BYTES);
  if (n_times == 0) return 0;
  const int nh = stranded_code >= 0 ? 3 : 2;
  double *out[3] = {H, H_submerged, H_stranded};
  if (n_trajectories == 0) {
    for (int k = 0; k < 3; ++k) if (out[k]) std::fill(out[k], out[k] + cells, 0.0);
    return 0;
  }

  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  void *hist;
  if (int rc = B.alloc(&hist, 3 * cells * cell_bytes)) return rc;      // (H_stranded's is written by nothing when there is no such category)
  HIPCHK(hipMemsetAsync(hist, 0, 3 * cells * cell_bytes, c->stream));
  ConcArgs A;
  memset(&A, 0, sizeof A);
  if (int rc = upload_axes(c, B, A, n_x_edges, x_edges, n_y_edges, y_edges, 0, nullptr)) return rc;
  A.cells = cells; A.n_times = n_times; A.stranded_code = stranded_code; A.outside_bin = (int)outside_bin;
  DevProj P;
  odr_i_proj_init(P, proj);
  const bool lds = n_x_edges + n_y_edges <= DENSITY_LDS_EDGES;
  const float *const in[5] = {lon, lat, z, status, weight};
  int rc = for_slabs(c, B, &c->clock[CLOCK_CONC], in, n_trajectories, n_times, [&](const float *const *ptr, long long count) {
    A.lon = ptr[0]; A.lat = ptr[1]; A.z = ptr[2]; A.aux = ptr[3]; A.weight = ptr[4];
    A.n = count;
    if (weighted) launch_bin<CONC_MASKS_W, double>(c, A, P, lds, (double *)hist);
    else launch_bin<CONC_MASKS, unsigned>(c, A, P, lds, (unsigned *)hist);
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = fetch_hist(c, hist, cells, nh, out, weighted))) return rc;
  if (nh == 2 && H_stranded) std::fill(H_stranded, H_stranded + cells, 0.0);
  return 0;
}

// get_radionuclide_density_array (models/radionuclides.py:1425-1492) for given edges and layer bounds: the counts of every output
// time, species and depth layer.  Synchronous.
int odr_species_layer_map(odr_ctx *c, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, const float *z,
                          const float *specie, const odr_proj_desc *proj, int32_t n_x_edges, const double *x_edges, int32_t n_y_edges,
                          const double *y_edges, int32_t n_z, const double *z_array, int32_t n_species, double *H) {
  REQUIRE(c && lon && lat && z && specie && x_edges && y_edges && z_array && H, "NULL argument");
  REQUIRE(n_trajectories >= 0 && n_times >= 0, "negative size");
  REQUIRE((unsigned long long)n_trajectories < (1ull << 32), "%lld trajectories: the counts are 32-bit", (long long)n_trajectories);
  REQUIRE(n_species >= 1 && n_species < (1 << 20), "%d species", (int)n_species);
  if (int rc = proj_ok(proj)) return rc;
  if (int rc = increasing(x_edges, n_x_edges, "x_edges")) return rc;
  if (int rc = increasing(y_edges, n_y_edges, "y_edges")) return rc;
  if (int rc = increasing(z_array, n_z, "z_array")) return rc;
  REQUIRE(n_z <= CONC_MAX_BOUNDS, "z_array: %d values, more than %d", (int)n_z, CONC_MAX_BOUNDS);
  const unsigned long long plane = (unsigned long long)(n_x_edges - 1) * (unsigned long long)(n_y_edges - 1);
  REQUIRE(plane <= (1ull << 28), "%llu bins per layer, more than 2^28", plane);
  const unsigned long long per_time = plane * (unsigned long long)n_species * (unsigned long long)(n_z - 1);
  REQUIRE(per_time <= (1ull << 28), "%llu bins per output time (species and layers included), more than 2^28", per_time);
  const size_t cells = (size_t)n_times * per_time;
  REQUIRE(cells <= CONC_HIST_BYTES / sizeof(unsigned), "%d output times of %llu bins take more than %llu bytes on the device", (int)n_times,
          per_time, (unsigned long long)CONC_HIST_BYTES);
  if (n_times == 0) return 0;
  if (n_trajectories == 0) { std::fill(H, H + cells, 0.0); return 0; }

  HIPCHK(hipSetDevice(c->device));
  DevScope B;
  unsigned *hist;
  if (int rc = B.alloc((void **)&hist, cells * sizeof(unsigned))) return rc;
  HIPCHK(hipMemsetAsync(hist, 0, cells * sizeof(unsigned), c->stream));
  ConcArgs A;
  memset(&A, 0, sizeof A);
  if (int rc = upload_axes(c, B, A, n_x_edges, x_edges, n_y_edges, y_edges, n_z, z_array)) return rc;
  A.cells = cells; A.n_times = n_times; A.stranded_code = -1; A.outside_bin = -1; A.n_species = n_species; A.n_bounds = n_z;
  DevProj P;
  odr_i_proj_init(P, proj);
  const bool lds = n_x_edges + n_y_edges <= DENSITY_LDS_EDGES;
  const float *const in[4] = {lon, lat, z, specie};
  int rc = for_slabs(c, B, &c->clock[CLOCK_CONC], in, n_trajectories, n_times, [&](const float *const *ptr, long long count) {
    A.lon = ptr[0]; A.lat = ptr[1]; A.z = ptr[2]; A.aux = ptr[3];
    A.n = count;
    launch_bin<CONC_SPECIES, unsigned>(c, A, P, lds, hist);
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return fetch_hist(c, hist, cells, 1, &H, false);
}

// Device time of the k_conc_bin launches of this context's last odr_density_map_proj or odr_species_layer_map [ms], summed over slabs
int odr_conc_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_CONC].read(ms);
}

// x.min(), x.max(), y.min(), y.max() of (x, y) = proj(lon, lat) over the finite projected positions.  Synchronous.
int odr_proj_extent(odr_ctx *c, const odr_proj_desc *proj, int64_t n, const float *lon, const float *lat, double *extent4) {
  REQUIRE(c && lon && lat && extent4, "NULL argument");
  REQUIRE(n >= 0, "negative size");
  if (int rc = proj_ok(proj)) return rc;
  double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
  if (n > 0) {
    HIPCHK(hipSetDevice(c->device));
    DevScope B;
    double *d_part;
    if (int rc = B.alloc((void **)&d_part, sizeof(double) * 4 * CONC_EXTENT_BLOCKS)) return rc;
    DevProj P;
    odr_i_proj_init(P, proj);
    std::vector<double> part(4 * CONC_EXTENT_BLOCKS);
    const float *const in[2] = {lon, lat};
    int rc = for_slabs(c, B, nullptr, in, n, 1, [&](const float *const *ptr, long long count) {
      const unsigned blocks = std::min<unsigned>(nblk(count), CONC_EXTENT_BLOCKS);
      hipLaunchKernelGGL(k_conc_extent, dim3(blocks), dim3(BLOCK), sizeof(double) * 4 * (BLOCK / 64), c->stream, P, ptr[0], ptr[1], count,
                         d_part);
      HIPCHK(hipGetLastError());
      D2H(part.data(), d_part, sizeof(double) * 4 * blocks);
      for (unsigned k = 0; k < blocks; ++k) {
        v[0] = std::fmin(v[0], part[4 * k]); v[1] = std::fmax(v[1], part[4 * k + 1]);
        v[2] = std::fmin(v[2], part[4 * k + 2]); v[3] = std::fmax(v[3], part[4 * k + 3]);
      }
      return 0;
    });
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  for (int k = 0; k < 4; ++k) extent4[k] = v[k];
  return 0;
}

// proj(X, Y, inverse=True) of Y, X = np.meshgrid(ys, xs): lon, lat [nx][ny].  Synchronous.
int odr_proj_grid_lonlat(odr_ctx *c, const odr_proj_desc *proj, int32_t nx, const double *xs, int32_t ny, const double *ys, double *lon,
                         double *lat) {
  REQUIRE(c && xs && ys && lon && lat, "NULL argument");
  REQUIRE(nx >= 1 && ny >= 1, "%d x %d grid points", (int)nx, (int)ny);
  if (int rc = proj_ok(proj)) return rc;
  for (int k = 0; k < nx; ++k) REQUIRE(std::isfinite(xs[k]), "xs[%d] is not finite", k);
  for (int k = 0; k < ny; ++k) REQUIRE(std::isfinite(ys[k]), "ys[%d] is not finite", k);
  const long long total = (long long)nx * (long long)ny, chunk = std::min(total, CONC_GRID_CHUNK);
  HIPCHK(hipSetDevice(c->device));
  DevScope B;
  double *axes, *dlon;
  if (int rc = B.alloc((void **)&axes, sizeof(double) * (size_t)(nx + ny))) return rc;
  if (int rc = B.alloc((void **)&dlon, sizeof(double) * 2 * (size_t)chunk)) return rc;
  H2D(axes, xs, sizeof(double) * (size_t)nx);
  H2D(axes + nx, ys, sizeof(double) * (size_t)ny);
  DevProj P;
  odr_i_proj_init(P, proj);
  double *dlat = dlon + chunk;
  for (long long k0 = 0; k0 < total; k0 += chunk) {
    const long long m = std::min(chunk, total - k0);
    hipLaunchKernelGGL(k_conc_grid, dim3(nblk(m)), dim3(BLOCK), 0, c->stream, P, (const double *)axes, (const double *)(axes + nx),
                       (int)ny, k0, m, dlon, dlat);
    HIPCHK(hipGetLastError());
    D2H(lon + k0, dlon, sizeof(double) * (size_t)m);
    D2H(lat + k0, dlat, sizeof(double) * (size_t)m);
  }
  return 0;
}

// horizontal_smooth (models/radionuclides.py:1518-1551) of n_planes planes [n0][n1].  Synchronous.
int odr_box_smooth(odr_ctx *c, int64_t n_planes, int32_t n0, int32_t n1, int32_t n, const double *a, double *out) {
  REQUIRE(c && a && out, "NULL argument");
  REQUIRE(n_planes >= 0 && n0 >= 1 && n1 >= 1, "%lld planes of %d x %d", (long long)n_planes, (int)n0, (int)n1);
  REQUIRE(n >= 0 && n < (1 << 26), "n = %d", (int)n);
  const size_t plane = (size_t)n0 * (size_t)n1;
  REQUIRE(plane <= (1ull << 28), "%llu cells per plane, more than 2^28", (unsigned long long)plane);
  for (int64_t p = 0; p < n_planes; ++p) {      // every window sum must be exact in float64, as the reference's is
    double total = 0;
    for (size_t k = 0; k < plane; ++k) {
      const double v = a[(size_t)p * plane + k];
      REQUIRE(std::isfinite(v), "plane %lld holds a value that is not finite", (long long)p);
      total += std::fabs(std::trunc(v));
    }
    REQUIRE(total < 9007199254740992.0, "plane %lld: the integer parts sum to 2^53 or more", (long long)p);
  }
  if (n == 0) {
    if (out != a) memcpy(out, a, sizeof(double) * plane * (size_t)n_planes);
    return 0;
  }
  if (n_planes == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  const long long per = std::max<long long>(1, std::min<long long>(n_planes, (long long)(CONC_BOX_CELLS / plane)));
  DevScope B;
  double *d_val;
  long long *d_sum;
  if (int rc = B.alloc((void **)&d_val, sizeof(double) * plane * (size_t)per)) return rc;
  if (int rc = B.alloc((void **)&d_sum, sizeof(long long) * plane * (size_t)per)) return rc;
  const double w = 2.0 * n + 1.0;
  for (long long p0 = 0; p0 < n_planes; p0 += per) {
    const long long m = std::min(per, n_planes - p0), cells = m * (long long)plane;
    H2D(d_val, a + (size_t)p0 * plane, sizeof(double) * (size_t)cells);
    hipLaunchKernelGGL((k_conc_box<true, double, long long>), dim3(nblk(cells)), dim3(BLOCK), 0, c->stream, (const double *)d_val, d_sum,
                       cells, (long long)n0, (long long)n1, (long long)n, 1.0);
    hipLaunchKernelGGL((k_conc_box<false, long long, double>), dim3(nblk(cells)), dim3(BLOCK), 0, c->stream, (const long long *)d_sum, d_val,
                       cells, (long long)n0, (long long)n1, (long long)n, w * w);
    HIPCHK(hipGetLastError());
    D2H(out + (size_t)p0 * plane, d_val, sizeof(double) * (size_t)cells);
  }
  return 0;
}
