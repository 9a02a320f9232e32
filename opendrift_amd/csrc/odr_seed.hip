// libodrift_hip.so, a translation unit of its own: the seeding geometry of seed_cone, seed_repeated_segment and seed_within_polygon
// (models/basemodel/__init__.py:1240-1353, :1402-1456, :1487-1558).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_seed.hip.h"

namespace {

constexpr long long POINTS_CHUNK = 1ll << 20;      // points of one odr_points_in_polygon launch

bool all_finite(const double *a, long long n) {
  for (long long k = 0; k < n; ++k) if (!std::isfinite(a[k])) return false;
  return true;
}

}  // namespace

// pyproj.Geod(ellps='WGS84').npts(lon1, lat1, lon2, lat2, npts) as seed_cone calls it (models/basemodel/__init__.py:1286-1291):
// npts points on the geodesic from point 1 to point 2 at i * s12 / (npts + 1), i = 1 .. npts.  Synchronous.
int odr_geod_npts(odr_ctx *c, double lon1, double lat1, double lon2, double lat2, int64_t npts, double *out_lon, double *out_lat) {
  REQUIRE(c && out_lon && out_lat, "NULL argument");
  REQUIRE(npts >= 0, "negative size");
  REQUIRE(std::isfinite(lon1) && std::isfinite(lon2) && std::fabs(lat1) <= 90 && std::fabs(lat2) <= 90,
          "end points (%g, %g) and (%g, %g)", lon1, lat1, lon2, lat2);
  if (npts == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  double *d_line, *d_lon, *d_lat;
  if (int rc = B.alloc((void **)&d_line, sizeof(double) * 2)) return rc;
  if (int rc = B.alloc((void **)&d_lon, sizeof(double) * (size_t)npts)) return rc;
  if (int rc = B.alloc((void **)&d_lat, sizeof(double) * (size_t)npts)) return rc;
  hipLaunchKernelGGL(k_npts_line, dim3(1), dim3(64), 0, c->stream, lon1, lat1, lon2, lat2, d_line);
  HIPCHK(hipGetLastError());
  const unsigned blocks = (unsigned)((npts + SEED_BLOCK - 1) / SEED_BLOCK);
  hipLaunchKernelGGL(k_npts_points, dim3(blocks), dim3(SEED_BLOCK), 0, c->stream, lon1, lat1, (const double *)d_line, (long long)npts, d_lon, d_lat);
  HIPCHK(hipGetLastError());
  D2H(out_lon, d_lon, sizeof(double) * (size_t)npts);
  D2H(out_lat, d_lat, sizeof(double) * (size_t)npts);
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// matplotlib.path.Path(ring).contains_points(points): the crossing rule for n points and a ring of m vertices.  Synchronous.
int odr_points_in_polygon(odr_ctx *c, int64_t n, const double *x, const double *y, int32_t m, const double *vx, const double *vy,
                          uint8_t *inside) {
  REQUIRE(c && x && y && vx && vy && inside, "NULL argument");
  REQUIRE(n >= 0, "negative size");
  REQUIRE(m >= 3, "%d vertices: a polygon needs three", m);
  REQUIRE(all_finite(vx, m) && all_finite(vy, m), "a vertex is not finite");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  const long long chunk = std::min<long long>(n, POINTS_CHUNK);
  double *d_x, *d_y, *d_vx, *d_vy;
  unsigned char *d_in;
  if (int rc = B.alloc((void **)&d_x, sizeof(double) * (size_t)chunk)) return rc;
  if (int rc = B.alloc((void **)&d_y, sizeof(double) * (size_t)chunk)) return rc;
  if (int rc = B.alloc((void **)&d_vx, sizeof(double) * (size_t)m)) return rc;
  if (int rc = B.alloc((void **)&d_vy, sizeof(double) * (size_t)m)) return rc;
  if (int rc = B.alloc((void **)&d_in, (size_t)chunk)) return rc;
  H2D(d_vx, vx, sizeof(double) * (size_t)m);
  H2D(d_vy, vy, sizeof(double) * (size_t)m);
  for (long long o = 0; o < n; o += chunk) {
    const long long k = std::min(chunk, n - o);
    H2D(d_x, x + o, sizeof(double) * (size_t)k);
    H2D(d_y, y + o, sizeof(double) * (size_t)k);
    const unsigned blocks = (unsigned)((k + SEED_BLOCK - 1) / SEED_BLOCK);
    hipLaunchKernelGGL(k_pip_points, dim3(blocks), dim3(SEED_BLOCK), 0, c->stream, k, (const double *)d_x, (const double *)d_y, (int)m,
                       (const double *)d_vx, (const double *)d_vy, d_in);
    HIPCHK(hipGetLastError());
    D2H(inside + o, d_in, (size_t)k);
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// OpenDriftSimulation.points_within_polygon (models/basemodel/__init__.py:1487-1558): `number` positions within the polygon.
// The set-up runs on the host (seed_plan); k_seed_edges tests every grid point, k_seed_scan turns the workgroups' counts into
// offsets, k_seed_compact writes the inside points in grid order; the duplicates behind them are copies on the host.  Synchronous.
int odr_polygon_points(odr_ctx *c, int32_t m, const double *lons, const double *lats, int64_t number, double *out_lon, double *out_lat,
                       int64_t *n_inside, int32_t *nx, int32_t *ny) {
  REQUIRE(c && lons && lats && out_lon && out_lat && n_inside && nx && ny, "NULL argument");
  REQUIRE(m >= 3, "%d vertices: a polygon needs three", m);
  REQUIRE(number >= 1, "%lld elements", (long long)number);
  REQUIRE(all_finite(lons, m) && all_finite(lats, m), "a vertex is not finite");
  SeedPlan P;
  std::vector<double> rx, ry;
  const int status = seed_plan(m, lons, lats, number, P, rx, ry);
  REQUIRE(status != SEED_NO_CONE, "the standard parallels %g and %g give no Albers cone", *std::min_element(lats, lats + m),
          *std::max_element(lats, lats + m));
  REQUIRE(status != SEED_NO_AREA, "the polygon has no area");
  REQUIRE(status != SEED_TOO_MANY, "a grid of 2^31 points or more");
  KernelClock &clock = c->clock[CLOCK_POLYGON_POINTS];
  clock.reset();
  *nx = P.nx; *ny = P.ny; *n_inside = 0;
  const long long n = (long long)P.nx * P.ny;
  if (n == 0) {
    seed_centre(m, lons, lats, number, out_lon, out_lat);
    return 0;
  }

  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  const int mc = (int)rx.size();
  const long long nwg = (n + SEED_BLOCK - 1) / SEED_BLOCK;
  double *d_vx, *d_vy;
  unsigned long long *d_masks;
  unsigned *d_counts, *d_offsets;
  if (int rc = B.alloc((void **)&d_vx, sizeof(double) * (size_t)mc)) return rc;
  if (int rc = B.alloc((void **)&d_vy, sizeof(double) * (size_t)mc)) return rc;
  if (int rc = B.alloc((void **)&d_masks, sizeof(unsigned long long) * (size_t)nwg * SEED_WAVES)) return rc;
  if (int rc = B.alloc((void **)&d_counts, sizeof(unsigned) * (size_t)nwg)) return rc;
  if (int rc = B.alloc((void **)&d_offsets, sizeof(unsigned) * (size_t)(nwg + 1))) return rc;
  H2D(d_vx, rx.data(), sizeof(double) * (size_t)mc);
  H2D(d_vy, ry.data(), sizeof(double) * (size_t)mc);
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_seed_edges, dim3((unsigned)nwg), dim3(SEED_BLOCK), 0, c->stream, P, n, mc, (const double *)d_vx, (const double *)d_vy,
                     d_masks, d_counts);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(SEED_BLOCK), 0, c->stream, (const unsigned *)d_counts, nwg, d_offsets);
  HIPCHK(hipGetLastError());
  if (int rc = clock.stop(c->stream)) return rc;
  unsigned total = 0;
  D2H(&total, d_offsets + nwg, sizeof(unsigned));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n_inside = total;
  if (total == 0) {
    seed_border(m, lons, lats, number, out_lon, out_lat);
    return 0;
  }

  const long long keep = std::min<long long>(total, number);
  double *d_lon, *d_lat;
  if (int rc = B.alloc((void **)&d_lon, sizeof(double) * (size_t)keep)) return rc;
  if (int rc = B.alloc((void **)&d_lat, sizeof(double) * (size_t)keep)) return rc;
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_seed_compact, dim3((unsigned)nwg), dim3(SEED_BLOCK), 0, c->stream, P, n, (const unsigned long long *)d_masks,
                     (const unsigned *)d_offsets, keep, d_lon, d_lat);
  HIPCHK(hipGetLastError());
  if (int rc = clock.stop(c->stream)) return rc;
  D2H(out_lon, d_lon, sizeof(double) * (size_t)keep);
  D2H(out_lat, d_lat, sizeof(double) * (size_t)keep);
  HIPCHK(hipStreamSynchronize(c->stream));
  seed_cyclic(out_lon, keep, number);
  seed_cyclic(out_lat, keep, number);
  return 0;
}

// Device time of the launches of the last odr_polygon_points of this context [ms]
int odr_polygon_points_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_POLYGON_POINTS].read(ms);
}
