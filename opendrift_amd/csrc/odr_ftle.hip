// libodrift_hip.so, a translation unit of its own: FTLE maps of a grid of elements (OpenDriftSimulation.calculate_ftle,
// models/basemodel/__init__.py:4844-4923; physics_methods.ftle, models/physics_methods.py:458-484).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_ftle.hip.h"

namespace {

bool kind_ok(int kind) {
  switch (kind) {
    case ODR_PROJ_LATLONG: case ODR_PROJ_STERE_EQUIT_SPHERE: case ODR_PROJ_STERE_POLAR: case ODR_PROJ_MERC: case ODR_PROJ_LCC:
    case ODR_PROJ_TMERC: case ODR_PROJ_LAEA: case ODR_PROJ_STERE_OBLIQUE: case ODR_PROJ_OB_TRAN: return true;
    default: return false;
  }
}

}  // namespace

// physics_methods.ftle (models/physics_methods.py:458-484) of the displacements b_x1 - X, b_y1 - Y that calculate_ftle forms from the
// last positions of one run (models/basemodel/__init__.py:4898-4902, :4911-4915).  Synchronous.
int odr_ftle_map(odr_ctx *c, const odr_proj_desc *proj, int32_t nx, int32_t ny, const double *xs, const double *ys, double delta,
                 double duration_seconds, const float *lon, const float *lat, float *ftle, double *displacement) {
  REQUIRE(c && proj && xs && ys && lon && lat && ftle, "NULL argument");
  REQUIRE(proj->kind != ODR_PROJ_CURVILINEAR, "a reader without a projection has no coordinates to differentiate in");
  REQUIRE(kind_ok(proj->kind), "unknown projection kind %d", (int)proj->kind);
  REQUIRE(nx >= 2 && ny >= 2, "%d x %d cells: np.gradient needs two along each axis", (int)nx, (int)ny);
  REQUIRE((long long)nx * (long long)ny < (1ll << 31), "%d x %d cells, 2^31 or more", (int)nx, (int)ny);
  REQUIRE(std::isfinite(delta) && delta > 0, "delta = %g", delta);
  REQUIRE(std::isfinite(duration_seconds) && duration_seconds != 0, "duration_seconds = %g", duration_seconds);
  for (int k = 0; k < nx; ++k) REQUIRE(std::isfinite(xs[k]), "xs[%d] is not finite", k);
  for (int k = 0; k < ny; ++k) REQUIRE(std::isfinite(ys[k]), "ys[%d] is not finite", k);
  const size_t n = (size_t)nx * (size_t)ny;

  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  const float *in[2] = {lon, lat};
  for (const float *&q : in) {
    if (odr_i_on_device(q)) continue;
    float *up;
    if (int rc = B.alloc((void **)&up, sizeof(float) * n)) return rc;
    H2D(up, q, sizeof(float) * n);
    q = up;
  }
  double *axes, *disp;
  float *out;
  if (int rc = B.alloc((void **)&axes, sizeof(double) * ((size_t)nx + (size_t)ny))) return rc;
  H2D(axes, xs, sizeof(double) * (size_t)nx);
  H2D(axes + nx, ys, sizeof(double) * (size_t)ny);
  if (int rc = B.alloc((void **)&disp, sizeof(double) * 2 * n)) return rc;
  if (int rc = B.alloc((void **)&out, sizeof(float) * n)) return rc;
  DevProj P;
  odr_i_proj_init(P, proj);

  KernelClock &clock = c->clock[CLOCK_FTLE];
  clock.reset();
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_ftle_displacement, dim3(nblk((long long)n)), dim3(BLOCK), 0, c->stream, P, in[0], in[1], axes, axes + nx, (int)nx,
                     (long long)n, disp, disp + n);
  HIPCHK(hipGetLastError());
  const unsigned tiles_x = (unsigned)((nx + FTLE_TILE_X - 1) / FTLE_TILE_X), tiles_y = (unsigned)((ny + FTLE_TILE_Y - 1) / FTLE_TILE_Y);
  // (tiles_x * tiles_y < 2^31: n < 2^31 and nx, ny >= 2 leave at most 2^28 + 2^24 tiles)
  hipLaunchKernelGGL(k_ftle_cell, dim3(tiles_x * tiles_y), dim3(FTLE_TILE_X * FTLE_TILE_Y), 0, c->stream, disp, disp + n, (int)nx, (int)ny,
                     tiles_x, 2 * delta, fabs(duration_seconds), out);
  HIPCHK(hipGetLastError());
  if (int rc = clock.stop(c->stream)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));

  D2H(ftle, out, sizeof(float) * n);
  if (displacement) D2H(displacement, disp, sizeof(double) * 2 * n);
  return 0;
}

// Device time of the two launches of the last odr_ftle_map of this context that got as far as launching [ms]
int odr_ftle_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_FTLE].read(ms);
}
