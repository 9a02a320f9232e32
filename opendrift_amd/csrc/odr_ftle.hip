// libodrift_hip.so, a translation unit of its own: FTLE maps of a grid of elements (OpenDriftSimulation.calculate_ftle,
// models/basemodel/__init__.py:4844-4923; physics_methods.ftle, models/physics_methods.py:458-484).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_ftle.hip.h"

namespace {

float g_kernel_ms = 0.f;      // odr_ftle_last_kernel_ms

struct FtleBuffers {      // released on every way out of odr_ftle_map
  float *lon = nullptr, *lat = nullptr, *out = nullptr;
  double *disp = nullptr, *axes = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~FtleBuffers() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (void *q : {(void *)lon, (void *)lat, (void *)out, (void *)disp, (void *)axes}) if (q) (void)hipFree(q);
  }
};

bool on_device(const void *ptr) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.type == hipMemoryTypeDevice;
  (void)hipGetLastError();      // plain pageable memory: not an error
  return false;
}

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
  FtleBuffers B;
  const float *dlon = lon, *dlat = lat;
  if (!on_device(lon)) {
    HIPCHK(hipMalloc((void **)&B.lon, sizeof(float) * n));
    H2D(B.lon, lon, sizeof(float) * n);
    dlon = B.lon;
  }
  if (!on_device(lat)) {
    HIPCHK(hipMalloc((void **)&B.lat, sizeof(float) * n));
    H2D(B.lat, lat, sizeof(float) * n);
    dlat = B.lat;
  }
  HIPCHK(hipMalloc((void **)&B.axes, sizeof(double) * ((size_t)nx + (size_t)ny)));
  H2D(B.axes, xs, sizeof(double) * (size_t)nx);
  H2D(B.axes + nx, ys, sizeof(double) * (size_t)ny);
  HIPCHK(hipMalloc((void **)&B.disp, sizeof(double) * 2 * n));
  HIPCHK(hipMalloc((void **)&B.out, sizeof(float) * n));
  DevProj P;
  odr_i_proj_init(P, proj);

  for (hipEvent_t &e : B.ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(B.ev[0], c->stream));
  hipLaunchKernelGGL(k_ftle_displacement, dim3(nblk((long long)n)), dim3(BLOCK), 0, c->stream, P, dlon, dlat, B.axes, B.axes + nx,
                     (int)nx, (long long)n, B.disp, B.disp + n);
  HIPCHK(hipGetLastError());
  const unsigned tiles_x = (unsigned)((nx + FTLE_TILE_X - 1) / FTLE_TILE_X), tiles_y = (unsigned)((ny + FTLE_TILE_Y - 1) / FTLE_TILE_Y);
  // (tiles_x * tiles_y < 2^31: n < 2^31 and nx, ny >= 2 leave at most 2^28 + 2^24 tiles)
  hipLaunchKernelGGL(k_ftle_cell, dim3(tiles_x * tiles_y), dim3(FTLE_TILE_X * FTLE_TILE_Y), 0, c->stream, B.disp, B.disp + n, (int)nx,
                     (int)ny, tiles_x, 2 * delta, fabs(duration_seconds), B.out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(B.ev[1], c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipEventElapsedTime(&g_kernel_ms, B.ev[0], B.ev[1]));

  D2H(ftle, B.out, sizeof(float) * n);
  if (displacement) D2H(displacement, B.disp, sizeof(double) * 2 * n);
  return 0;
}

// Device time of the two launches of the last odr_ftle_map of this process that got as far as launching [ms]
int odr_ftle_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  *ms = g_kernel_ms;
  return 0;
}
