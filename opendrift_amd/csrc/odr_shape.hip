// libodrift_hip.so, a translation unit of its own: the land mask of coastline polygons (readers/reader_shape.py) -- an exact
// point-in-polygon-set test behind a uniform grid.  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_shape.hip.h"

struct odr_shape {
  ShGrid dev;      // off / ent / tag: device arrays
  DevProj proj;
  std::vector<void *> bufs;
  long long entries, longest, nonempty;
  int nudges;
};

namespace {

constexpr long long CONTAINS_CHUNK = 1ll << 20;      // points of one odr_shape_contains launch

// odr_shape_last_kernel_ms: the launches of odr_shape_contains are timed as they run (the call is synchronous); the launch of
// odr_shape_sample is bracketed by two events that are read when the time is asked for
float g_kernel_ms = 0.f;
hipEvent_t g_ev[2] = {nullptr, nullptr};
bool g_pending = false;
int g_ev_device = -1;      // the device the two events belong to

int ensure_events(const odr_ctx *c) {
  if (g_ev_device != c->device) {
    for (hipEvent_t &e : g_ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    g_pending = false;
    g_ev_device = c->device;
  }
  for (hipEvent_t &e : g_ev) if (!e) HIPCHK(hipEventCreate(&e));
  return 0;
}

int upload(odr_ctx *c, odr_shape *s, const void *host, size_t bytes, const void **dev) {
  void *p = nullptr;
  HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 16)));      // (a shape without entries still has arrays to point at)
  s->bufs.push_back(p);
  if (bytes) H2D(p, host, bytes);
  *dev = p;
  return 0;
}

void release(odr_shape *s) {
  for (void *p : s->bufs) (void)hipFree(p);
  delete s;
}

}  // namespace

// The polygons on the device: the grid and its lists are built here, on the host, once.
int odr_shape_create(odr_ctx *c, const odr_proj_desc *proj, int64_t n_edges, const double *x1, const double *y1, const double *x2,
                     const double *y2, const int32_t *poly, int32_t n_poly, int32_t nx, int32_t ny, int invert, odr_shape **out) {
  REQUIRE(c && x1 && y1 && x2 && y2 && poly && out, "NULL argument");
  REQUIRE(n_edges >= 1 && n_edges < (1ll << 31), "%lld edges", (long long)n_edges);
  REQUIRE(!proj || (proj->kind >= ODR_PROJ_LATLONG && proj->kind <= ODR_PROJ_STERE_OBLIQUE && proj->kind != PROJ_CURVILINEAR),
          "projection kind %d does not serve a shape", proj ? proj->kind : 0);
  std::vector<ShEdge> e((size_t)n_edges);
  for (int64_t k = 0; k < n_edges; ++k) e[(size_t)k] = ShEdge{x1[k], y1[k], x2[k], y2[k]};
  ShIndex I;
  const std::string err = sh_build(n_edges, e.data(), poly, n_poly, nx, ny, invert, I);
  REQUIRE(err.empty(), "odr_shape_create: %s", err.c_str());
  HIPCHK(hipSetDevice(c->device));
  odr_shape *s = new odr_shape();
  s->dev = I.g;
  s->dev.off = nullptr; s->dev.ent = nullptr; s->dev.tag = nullptr;
  proj_init(s->proj, proj);
  s->dev.lon_mode = s->proj.kind == PROJ_LATLONG ? (I.g.xmin < 0 ? 1 : 2) : 0;      // modulate_longitude, variables.py:259-280
  s->entries = (long long)I.tag.size();
  s->longest = I.longest;
  s->nonempty = I.nonempty;
  s->nudges = I.nudges;
  int rc = upload(c, s, I.off.data(), sizeof(long long) * I.off.size(), (const void **)&s->dev.off);
  if (!rc) rc = upload(c, s, I.ent.data(), sizeof(ShEdge) * I.ent.size(), (const void **)&s->dev.ent);
  if (!rc) rc = upload(c, s, I.tag.data(), sizeof(int) * I.tag.size(), (const void **)&s->dev.tag);
  if (rc) {
    release(s);
    return rc;
  }
  *out = s;
  return 0;
}

int odr_shape_destroy(odr_ctx *c, odr_shape *s) {
  REQUIRE(c, "NULL argument");
  if (!s) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  release(s);
  return 0;
}

// stats[0 .. 7]: cells, entries, longest list, mean list of the cells that have one, times the origin was shifted, bytes of the index, nx, ny
int odr_shape_stats(odr_ctx *c, odr_shape *s, double *stats) {
  REQUIRE(c && s && stats, "NULL argument");
  const double cells = (double)s->dev.nx * (double)s->dev.ny;
  stats[0] = cells;
  stats[1] = (double)s->entries;
  stats[2] = (double)s->longest;
  stats[3] = s->nonempty ? (double)s->entries / (double)s->nonempty : 0.0;
  stats[4] = (double)s->nudges;
  stats[5] = 8.0 * (cells + 1.0) + (double)(sizeof(ShEdge) + sizeof(int)) * (double)s->entries;
  stats[6] = (double)s->dev.nx;
  stats[7] = (double)s->dev.ny;
  return 0;
}

// Reader.get_variables + the priority-list merge of land_binary_mask for every element of the set, ONE launch; the positions
// stay on the device.  first != 0: the reader heads the variable's list.
int odr_shape_sample(odr_ctx *c, odr_particles *p, odr_shape *s, int first) {
  REQUIRE(c && p && s, "NULL argument");
  const int v = VAR_LAND;
  p->epoch++;      // invalidates the cached reductions (reduce())
  if (!p->env[v]) {      // never sampled: nothing finite in the slot (every byte 0xff: a NaN)
    HIPCHK(hipMalloc((void **)&p->env[v], sizeof(float) * (size_t)p->cap));
    HIPCHK(hipMemsetAsync(p->env[v], 0xff, sizeof(float) * (size_t)p->cap, c->stream));
  }
  p->env_cok[v] = false;
  if (p->n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_events(c)) return rc;
  HIPCHK(hipEventRecord(g_ev[0], c->stream));
  hipLaunchKernelGGL(k_shape_sample, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, s->proj, s->dev, first != 0 ? 1 : 0, p->n,
                     (const double *)p->d64[0], (const double *)p->d64[1], p->env[v]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(g_ev[1], c->stream));
  g_pending = true;
  return 0;
}

// The bare query: land_binary_mask at n points in the reader's own coordinates.  x, y, out: host.  Synchronous.
int odr_shape_contains(odr_ctx *c, odr_shape *s, int64_t n, const double *x, const double *y, float *out) {
  REQUIRE(c && s, "NULL argument");
  REQUIRE(n >= 0 && (n == 0 || (x && y && out)), "bad arguments");
  g_kernel_ms = 0.f;
  g_pending = false;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_events(c)) return rc;
  const long long chunk = std::min<long long>(n, CONTAINS_CHUNK);
  double *d_xy = nullptr;
  float *d_out = nullptr;
  HIPCHK(hipMalloc((void **)&d_xy, sizeof(double) * 2 * (size_t)chunk));
  if (hipMalloc((void **)&d_out, sizeof(float) * (size_t)chunk) != hipSuccess) {
    (void)hipFree(d_xy);
    return fail(ODR_ERR_HIP, "hipMalloc of %lld values", chunk);
  }
  int rc = 0;
  for (long long o = 0; o < n && !rc; o += chunk) {
    const long long k = std::min(chunk, (long long)n - o);
    rc = odr_i_h2d(c, d_xy, x + o, sizeof(double) * (size_t)k, c->stream);
    if (!rc) rc = odr_i_h2d(c, d_xy + chunk, y + o, sizeof(double) * (size_t)k, c->stream);
    if (rc) break;
    (void)hipEventRecord(g_ev[0], c->stream);
    hipLaunchKernelGGL(k_shape_contains, dim3(nblk(k)), dim3(BLOCK), 0, c->stream, s->dev, k, (const double *)d_xy, (const double *)(d_xy + chunk), d_out);
    if (hipGetLastError() != hipSuccess) { rc = fail(ODR_ERR_HIP, "k_shape_contains did not launch"); break; }
    (void)hipEventRecord(g_ev[1], c->stream);
    rc = odr_i_d2h(c, out + o, d_out, sizeof(float) * (size_t)k, c->stream);
    float ms = 0.f;
    if (!rc && hipEventElapsedTime(&ms, g_ev[0], g_ev[1]) == hipSuccess) g_kernel_ms += ms;
  }
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d_xy);
  (void)hipFree(d_out);
  return rc;
}

// Device time [ms] of the launches of this process's last odr_shape_contains, or of the launch of its last odr_shape_sample
int odr_shape_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  if (g_pending) {
    HIPCHK(hipEventSynchronize(g_ev[1]));
    HIPCHK(hipEventElapsedTime(&g_kernel_ms, g_ev[0], g_ev[1]));
    g_pending = false;
  }
  *ms = g_kernel_ms;
  return 0;
}
