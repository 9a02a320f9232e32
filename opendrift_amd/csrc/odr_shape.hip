// libodrift_hip.so, a translation unit of its own: the land mask of coastline polygons (readers/reader_shape.py) -- an exact
// point-in-polygon-set test behind a uniform grid.  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_shape.hip.h"

struct odr_shape {
  ShGrid dev;      // off / ent / tag: device arrays
  DevProj proj;
  DevScope bufs;
  long long entries, longest, nonempty;
  int nudges;
};

namespace {

constexpr long long CONTAINS_CHUNK = 1ll << 20;      // points of one odr_shape_contains launch

int upload(odr_ctx *c, odr_shape *s, const void *host, size_t bytes, const void **dev) {
  void *p;
  if (int rc = s->bufs.alloc(&p, std::max<size_t>(bytes, 16))) return rc;      // (a shape without entries still has arrays to point at)
  if (bytes) H2D(p, host, bytes);
  *dev = p;
  return 0;
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
    delete s;
    return rc;
  }
  *out = s;
  return 0;
}

int odr_shape_destroy(odr_ctx *c, odr_shape *s) {
  REQUIRE(c, "NULL argument");
  if (!s) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  delete s;
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
  KernelClock &clock = c->clock[CLOCK_SHAPE];
  clock.reset();
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_shape_sample, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, s->proj, s->dev, first != 0 ? 1 : 0, p->n,
                     (const double *)p->d64[0], (const double *)p->d64[1], p->env[v]);
  HIPCHK(hipGetLastError());
  return clock.stop(c->stream);
}

// The bare query: land_binary_mask at n points in the reader's own coordinates.  x, y, out: host.  Synchronous.
int odr_shape_contains(odr_ctx *c, odr_shape *s, int64_t n, const double *x, const double *y, float *out) {
  REQUIRE(c && s, "NULL argument");
  REQUIRE(n >= 0 && (n == 0 || (x && y && out)), "bad arguments");
  KernelClock &clock = c->clock[CLOCK_SHAPE];
  clock.reset();
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  const long long chunk = std::min<long long>(n, CONTAINS_CHUNK);
  DevScope B;      // released on every way out
  double *d_xy;
  float *d_out;
  if (int rc = B.alloc((void **)&d_xy, sizeof(double) * 2 * (size_t)chunk)) return rc;
  if (int rc = B.alloc((void **)&d_out, sizeof(float) * (size_t)chunk)) return rc;
  for (long long o = 0; o < n; o += chunk) {
    const long long k = std::min(chunk, (long long)n - o);
    H2D(d_xy, x + o, sizeof(double) * (size_t)k);
    H2D(d_xy + chunk, y + o, sizeof(double) * (size_t)k);
    if (int rc = clock.start(c->stream)) return rc;
    hipLaunchKernelGGL(k_shape_contains, dim3(nblk(k)), dim3(BLOCK), 0, c->stream, s->dev, k, (const double *)d_xy, (const double *)(d_xy + chunk), d_out);
    HIPCHK(hipGetLastError());
    if (int rc = clock.stop(c->stream)) return rc;
    D2H(out + o, d_out, sizeof(float) * (size_t)k);      // waits for the stream: the next chunk may overwrite d_xy
  }
  return 0;
}

// Device time [ms] of the launches of this context's last odr_shape_contains, or of the launch of its last odr_shape_sample
int odr_shape_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_SHAPE].read(ms);
}
