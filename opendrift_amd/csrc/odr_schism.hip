// libodrift_hip.so, a translation unit of its own: the SCHISM-style mesh reader -- the inverse-distance mean over the three nearest
// points of a time level's cloud, two time levels blended (readers/reader_schism_native.py).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_schism.hip.h"

struct odr_schism {
  ScMesh dev;
  DevProj proj;
  int n_nodes, n_levels;
  DevScope bufs;      // the search index and the hull's grid
  struct Level {
    double t;
    float *zcor;             // [node][n_levels], or NULL
    long long *off;          // [node + 1]: finite levels in front of the node (sc_ref_index)
    float *data[NVAR];
    int levels[NVAR];        // 0: [node]; n_levels: [node][n_levels]
  } level[SCHISM_MAXLEVELS];
};

namespace {

constexpr long long NEAREST_CHUNK = 1ll << 20;      // points of one odr_schism_nearest3 launch

bool all_finite(const double *a, long long n) {
  for (long long k = 0; k < n; ++k) if (!std::isfinite(a[k])) return false;
  return true;
}

int upload(odr_ctx *c, odr_schism *m, const void *host, size_t bytes, const void **dev) {
  void *p;
  if (int rc = m->bufs.alloc(&p, std::max<size_t>(bytes, 16))) return rc;
  if (bytes) H2D(p, host, bytes);
  *dev = p;
  return 0;
}

void release(odr_schism *m) {
  for (auto &L : m->level) {      // (replaced in place by the level uploads: not in bufs)
    if (L.zcor) (void)hipFree(L.zcor);
    if (L.off) (void)hipFree(L.off);
    for (float *p : L.data) if (p) (void)hipFree(p);
  }
  delete m;
}

// a device array of `bytes` in *slot: kept when it has that size already (the launches in flight read the old one otherwise)
int resident(odr_ctx *c, void **slot, bool same_size, size_t bytes) {
  if (*slot && same_size) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (*slot) HIPCHK(hipFree(*slot));
  *slot = nullptr;
  HIPCHK(hipMalloc(slot, bytes));
  return 0;
}

int partner_of(int var) {      // the y component of a vector pair's x component (vector_pairs_xy, variables.py)
  return var == VAR_U ? VAR_V : var == VAR_XWIND ? VAR_YWIND : var == VAR_SX ? VAR_SY : var == VAR_ICE_U ? VAR_ICE_V : -1;
}

}  // namespace

// The mesh on the device: the search index over the nodes and the grid over the hull's ring, both built here, on the host, once.
int odr_schism_create(odr_ctx *c, const odr_proj_desc *proj, int32_t n_nodes, const double *x, const double *y, int32_t n_levels,
                      int32_t n_hull, const double *hull_x, const double *hull_y, odr_schism **out) {
  REQUIRE(c && x && y && hull_x && hull_y && out, "NULL argument");
  REQUIRE(n_nodes >= 3 && n_nodes < (1 << 30), "%d nodes: the mean is over the three nearest", n_nodes);
  REQUIRE(n_levels >= 0 && n_levels <= UMESH_MAXSIGMA, "%d vertical levels (at most %d)", n_levels, UMESH_MAXSIGMA);
  REQUIRE(n_hull >= 3 && n_hull <= n_nodes, "a hull of %d vertices on a mesh of %d nodes", n_hull, n_nodes);
  REQUIRE(!proj || (proj->kind >= ODR_PROJ_LATLONG && proj->kind <= ODR_PROJ_STERE_OBLIQUE && proj->kind != PROJ_CURVILINEAR),
          "projection kind %d does not serve a mesh", proj ? proj->kind : 0);
  REQUIRE(all_finite(x, n_nodes) && all_finite(y, n_nodes), "a node position is not finite");
  REQUIRE(all_finite(hull_x, n_hull) && all_finite(hull_y, n_hull), "a hull vertex is not finite");
  std::vector<ShEdge> e;
  for (int k = 0; k < n_hull; ++k) {
    const int j = (k + 1) % n_hull;
    if (hull_x[k] != hull_x[j] || hull_y[k] != hull_y[j]) e.push_back(ShEdge{hull_x[k], hull_y[k], hull_x[j], hull_y[j]});
  }
  REQUIRE(e.size() >= 3, "the hull has %d edges of non-zero length", (int)e.size());
  std::vector<int> poly(e.size(), 0);
  ShIndex I;
  const std::string err = sh_build((long long)e.size(), e.data(), poly.data(), 1, 0, 0, 0, I);
  REQUIRE(err.empty(), "odr_schism_create: the hull: %s", err.c_str());
  HIPCHK(hipSetDevice(c->device));
  odr_schism *m = new odr_schism();
  memset(&m->dev, 0, sizeof m->dev);
  memset(m->level, 0, sizeof m->level);
  proj_init(m->proj, proj);
  m->n_nodes = n_nodes;
  m->n_levels = n_levels;
  ScMesh &M = m->dev;
  M.n_levels = n_levels;
  M.hull = I.g;
  M.hull.off = nullptr; M.hull.ent = nullptr; M.hull.tag = nullptr;
  const double xmin = *std::min_element(x, x + n_nodes);
  M.hull.lon_mode = m->proj.kind == PROJ_LATLONG ? (xmin < 0 ? 1 : 2) : 0;      // modulate_longitude, variables.py:259-280
  std::vector<UmPoint> pt;
  std::vector<int> id;
  um_build(n_nodes, x, y, pt, id);
  M.node.n = n_nodes;
  M.node.pad = 0;
  int rc = upload(c, m, pt.data(), sizeof(UmPoint) * (size_t)n_nodes, (const void **)&M.node.pt);
  if (!rc) rc = upload(c, m, id.data(), sizeof(int) * (size_t)n_nodes, (const void **)&M.node.id);
  if (!rc) rc = upload(c, m, I.off.data(), sizeof(long long) * I.off.size(), (const void **)&M.hull.off);
  if (!rc) rc = upload(c, m, I.ent.data(), sizeof(ShEdge) * I.ent.size(), (const void **)&M.hull.ent);
  if (!rc) rc = upload(c, m, I.tag.data(), sizeof(int) * I.tag.size(), (const void **)&M.hull.tag);
  if (rc) {
    release(m);
    return rc;
  }
  *out = m;
  return 0;
}

int odr_schism_destroy(odr_ctx *c, odr_schism *m) {
  REQUIRE(c, "NULL argument");
  if (!m) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  release(m);
  return 0;
}

// The vertical coordinate of the time level in `slot`: zcor [node][n_levels] float32, NaN below the sea bed.  Synchronous.
int odr_schism_set_zcor(odr_ctx *c, odr_schism *m, int32_t slot, double t_epoch, const float *zcor) {
  REQUIRE(c && m && zcor, "NULL argument");
  REQUIRE(slot >= 0 && slot < SCHISM_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot, SCHISM_MAXLEVELS);
  REQUIRE(m->n_levels > 0, "zcor on a mesh without vertical levels");
  const size_t nn = (size_t)m->n_nodes, nl = (size_t)m->n_levels;
  std::vector<long long> off(nn + 1);
  const long long points = sc_offsets(m->n_nodes, m->n_levels, zcor, off.data());
  REQUIRE(points >= 3, "zcor holds %lld finite entries: the mean is over the three nearest", points);
  HIPCHK(hipSetDevice(c->device));
  odr_schism::Level &L = m->level[slot];
  if (int rc = resident(c, (void **)&L.zcor, true, sizeof(float) * nn * nl)) return rc;
  if (int rc = resident(c, (void **)&L.off, true, sizeof(long long) * (nn + 1))) return rc;
  H2D(L.zcor, zcor, sizeof(float) * nn * nl);
  H2D(L.off, off.data(), sizeof(long long) * (nn + 1));
  L.t = t_epoch;
  return 0;
}

// One variable of one resident time level: [node] float32 (n_levels 0) or [node][n_levels].  Synchronous.
int odr_schism_set_level(odr_ctx *c, odr_schism *m, int32_t slot, double t_epoch, int32_t var, int32_t n_levels, const float *data) {
  REQUIRE(c && m && data, "NULL argument");
  REQUIRE(slot >= 0 && slot < SCHISM_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot, SCHISM_MAXLEVELS);
  REQUIRE(var >= 0 && var < NVAR, "bad variable id %d", var);
  REQUIRE(n_levels == 0 || (m->n_levels > 0 && n_levels == m->n_levels), "%d levels on a mesh of %d vertical levels", n_levels, m->n_levels);
  HIPCHK(hipSetDevice(c->device));
  odr_schism::Level &L = m->level[slot];
  const size_t floats = (size_t)(n_levels ? n_levels : 1) * (size_t)m->n_nodes;
  if (int rc = resident(c, (void **)&L.data[var], L.levels[var] == n_levels, sizeof(float) * floats)) return rc;
  L.levels[var] = n_levels;
  H2D(L.data[var], data, sizeof(float) * floats);
  L.t = t_epoch;
  return 0;
}

// Reader._get_variables_interpolated_ + the rotation and the priority-list merge for every element of the set, ONE launch; the
// positions stay on the device.  slot_after < 0: the values of slot_before alone (the time is that level's, or every variable of
// the call is static); else value = before * (1 - w) + after * w.  first_flags[k] != 0: the mesh is first in the list of variable k.
int odr_schism_sample(odr_ctx *c, odr_particles *p, odr_schism *m, int32_t slot_before, int32_t slot_after, double w, int32_t nvars,
                      const int32_t *var_ids, const int32_t *first_flags) {
  REQUIRE(c && p && m && var_ids && first_flags, "NULL argument");
  REQUIRE(slot_before >= 0 && slot_before < SCHISM_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot_before, SCHISM_MAXLEVELS);
  REQUIRE(slot_after < SCHISM_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot_after, SCHISM_MAXLEVELS);
  REQUIRE(slot_after < 0 || (w >= 0.0 && w <= 1.0), "a time weight of %g", w);
  REQUIRE(nvars >= 1 && nvars <= UMESH_MAXV, "%d variables: one launch serves 1 .. %d", nvars, UMESH_MAXV);
  const bool blend = slot_after >= 0;
  const odr_schism::Level &lb = m->level[slot_before], &la = m->level[blend ? slot_after : slot_before];
  int order[UMESH_MAXV], no = 0;      // an x component directly in front of its y component
  bool taken[UMESH_MAXV] = {false};
  for (int k = 0; k < nvars; ++k) {
    const int v = var_ids[k];
    REQUIRE(v >= 0 && v < NVAR, "bad variable id %d", v);
    for (int j = 0; j < k; ++j) REQUIRE(var_ids[j] != v, "variable %d given twice", v);
    if (!lb.data[v]) return fail(ODR_ERR_STATE, "time level %d of the mesh does not hold variable %d", slot_before, v);
    if (!la.data[v] || la.levels[v] != lb.levels[v])
      return fail(ODR_ERR_STATE, "time level %d of the mesh does not hold variable %d as level %d does", slot_after, v, slot_before);
    if (lb.levels[v] && (!lb.zcor || !la.zcor)) return fail(ODR_ERR_STATE, "variable %d has vertical levels and a time level is without zcor", v);
  }
  ScLaunch L;
  memset(&L, 0, sizeof L);
  for (int k = 0; k < nvars; ++k) {
    if (taken[k]) continue;
    int mate = -1;
    for (int j = 0; j < nvars; ++j)
      if (j != k && !taken[j] && (partner_of(var_ids[k]) == var_ids[j] || partner_of(var_ids[j]) == var_ids[k])) mate = j;
    if (mate < 0) {
      order[no++] = k;
      taken[k] = true;
      continue;
    }
    const int kx = partner_of(var_ids[k]) == var_ids[mate] ? k : mate, ky = kx == k ? mate : k;
    L.v[no].pair = 1;
    order[no++] = kx;
    order[no++] = ky;
    taken[kx] = taken[ky] = true;
  }
  L.nvars = nvars;
  L.blend = blend ? 1 : 0;
  L.w = blend ? w : 0.0;
  L.zb = lb.zcor;
  L.za = la.zcor;
  p->epoch++;      // invalidates the cached reductions (reduce())
  for (int k = 0; k < nvars; ++k) {
    const int v = var_ids[order[k]];
    if (!p->env[v]) {      // never sampled: nothing finite in the slot (every byte 0xff: a NaN)
      HIPCHK(hipMalloc((void **)&p->env[v], sizeof(float) * (size_t)p->cap));
      HIPCHK(hipMemsetAsync(p->env[v], 0xff, sizeof(float) * (size_t)p->cap, c->stream));
    }
    p->env_cok[v] = false;
    ScVar &V = L.v[k];
    V.b = lb.data[v];
    V.a = la.data[v];
    V.out = p->env[v];
    V.levels = lb.levels[v];
    V.first = first_flags[order[k]] != 0;
    (V.levels ? L.need3 : L.need2) = 1;
  }
  if (p->n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  KernelClock &clock = c->clock[CLOCK_SCHISM];
  clock.reset();
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_schism_sample, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, m->proj, m->dev, L, p->n, (const double *)p->d64[0],
                     (const double *)p->d64[1], (const double *)p->d64[2]);
  HIPCHK(hipGetLastError());
  return clock.stop(c->stream);
}

// The bare query: the three nearest points of each of n points in the mesh's own coordinates, ascending.  z NULL: among the nodes;
// else among node x level at the zcor of `slot`.  x, y, z, idx_out [n][3], dist_out [n][3], visits_out [n] (may be NULL): host.
// idx: the node, or the reference's numbering of the cloud (sc_ref_index); -1 / inf where the point is not finite.  Synchronous.
int odr_schism_nearest3(odr_ctx *c, odr_schism *m, int32_t slot, int64_t n, const double *x, const double *y, const double *z, int64_t *idx_out,
                        double *dist_out, int32_t *visits_out) {
  REQUIRE(c && m, "NULL argument");
  REQUIRE(n >= 0 && (n == 0 || (x && y && idx_out && dist_out)), "bad arguments");
  const float *zcor = nullptr;
  const long long *off = nullptr;
  if (z) {
    REQUIRE(slot >= 0 && slot < SCHISM_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot, SCHISM_MAXLEVELS);
    if (!m->level[slot].zcor) return fail(ODR_ERR_STATE, "time level %d of the mesh is without zcor", slot);
    zcor = m->level[slot].zcor;
    off = m->level[slot].off;
  }
  KernelClock &clock = c->clock[CLOCK_SCHISM];
  clock.reset();
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  const long long chunk = std::min<long long>(n, NEAREST_CHUNK);
  DevScope B;      // released on every way out
  double *d_xyz, *d_dist;
  long long *d_idx;
  int *d_vis = nullptr;
  if (int rc = B.alloc((void **)&d_xyz, sizeof(double) * 3 * (size_t)chunk)) return rc;
  if (int rc = B.alloc((void **)&d_dist, sizeof(double) * 3 * (size_t)chunk)) return rc;
  if (int rc = B.alloc((void **)&d_idx, sizeof(long long) * 3 * (size_t)chunk)) return rc;
  if (visits_out)
    if (int rc = B.alloc((void **)&d_vis, sizeof(int) * (size_t)chunk)) return rc;
  for (long long o = 0; o < n; o += chunk) {
    const long long k = std::min(chunk, (long long)n - o);
    H2D(d_xyz, x + o, sizeof(double) * (size_t)k);
    H2D(d_xyz + chunk, y + o, sizeof(double) * (size_t)k);
    if (z) H2D(d_xyz + 2 * chunk, z + o, sizeof(double) * (size_t)k);
    if (int rc = clock.start(c->stream)) return rc;
    hipLaunchKernelGGL(k_schism_nearest3, dim3(nblk(k)), dim3(BLOCK), 0, c->stream, m->dev.node, zcor, off, m->n_levels, k, (const double *)d_xyz,
                       (const double *)(d_xyz + chunk), (const double *)(d_xyz + 2 * chunk), d_idx, d_dist, d_vis);
    HIPCHK(hipGetLastError());
    if (int rc = clock.stop(c->stream)) return rc;
    D2H(idx_out + 3 * o, d_idx, sizeof(long long) * 3 * (size_t)k);      // waits for the stream: the next chunk may overwrite d_xyz
    D2H(dist_out + 3 * o, d_dist, sizeof(double) * 3 * (size_t)k);
    if (visits_out) D2H(visits_out + o, d_vis, sizeof(int) * (size_t)k);
  }
  return 0;
}

// Device time [ms] of the launches of this context's last odr_schism_nearest3, or of the launch of its last odr_schism_sample
int odr_schism_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_SCHISM].read(ms);
}
