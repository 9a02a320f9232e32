// libodrift_hip.so, a translation unit of its own: unstructured (triangular-mesh) readers -- nearest node / face centre, nearest
// sigma layer or level, nearest time level (readers/basereader/unstructured.py, readers/reader_netCDF_CF_unstructured.py).
// See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_umesh.hip.h"

struct odr_umesh {
  UmMesh dev;
  DevProj proj;
  int n_nodes, n_faces;
  DevScope bufs;      // coordinates, index and sigma arrays
  struct Level {
    double t;
    float *data[NVAR];
    size_t floats[NVAR];
    int on_faces[NVAR], n_levels[NVAR];
  } level[UMESH_MAXLEVELS];
};

namespace {

constexpr long long NEAREST_CHUNK = 1ll << 20;      // points of one odr_umesh_nearest launch

bool all_finite(const double *a, long long n) {
  for (long long k = 0; k < n; ++k) if (!std::isfinite(a[k])) return false;
  return true;
}

int upload(odr_ctx *c, odr_umesh *m, const void *host, size_t bytes, const void **dev) {
  void *p;
  if (int rc = m->bufs.alloc(&p, bytes)) return rc;
  H2D(p, host, bytes);
  *dev = p;
  return 0;
}

int upload_index(odr_ctx *c, odr_umesh *m, int n, const double *x, const double *y, UmIndex &T) {
  std::vector<UmPoint> pt;
  std::vector<int> id;
  um_build(n, x, y, pt, id);
  T.n = n;
  T.pad = 0;
  if (int rc = upload(c, m, pt.data(), sizeof(UmPoint) * (size_t)n, (const void **)&T.pt)) return rc;
  return upload(c, m, id.data(), sizeof(int) * (size_t)n, (const void **)&T.id);
}

void release(odr_umesh *m) {
  for (auto &L : m->level)      // (replaced in place by odr_umesh_set_level: not in bufs)
    for (float *p : L.data) if (p) (void)hipFree(p);
  delete m;
}

int partner_of(int var) {      // the y component of a vector pair's x component (vector_pairs_xy, variables.py)
  return var == VAR_U ? VAR_V : var == VAR_XWIND ? VAR_YWIND : var == VAR_SX ? VAR_SY : var == VAR_ICE_U ? VAR_ICE_V : -1;
}

}  // namespace

// The mesh on the device: the two search indices (built here, on the host, once), the box of the nodes, the sigma and depth arrays.
int odr_umesh_create(odr_ctx *c, const odr_proj_desc *proj, int32_t n_nodes, const double *x, const double *y, int32_t n_faces,
                     const double *xc, const double *yc, int32_t n_siglay, const float *siglay, const float *siglev,
                     const float *siglay_center, const float *siglev_center, const float *h, const float *h_center, odr_umesh **out) {
  REQUIRE(c && x && y && out, "NULL argument");
  REQUIRE(n_nodes >= 1 && n_nodes < (1 << 30), "%d nodes", n_nodes);
  REQUIRE(n_faces >= 0 && n_faces < (1 << 30) && (n_faces == 0 || (xc && yc)), "%d faces, or their centres are missing", n_faces);
  REQUIRE(n_siglay >= 0 && n_siglay < UMESH_MAXSIGMA, "%d sigma layers (at most %d)", n_siglay, UMESH_MAXSIGMA - 1);
  REQUIRE(!proj || (proj->kind >= ODR_PROJ_LATLONG && proj->kind <= ODR_PROJ_STERE_OBLIQUE && proj->kind != PROJ_CURVILINEAR),
          "projection kind %d does not serve a mesh", proj ? proj->kind : 0);
  REQUIRE(all_finite(x, n_nodes) && all_finite(y, n_nodes), "a node position is not finite");
  REQUIRE(all_finite(xc, n_faces) && all_finite(yc, n_faces), "a face centre is not finite");
  // sigma arrays come with their depth: (siglay | siglev, h) on the nodes, (siglay_center | siglev_center, h_center) on the faces
  REQUIRE(n_siglay > 0 || !(siglay || siglev || siglay_center || siglev_center), "sigma arrays without a layer count");
  REQUIRE(!(siglay || siglev) || h, "sigma arrays on the nodes without the depth h");
  REQUIRE(!(siglay_center || siglev_center) || (h_center && n_faces > 0), "sigma arrays on the faces without the depth h_center");
  HIPCHK(hipSetDevice(c->device));
  odr_umesh *m = new odr_umesh();
  memset(&m->dev, 0, sizeof m->dev);
  memset(m->level, 0, sizeof m->level);
  proj_init(m->proj, proj);
  m->n_nodes = n_nodes;
  m->n_faces = n_faces;
  UmMesh &M = m->dev;
  M.xmin = *std::min_element(x, x + n_nodes); M.xmax = *std::max_element(x, x + n_nodes);
  M.ymin = *std::min_element(y, y + n_nodes); M.ymax = *std::max_element(y, y + n_nodes);
  M.n_siglay = n_siglay;
  M.lon_mode = m->proj.kind == PROJ_LATLONG ? (M.xmin < 0 ? 1 : 2) : 0;      // modulate_longitude, variables.py:259-280
  int rc = upload_index(c, m, n_nodes, x, y, M.node);
  if (!rc && n_faces > 0) rc = upload_index(c, m, n_faces, xc, yc, M.face);
  const size_t nn = (size_t)n_nodes, nf = (size_t)n_faces, L = (size_t)n_siglay;
  if (!rc && siglay) rc = upload(c, m, siglay, 4 * L * nn, (const void **)&M.siglay);
  if (!rc && siglev) rc = upload(c, m, siglev, 4 * (L + 1) * nn, (const void **)&M.siglev);
  if (!rc && h) rc = upload(c, m, h, 4 * nn, (const void **)&M.h);
  if (!rc && siglay_center) rc = upload(c, m, siglay_center, 4 * L * nf, (const void **)&M.siglay_c);
  if (!rc && siglev_center) rc = upload(c, m, siglev_center, 4 * (L + 1) * nf, (const void **)&M.siglev_c);
  if (!rc && h_center && n_faces > 0) rc = upload(c, m, h_center, 4 * nf, (const void **)&M.h_c);
  if (rc) {
    release(m);
    return rc;
  }
  *out = m;
  return 0;
}

int odr_umesh_destroy(odr_ctx *c, odr_umesh *m) {
  REQUIRE(c, "NULL argument");
  if (!m) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  release(m);
  return 0;
}

// One variable of one resident time level: [n_levels][points] float32, or [points] with n_levels 0.  Synchronous.
int odr_umesh_set_level(odr_ctx *c, odr_umesh *m, int32_t slot, double t_epoch, int32_t var, int on_faces, int32_t n_levels,
                        const float *data) {
  REQUIRE(c && m && data, "NULL argument");
  REQUIRE(slot >= 0 && slot < UMESH_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot, UMESH_MAXLEVELS);
  REQUIRE(var >= 0 && var < NVAR, "bad variable id %d", var);
  REQUIRE(!on_faces || m->n_faces > 0, "a face variable on a mesh without faces");
  const UmMesh &M = m->dev;
  if (n_levels != 0) {
    REQUIRE(M.n_siglay > 0 && (n_levels == M.n_siglay || n_levels == M.n_siglay + 1), "%d levels on a mesh of %d sigma layers", n_levels,
            M.n_siglay);
    const bool lay = n_levels == M.n_siglay;
    const float *sigma = on_faces ? (lay ? M.siglay_c : M.siglev_c) : (lay ? M.siglay : M.siglev);
    REQUIRE(sigma && (on_faces ? M.h_c : M.h), "a variable with %d levels on the %s needs the mesh's %s%s and %s", n_levels,
            on_faces ? "faces" : "nodes", lay ? "siglay" : "siglev", on_faces ? "_center" : "", on_faces ? "h_center" : "h");
  }
  HIPCHK(hipSetDevice(c->device));
  odr_umesh::Level &L = m->level[slot];
  const size_t floats = (size_t)(n_levels ? n_levels : 1) * (size_t)(on_faces ? m->n_faces : m->n_nodes);
  if (L.floats[var] != floats) {
    HIPCHK(hipStreamSynchronize(c->stream));      // a launch may still read the array this one replaces
    if (L.data[var]) HIPCHK(hipFree(L.data[var]));
    L.data[var] = nullptr;
    L.floats[var] = 0;
    HIPCHK(hipMalloc((void **)&L.data[var], sizeof(float) * floats));
    L.floats[var] = floats;
  }
  H2D(L.data[var], data, sizeof(float) * floats);
  L.t = t_epoch;
  L.on_faces[var] = on_faces != 0;
  L.n_levels[var] = n_levels;
  return 0;
}

// Reader.get_variables + the rotation and the priority-list merge for every element of the set, ONE launch; the positions stay
// on the device.  var_ids: each served by the level `slot`; first_flags[k] != 0: the mesh is first in the list of variable k.
int odr_umesh_sample(odr_ctx *c, odr_particles *p, odr_umesh *m, int32_t slot, int32_t nvars, const int32_t *var_ids,
                     const int32_t *first_flags) {
  REQUIRE(c && p && m && var_ids && first_flags, "NULL argument");
  REQUIRE(slot >= 0 && slot < UMESH_MAXLEVELS, "slot %d: a mesh holds %d time levels", slot, UMESH_MAXLEVELS);
  REQUIRE(nvars >= 1 && nvars <= UMESH_MAXV, "%d variables: one launch serves 1 .. %d", nvars, UMESH_MAXV);
  const odr_umesh::Level &lv = m->level[slot];
  int order[UMESH_MAXV], no = 0;      // an x component directly in front of its y component
  bool taken[UMESH_MAXV] = {false};
  for (int k = 0; k < nvars; ++k) {
    const int v = var_ids[k];
    REQUIRE(v >= 0 && v < NVAR, "bad variable id %d", v);
    for (int j = 0; j < k; ++j) REQUIRE(var_ids[j] != v, "variable %d given twice", v);
    if (!lv.data[v]) return fail(ODR_ERR_STATE, "time level %d of the mesh does not hold variable %d", slot, v);
  }
  UmLaunch L;
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
  p->epoch++;      // invalidates the cached reductions (reduce())
  for (int k = 0; k < nvars; ++k) {
    const int v = var_ids[order[k]];
    if (!p->env[v]) {      // never sampled: nothing finite in the slot (every byte 0xff: a NaN)
      HIPCHK(hipMalloc((void **)&p->env[v], sizeof(float) * (size_t)p->cap));
      HIPCHK(hipMemsetAsync(p->env[v], 0xff, sizeof(float) * (size_t)p->cap, c->stream));
    }
    p->env_cok[v] = false;
    UmVar &V = L.v[k];
    V.data = lv.data[v];
    V.out = p->env[v];
    V.on_faces = lv.on_faces[v];
    V.n_levels = lv.n_levels[v];
    V.first = first_flags[order[k]] != 0;
    (V.on_faces ? L.need_face : L.need_node) = 1;
  }
  if (p->n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  KernelClock &clock = c->clock[CLOCK_UMESH];
  clock.reset();
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_umesh_sample, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, m->proj, m->dev, L, p->n, (const double *)p->d64[0],
                     (const double *)p->d64[1], (const double *)p->d64[2]);
  HIPCHK(hipGetLastError());
  return clock.stop(c->stream);
}

// The bare query: the index of the node (on_faces 0) or face centre nearest to each of n points in the mesh's own coordinates.
// x, y, idx_out: host.  -1 for a point that is not finite.  Synchronous.
int odr_umesh_nearest(odr_ctx *c, odr_umesh *m, int on_faces, int64_t n, const double *x, const double *y, int32_t *idx_out) {
  REQUIRE(c && m, "NULL argument");
  REQUIRE(n >= 0 && (n == 0 || (x && y && idx_out)), "bad arguments");
  REQUIRE(!on_faces || m->n_faces > 0, "the mesh has no faces");
  KernelClock &clock = c->clock[CLOCK_UMESH];
  clock.reset();
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  const UmIndex &T = on_faces ? m->dev.face : m->dev.node;
  const long long chunk = std::min<long long>(n, NEAREST_CHUNK);
  DevScope B;      // released on every way out
  double *d_xy;
  int *d_idx;
  if (int rc = B.alloc((void **)&d_xy, sizeof(double) * 2 * (size_t)chunk)) return rc;
  if (int rc = B.alloc((void **)&d_idx, sizeof(int) * (size_t)chunk)) return rc;
  for (long long o = 0; o < n; o += chunk) {
    const long long k = std::min(chunk, n - o);
    H2D(d_xy, x + o, sizeof(double) * (size_t)k);
    H2D(d_xy + chunk, y + o, sizeof(double) * (size_t)k);
    if (int rc = clock.start(c->stream)) return rc;
    hipLaunchKernelGGL(k_umesh_nearest, dim3(nblk(k)), dim3(BLOCK), 0, c->stream, T, k, (const double *)d_xy, (const double *)(d_xy + chunk), d_idx);
    HIPCHK(hipGetLastError());
    if (int rc = clock.stop(c->stream)) return rc;
    D2H(idx_out + o, d_idx, sizeof(int) * (size_t)k);      // waits for the stream: the next chunk may overwrite d_xy
  }
  return 0;
}

// Device time [ms] of the launches of this context's last odr_umesh_nearest, or of the launch of its last odr_umesh_sample
int odr_umesh_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_UMESH].read(ms);
}
