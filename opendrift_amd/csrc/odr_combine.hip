// libodrift_hip.so, a translation unit of its own: reader operators (readers/operators/) -- sums of readers, a reader combined with a
// number and Gaussian blends, evaluated per element in one launch.  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_combine.hip.h"

struct odr_combined {
  int n_ops;
  CombOp op[COMB_MAXOPS];
  DevScope bufs;
  int *partial;      // device (in bufs), [MAXSRC]: k_combined_front -> k_combined_sample
};

namespace {

// what the kernel would read of source `sid` for variable `var` at time t is there
int leaf_ready(const odr_ctx *c, int sid, int var, double t) {
  const DevSource &s = c->hw.src[sid];
  if (s.kind != SRC_GRID) return 0;
  if (source_has_members(s)) return fail(ODR_ERR_INVALID, "source %d hands out ensemble members: not under a reader operator", sid);
  if (!s.always_valid && (t < s.tmin || t > s.tmax)) return 0;      // the kernel leaves such a source alone
  if (s.nlevels < 1) return fail(ODR_ERR_STATE, "source %d holds no time level", sid);
  int ib, ia;
  host_bracket(s, t, ib, ia);
  if (!s.slot[ib].data[var] || (ia >= 0 && !s.slot[ia].data[var]))
    return fail(ODR_ERR_STATE, "the resident time levels of source %d do not hold variable %d", sid, var);
  return 0;
}

}  // namespace

int odr_combined_create(odr_ctx *c, int32_t n_ops, const odr_combine_op *ops, odr_combined **out) {
  REQUIRE(c && ops && out, "NULL argument");
  REQUIRE(n_ops >= 1 && n_ops <= COMB_MAXOPS, "%d operations: a program has 1 .. %d", n_ops, COMB_MAXOPS);
  odr_combined *m = new odr_combined();
  m->partial = nullptr;
  m->n_ops = n_ops;
  for (int k = 0; k < n_ops; ++k) {
    m->op[k].kind = ops[k].kind;
    m->op[k].index = ops[k].index;
    for (int j = 0; j < 3; ++j) m->op[k].d[j] = ops[k].d[j];
  }
  const char *why = comb_check(m->op, n_ops, c->nsrc);
  for (int k = 0; !why && k < n_ops; ++k)
    if (m->op[k].kind == COMB_SOURCE && c->src_free[m->op[k].index]) why = "a source leaf names a released source";
  if (why) {
    delete m;
    return fail(ODR_ERR_INVALID, "odr_combined_create: %s", why);
  }
  if (hipSetDevice(c->device) != hipSuccess || m->bufs.alloc((void **)&m->partial, sizeof(int) * MAXSRC)) {
    delete m;
    return fail(ODR_ERR_HIP, "odr_combined_create: hipMalloc of the coverage flags");
  }
  *out = m;
  return 0;
}

int odr_combined_destroy(odr_ctx *c, odr_combined *m) {
  REQUIRE(c, "NULL argument");
  if (!m) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));      // a launch may still read the flags
  delete m;
  return 0;
}

// The expression's values + the priority-list merge for every element of the set: the front door (projection, coverage and the dtype class
// of every leaf, once per leaf whatever the number of variables), then ONE sampling launch; the positions stay on the device.
// first[k] != 0: the combined reader heads the list of variable k.  uniform_values: [nvars][n_uniform].
int odr_combined_sample(odr_ctx *c, odr_particles *p, odr_combined *m, int32_t nvars, const int32_t *var_ids, const uint8_t *first,
                        double t_epoch, int32_t n_uniform, const double *uniform_values) {
  REQUIRE(c && p && m && var_ids && first, "NULL argument");
  REQUIRE(nvars >= 1 && nvars <= COMB_MAXVARS, "%d variables: one launch serves 1 .. %d", nvars, COMB_MAXVARS);
  REQUIRE(n_uniform >= 0 && n_uniform <= COMB_MAXUNI && (n_uniform == 0 || uniform_values), "%d uniform leaves (at most %d), or their values are missing",
          n_uniform, COMB_MAXUNI);
  for (int k = 0; k < nvars; ++k) {
    REQUIRE(var_ids[k] >= 0 && var_ids[k] < NVAR, "bad variable id %d", var_ids[k]);
    for (int j = 0; j < k; ++j) REQUIRE(var_ids[j] != var_ids[k], "variable %d given twice", var_ids[k]);
  }
  for (int k = 0; k < m->n_ops; ++k) {
    const CombOp &o = m->op[k];
    if (o.kind == COMB_SOURCE) {
      REQUIRE(o.index < c->nsrc && !c->src_free[o.index], "source %d of the program has been released", o.index);
      for (int v = 0; v < nvars; ++v) if (int rc = leaf_ready(c, o.index, var_ids[v], t_epoch)) return rc;
    } else if (o.kind == COMB_UNIFORM || o.kind == COMB_GAUSS_TERM) {
      REQUIRE(o.index < n_uniform, "the program reads uniform leaf %d, %d were given", o.index, n_uniform);
    }
  }
  CombLaunch L;
  memset(&L, 0, sizeof L);
  L.n_ops = m->n_ops;
  memcpy(L.op, m->op, sizeof(CombOp) * (size_t)m->n_ops);
  L.n_vars = nvars;
  HIPCHK(hipSetDevice(c->device));
  p->epoch++;      // invalidates the cached reductions (reduce())
  for (int k = 0; k < nvars; ++k) {
    const int v = var_ids[k];
    if (!p->env[v]) {      // never sampled: nothing finite in the slot (every byte 0xff: a NaN)
      HIPCHK(hipMalloc((void **)&p->env[v], sizeof(float) * (size_t)p->cap));
      HIPCHK(hipMemsetAsync(p->env[v], 0xff, sizeof(float) * (size_t)p->cap, c->stream));
    }
    p->env_cok[v] = false;
    L.var[k] = v;
    L.first[k] = first[k] != 0;
    L.out[k] = p->env[v];
    for (int u = 0; u < n_uniform; ++u) L.uni[k * COMB_MAXUNI + u] = uniform_values[(size_t)k * (size_t)n_uniform + (size_t)u];
  }
  if (p->n == 0) return 0;
  if (int rc = flush_world(c)) return rc;
  // the positions in the leaves' own coordinates: [source leaf in program order][x, y][n] doubles in the set's scratch memory
  int n_leaves = 0;
  for (int k = 0; k < m->n_ops; ++k) n_leaves += m->op[k].kind == COMB_SOURCE;
  double *xy = nullptr;
  if (int rc = scratch(c, p, sizeof(double) * 2 * (size_t)std::max(n_leaves, 1) * (size_t)p->n, (void **)&xy)) return rc;
  HIPCHK(hipMemsetAsync(m->partial, 0, sizeof(int) * MAXSRC, c->stream));
  KernelClock &clock = c->clock[CLOCK_COMBINED];
  clock.reset();
  if (int rc = clock.start(c->stream)) return rc;
  hipLaunchKernelGGL(k_combined_front, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, c->dw, L, p->n, (const double *)p->d64[0],
                     (const double *)p->d64[1], (const double *)p->d64[2], t_epoch, m->partial, xy);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_combined_sample, dim3(nblk(p->n)), dim3(BLOCK), 0, c->stream, c->dw, L, p->n, (const double *)p->d64[0],
                     (const double *)p->d64[1], (const double *)p->d64[2], t_epoch, (const int *)m->partial, (const double *)xy);
  HIPCHK(hipGetLastError());
  return clock.stop(c->stream);
}

// Device time [ms] of the two launches of this context's last odr_combined_sample (waits for them)
int odr_combined_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_COMBINED].read(ms);
}
