// TEST INFRASTRUCTURE: the three-nearest search in 2-D and over the columnar 3-D cloud, the weights, the time blend, the hull test,
// the rotation and the merge of opendrift_amd/csrc/odr_schism.hip.h (the device code of readers.SchismReader) compiled for the CPU
// with g++ -ffp-contract=off, so that they can be compared with scipy's cKDTree and with the reference's values without a GPU
// (tests/test_schism_device_arithmetic.py).  tests/hostshim stands in for <hip/hip_runtime.h>; the kernels are excluded by
// ODR_SCHISM_HOST.  The loops do what the kernels do with one element.
#include <hip/hip_runtime.h>

#define ODR_SCHISM_HOST 1
#include "../opendrift_amd/csrc/odr_schism.hip.h"

struct sch_mesh {
  std::vector<odr::UmPoint> pt;
  std::vector<int> id;
  odr::ShIndex hull;
  bool has_hull = false;
  odr::UmIndex view() const { return odr::UmIndex{pt.data(), id.data(), (int)pt.size(), 0}; }
};

// hull_x / hull_y may be NULL (nh 0): a mesh for the bare search only.  NULL when the hull's grid cannot be built.
extern "C" sch_mesh *sch_build(int n, const double *x, const double *y, int nh, const double *hx, const double *hy) {
  sch_mesh *M = new sch_mesh();
  odr::um_build(n, x, y, M->pt, M->id);
  if (nh > 0) {
    std::vector<odr::ShEdge> e;
    for (int k = 0; k < nh; ++k) e.push_back(odr::ShEdge{hx[k], hy[k], hx[(k + 1) % nh], hy[(k + 1) % nh]});
    std::vector<int> poly(e.size(), 0);
    if (!odr::sh_build((long long)e.size(), e.data(), poly.data(), 1, 0, 0, 0, M->hull).empty()) {
      delete M;
      return nullptr;
    }
    M->has_hull = true;
  }
  return M;
}
extern "C" void sch_free(sch_mesh *M) { delete M; }

// zcor NULL: among the nodes; else [n_nodes][L].  idx [n][3], dist [n][3], visits [n] (may be NULL)
extern "C" void sch_nearest3(const sch_mesh *M, const float *zcor, int L, long long n, const double *x, const double *y, const double *z,
                             long long *idx, double *dist, int *visits) {
  const odr::UmIndex T = M->view();
  std::vector<long long> off;
  if (zcor) {
    off.resize((size_t)T.n + 1);
    odr::sc_offsets(T.n, L, zcor, off.data());
  }
  for (long long i = 0; i < n; ++i) {
    const int seen = odr::sc_nearest3(T, zcor, zcor ? off.data() : nullptr, L, x[i], y[i], zcor ? z[i] : 0.0, idx + 3 * i, dist + 3 * i);
    if (visits) visits[i] = seen;
  }
}

extern "C" void sch_covers(const sch_mesh *M, long long n, const double *x, const double *y, int *out) {
  for (long long i = 0; i < n; ++i) out[i] = odr::sc_covers(M->hull.g, x[i], y[i]) ? 1 : 0;
}

// One variable, or a vector pair (nv 2: b[0] / a[0] the x component), for n elements at (x, y, z) in mesh coordinates: levels 0: planes
// [node]; else [node][levels] with zcor zb / za.  blend 0: the level `b` alone.  cs / sn NULL: no rotation.  out[v][i] becomes the
// merged value.
extern "C" void sch_sample(const sch_mesh *M, long long n, const double *x, const double *y, const double *z, int levels, const float *zb,
                           const float *za, int blend, double w, int nv, const float *const *b, const float *const *a, const double *cs,
                           const double *sn, int first, float *const *out) {
  const odr::UmIndex T = M->view();
  for (long long i = 0; i < n; ++i) {
    if (!odr::sc_covers(M->hull.g, x[i], y[i])) continue;
    odr::Sc3 B;
    odr::ScW Wb, Wa;
    odr::sc_none(Wa);
    if (levels) odr::sc_search<true>(T, zb, levels, x[i], y[i], z[i], B);
    else odr::sc_search<false>(T, nullptr, 0, x[i], y[i], 0.0, B);
    odr::sc_weights(B, levels, Wb);
    if (blend && levels) {
      odr::sc_search<true>(T, za, levels, x[i], y[i], z[i], B);
      odr::sc_weights(B, levels, Wa);
    } else Wa = Wb;
    double val[2] = {NAN, NAN};
    for (int v = 0; v < nv; ++v) {
      val[v] = odr::sc_value(b[v], Wb);
      if (blend) val[v] = (double)(float)odr::sc_blend(val[v], odr::sc_value(a[v], Wa), w);
    }
    if (nv == 2 && cs) odr::sc_rotate(val[0], val[1], cs[i], sn[i]);
    for (int v = 0; v < nv; ++v) out[v][i] = odr::um_merge((float)val[v], out[v][i], first);
  }
}
