// TEST INFRASTRUCTURE: the search index, the sigma rule, the coverage test, the rotation and the merge of
// opendrift_amd/csrc/odr_umesh.hip.h (the device code of readers.UnstructuredReader) compiled for the CPU with g++
// -ffp-contract=off, so that they can be compared with scipy's cKDTree and with the reference's values without a GPU
// (tests/test_umesh_device_arithmetic.py).  tests/hostshim stands in for <hip/hip_runtime.h>; the kernels are excluded by
// ODR_UMESH_HOST.  The loops do what the kernels do with one element.
#include <hip/hip_runtime.h>

#define ODR_UMESH_HOST 1
#include "../opendrift_amd/csrc/odr_umesh.hip.h"

struct umh_index {
  std::vector<odr::UmPoint> pt;
  std::vector<int> id;
  odr::UmIndex view() const { return odr::UmIndex{pt.data(), id.data(), (int)pt.size(), 0}; }
};

extern "C" umh_index *umh_build(int n, const double *x, const double *y) {
  umh_index *T = new umh_index();
  odr::um_build(n, x, y, T->pt, T->id);
  return T;
}
extern "C" void umh_free(umh_index *T) { delete T; }

// the tree as it is uploaded: node k holds point id[k] at (px[k], py[k])
extern "C" void umh_layout(const umh_index *T, double *px, double *py, int *id) {
  for (size_t k = 0; k < T->pt.size(); ++k) { px[k] = T->pt[k].x; py[k] = T->pt[k].y; id[k] = T->id[k]; }
}

extern "C" void umh_nearest(const umh_index *T, long long n, const double *x, const double *y, int *out, double *d2) {
  const odr::UmIndex V = T->view();
  for (long long i = 0; i < n; ++i) out[i] = odr::um_nearest(V, x[i], y[i], d2 ? d2 + i : nullptr);
}

// One variable for n elements whose nearest point is idx[i] (x, y: mesh coordinates, for the coverage test): out[i] becomes the
// merged value.  sigma / h NULL or n_levels 0: a 2-D variable.  sigma_out (may be NULL): the sigma index, -1 outside coverage.
extern "C" void umh_sample(long long n, const double *x, const double *y, const double *z, const int *idx, const double *box, long long npts,
                           int n_levels, const float *sigma, const float *h, const float *data, int first, float *out, int *sigma_out) {
  for (long long i = 0; i < n; ++i) {
    if (sigma_out) sigma_out[i] = -1;
    if (!odr::um_covers(x[i], y[i], box[0], box[1], box[2], box[3]) || idx[i] < 0) continue;
    long long at = idx[i];
    if (n_levels > 0) {
      const int s = odr::um_sigma_index(sigma, npts, n_levels, idx[i], h[idx[i]], z[i]);
      if (sigma_out) sigma_out[i] = s;
      at += (long long)s * npts;
    }
    out[i] = odr::um_merge(data[at], out[i], first);
  }
}

extern "C" void umh_rotate(long long n, float *u, float *v, const double *cs, const double *sn) {
  for (long long i = 0; i < n; ++i) odr::um_rotate(u[i], v[i], cs[i], sn[i]);
}
