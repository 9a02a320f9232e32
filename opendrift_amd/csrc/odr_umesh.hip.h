// Unstructured (triangular-mesh) readers: nearest node / nearest face centre, nearest sigma layer or level, nearest time level.
//
//   UnstructuredReader._nearest_node_ / _nearest_face_   readers/basereader/unstructured.py:150-186     um_nearest, k_umesh_nearest
//   Reader.get_variables                                 readers/reader_netCDF_CF_unstructured.py:213-330   k_umesh_sample
//   __nearest_node_sigma__ / __nearest_face_sigma__      :348-407, z_from_sigma :410-424                um_sigma_index
//   covers_positions_xy, check_arguments                 readers/basereader/variables.py:229-257, :376-382   um_covers
//   rotate_vectors                                       variables.py:59-109                            um_rotate
//
// The reference asks a 2-D scipy cKDTree for the nearest point.  Here the index is a LEFT-BALANCED k-d tree stored in level
// order: the children of node i are 2 i + 1 and 2 i + 2, the tree of n points has exactly n nodes and no pointers, the split
// axis of a node is its depth & 1 (depth = floor(log2(i + 1))), and the median split keeps the depth at ceil(log2(n + 1))
// whatever the spacing of the mesh -- a coastal mesh graded 100 : 1 costs what a uniform one costs, which a bucket grid does
// not.  The query is the stack-free walk (current node, previous node, best so far): the parent of i is (i + 1) / 2 - 1, so
// the way back up needs no stack, no per-thread array and no scratch memory.  It is exact: a far subtree is skipped only when
// the squared distance to its splitting line, formed as the point distances are, exceeds the best squared distance -- rounding
// is monotonic, so no point of that subtree can have a smaller float64 distance.  Squared distances are dx * dx + dy * dy in
// float64 with every operation rounded on its own (no fused multiply-add), as scipy forms them.
//
// Everything above the kernels is plain C++ and is compiled for the CPU by tests/umesh_host.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace odr {

constexpr int UMESH_MAXV = 8;         // variables of one k_umesh_sample launch
constexpr int UMESH_MAXLEVELS = 3;    // resident time levels of a mesh: the nearest ones of t0, t0 + dt / 2 and t0 + dt
constexpr int UMESH_MAXSIGMA = 128;   // sigma levels of a mesh

struct UmPoint { double x, y; };
struct UmIndex { const UmPoint *pt; const int *id; int n, pad; };      // node k of the tree: its point and the point's own index

__host__ __device__ __forceinline__ int um_depth(int i) { return 31 - __builtin_clz((unsigned)i + 1u); }

__host__ __device__ __forceinline__ double um_dist2(double qx, double qy, double px, double py) {
  const double dx = __dsub_rn(px, qx), dy = __dsub_rn(py, qy);
  return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
}

// Index (in the caller's numbering) of the point nearest to (qx, qy); -1 when no distance compares (a query that is not finite).
// d2 (may be NULL): the squared distance to it.
__host__ __device__ __forceinline__ int um_nearest(const UmIndex &T, double qx, double qy, double *d2 = nullptr) {
  const int n = T.n;
  int cur = 0, prev = -1, best = -1;
  double bd = INFINITY;
  while (cur >= 0) {
    const int parent = ((cur + 1) >> 1) - 1;
    if (cur >= n) {      // a child the tree does not have: straight back
      prev = cur;
      cur = parent;
      continue;
    }
    const bool down = prev == parent;      // entered from above: the node itself is a candidate
    const UmPoint p = T.pt[cur];
    if (down) {
      const double d = um_dist2(qx, qy, p.x, p.y);
      if (d < bd) { bd = d; best = cur; }
    }
    const double s = (um_depth(cur) & 1) ? __dsub_rn(qy, p.y) : __dsub_rn(qx, p.x);
    const int right = s > 0 ? 1 : 0;
    const int near = 2 * cur + 1 + right, far = 2 * cur + 2 - right;
    int next = parent;
    if (down) next = near;
    else if (prev == near && __dmul_rn(s, s) <= bd) next = far;
    prev = cur;
    cur = next;
  }
  if (d2) *d2 = bd;
  return best < 0 ? -1 : T.id[best];
}

// argmin(|sigma[:, idx] * h[idx] - z|), the first minimum (__nearest_node_sigma__ -> _vector_nearest_): the product is float32
// (both arrays are), the difference with the element's float64 z is float64.  sigma is [nlev][npts].
__host__ __device__ __forceinline__ int um_sigma_index(const float *sigma, long long npts, int nlev, long long idx, float h, double z) {
  int best = 0;
  double bd = 0.0;
  for (int k = 0; k < nlev; ++k) {
    const float depth = sigma[(long long)k * npts + idx] * h;
    const double a = fabs(__dsub_rn((double)depth, z));
    if (k == 0 || a < bd) { bd = a; best = k; }
  }
  return best;
}

// covers_positions_xy with the reader's default zmin / zmax: the bounding box of the nodes; x + y not finite is outside
__host__ __device__ __forceinline__ bool um_covers(double x, double y, double xmin, double xmax, double ymin, double ymax) {
  return std::isfinite(x + y) && x >= xmin && x <= xmax && y >= ymin && y <= ymax;
}

// the priority-list rule for a reader outside the device's own lists: a finite value is taken when the reader is first in the
// variable's list or the slot holds nothing finite
__host__ __device__ __forceinline__ float um_merge(float val, float cur, int first) {
  return std::isfinite(val) && (first || !std::isfinite(cur)) ? val : cur;
}

// rotate_vectors :104-107: float32 components times the float64 cosine and sine, stored as float32
__host__ __device__ __forceinline__ void um_rotate(float &u, float &v, double cs, double sn) {
  const double uu = (double)u, vv = (double)v;
  u = (float)__dsub_rn(__dmul_rn(uu, cs), __dmul_rn(vv, sn));
  v = (float)__dadd_rn(__dmul_rn(uu, sn), __dmul_rn(vv, cs));
}

// ---- the index, built once per mesh on the host
inline int um_left_size(int n) {      // nodes of the left subtree of a left-balanced tree of n nodes
  if (n <= 1) return 0;
  int m = 1;
  while (2 * m <= n) m *= 2;          // the last level starts at node m - 1 and holds n - m + 1 of its m places
  return m / 2 - 1 + std::min(n - m + 1, m / 2);
}

inline void um_build(int n, const double *x, const double *y, std::vector<UmPoint> &pt, std::vector<int> &id) {
  pt.resize((size_t)n);
  id.resize((size_t)n);
  std::vector<int> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0);
  struct Job { int lo, hi, node; };
  std::vector<Job> todo;
  todo.push_back({0, n, 0});
  while (!todo.empty()) {
    const Job j = todo.back();
    todo.pop_back();
    const int count = j.hi - j.lo;
    if (count <= 0) continue;
    const double *c = (um_depth(j.node) & 1) ? y : x;
    const int left = um_left_size(count);
    std::nth_element(perm.begin() + j.lo, perm.begin() + j.lo + left, perm.begin() + j.hi,
                     [c](int a, int b) { return c[a] < c[b] || (c[a] == c[b] && a < b); });
    const int m = perm[(size_t)(j.lo + left)];
    pt[(size_t)j.node] = {x[m], y[m]};
    id[(size_t)j.node] = m;
    todo.push_back({j.lo, j.lo + left, 2 * j.node + 1});
    todo.push_back({j.lo + left + 1, j.hi, 2 * j.node + 2});
  }
}

#ifndef ODR_UMESH_HOST
struct UmMesh {
  UmIndex node, face;
  double xmin, xmax, ymin, ymax;
  const float *siglay, *siglev, *siglay_c, *siglev_c, *h, *h_c;      // [n_siglay | n_siglay + 1][n_nodes | n_faces]; depths [n_nodes | n_faces]
  int n_siglay, lon_mode;      // lon_mode (geographic meshes): 1 = longitudes -180 .. 180, 2 = 0 .. 360 (modulate_longitude)
};
// pair: this variable is the x component and the next one of the launch its y component (rotated together)
struct UmVar { const float *data; float *out; int on_faces, n_levels, first, pair; };
struct UmLaunch { int nvars, need_node, need_face, pad; UmVar v[UMESH_MAXV]; };

__global__ __launch_bounds__(BLOCK) void k_umesh_nearest(UmIndex T, long long n, const double *__restrict__ x, const double *__restrict__ y,
                                                         int *__restrict__ out) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = um_nearest(T, x[i], y[i]);
}

// One element per lane: position -> mesh coordinates -> nearest node and / or face (one search each) -> per variable the sigma
// index, the gather from the resident time level, the rotation of vector pairs, the merge into the environment slot.
__global__ __launch_bounds__(BLOCK) void k_umesh_sample(DevProj P, UmMesh M, UmLaunch L, long long n, const double *__restrict__ lon,
                                                        const double *__restrict__ lat, const double *__restrict__ zs) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double x, y;
  if (P.kind == PROJ_LATLONG) {      // get_variables_interpolated: modulate_longitude, then lonlat2xy is the identity
    x = lon[i];
    y = lat[i];
    if (M.lon_mode == 1) x = np_mod(x + 180.0, 360.0) - 180.0;
    else if (M.lon_mode == 2) x = np_mod(x, 360.0);
  } else proj_fwd(P, lon[i], lat[i], x, y);
  if (!um_covers(x, y, M.xmin, M.xmax, M.ymin, M.ymax)) return;      // keeps what it has
  const double z = zs[i];
  const int in = L.need_node ? um_nearest(M.node, x, y) : -1;
  const int jf = L.need_face ? um_nearest(M.face, x, y) : -1;
  int prev_key = -1, prev_s = 0;      // neighbouring variables of one kind (u, v, w on the faces' layers) share one sigma search
  float val[UMESH_MAXV];
#pragma unroll
  for (int k = 0; k < UMESH_MAXV; ++k) {
    val[k] = NAN;
    if (k >= L.nvars) continue;
    const UmVar &V = L.v[k];
    const long long idx = V.on_faces ? jf : in, npts = V.on_faces ? M.face.n : M.node.n;
    if (idx < 0) continue;
    long long at = idx;
    if (V.n_levels > 0) {
      const int key = V.on_faces * (2 * UMESH_MAXSIGMA) + V.n_levels;
      if (key != prev_key) {
        const bool lay = V.n_levels == M.n_siglay;      // as the reference decides: by the level count (shp[1])
        const float *sigma = V.on_faces ? (lay ? M.siglay_c : M.siglev_c) : (lay ? M.siglay : M.siglev);
        prev_s = um_sigma_index(sigma, npts, V.n_levels, idx, (V.on_faces ? M.h_c : M.h)[idx], z);
        prev_key = key;
      }
      at += (long long)prev_s * npts;
    }
    val[k] = V.data[at];
  }
  bool rotates = false;
#pragma unroll
  for (int k = 0; k + 1 < UMESH_MAXV; ++k) rotates |= k + 1 < L.nvars && L.v[k].pair;
  if (rotates && P.kind != PROJ_LATLONG) {      // (a geographic mesh is not rotated, variables.py:800-802)
    double cs, sn;
    rotation_cs(P, x, y, cs, sn);
#pragma unroll
    for (int k = 0; k + 1 < UMESH_MAXV; ++k)
      if (k + 1 < L.nvars && L.v[k].pair) um_rotate(val[k], val[k + 1], cs, sn);
  }
#pragma unroll
  for (int k = 0; k < UMESH_MAXV; ++k)
    if (k < L.nvars) L.v[k].out[i] = um_merge(val[k], L.v[k].out[i], L.v[k].first);
}
#endif  // ODR_UMESH_HOST

}  // namespace odr
