// SCHISM-style mesh reader: inverse-distance mean over the three nearest points of a time level's cloud, two time levels blended.
//
//   ReaderBlockUnstruct.interpolate            readers/reader_schism_native.py:982-1056     sc_search, sc_weights, sc_value
//   Reader.convert_3d_to_array                 :384-438                                      the cloud of a 3-D level, sc_ref_index
//   Reader._get_variables_interpolated_        :440-677 (the time weights :614-642)          sc_blend, k_schism_sample
//   covers_positions (convex hull of the nodes) readers/basereader/unstructured.py:76-144    sc_covers (sh_contains of odr_shape.hip.h)
//   rotate_vectors                             readers/basereader/variables.py:59-109        sc_rotate
//
// A time level is a cloud of points: the nodes (2-D variables), or node x vertical level at the level's own zcor (3-D variables;
// NaN: below the sea bed of that node).  The reference asks a 2-D or a 3-D scipy cKDTree for the three nearest points.
//
// 2-D: the left-balanced tree of odr_umesh.hip.h and its stack-free walk, keeping the best THREE: three (d2, index) pairs in
// named scalars, inserted by compare-and-shift (nothing is indexed at run time).  A far subtree is skipped only when the squared
// distance to its splitting line exceeds the third best squared distance; rounding is monotonic, so the argument of the nearest
// search carries over: the three are exact.
//
// 3-D, WITHOUT a 3-D tree: the cloud is columnar -- every point of node n has the node's (x, y) -- and its squared distance
//     fl(fl(dx2 + dy2) + dz2) >= fl(dx2 + dy2) >= the squared distance to any splitting line between the query and n,
// so the SAME 2-D tree is walked, pruned on the horizontal squared distance against the third best 3-D squared distance, and
// every visited node whose horizontal squared distance is below that bound offers the finite levels of its column.  The tree is
// built once per mesh; a time level costs the upload of its zcor plane and data planes.  zcor and the 3-D planes are [node][level]
// (SCHISM's own order): a lane owns a column and reads it as one run of consecutive floats.
//
// Distances are formed as scipy forms them: squared differences added in axis order, each operation rounded on its own, the
// square root at the end.  Weights, sums and the time blend are float64 in the reference's operation order with no fused
// multiply-add; a host build gives the device's bits.  Everything above the kernels is plain C++ and is compiled for the CPU by
// tests/schism_host.cpp.
#pragma once
// the arithmetic of the mesh and shape units without their kernels: those are defined in the units that launch them
#ifndef ODR_UMESH_HOST
#define ODR_UMESH_HOST 1
#endif
#ifndef ODR_SHAPE_HOST
#define ODR_SHAPE_HOST 1
#endif
#include "odr_shape.hip.h"
#include "odr_umesh.hip.h"

namespace odr {

constexpr int SCHISM_MAXLEVELS = 4;      // resident time levels of a mesh: the levels that bracket t0, t0 + dt / 2 and t0 + dt
constexpr double SCHISM_DMIN = 1e-10;    // DMIN of interpolate (:1019)

// IEEE division and square root, one rounding each
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double sc_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double sc_sqrt(double a) { return __dsqrt_rn(a); }
#else
inline double sc_div(double a, double b) { return a / b; }
inline double sc_sqrt(double a) { return std::sqrt(a); }
#endif

// The best three of a search, ascending: d = squared distance; i = node of the TREE (2-D search) or the node's own index (3-D
// search), -1: none; k = vertical level (3-D search).
struct Sc3 {
  double d0, d1, d2;
  int i0, i1, i2;
  int k0, k1, k2;
};

__host__ __device__ __forceinline__ void sc_clear(Sc3 &B) {
  B.d0 = B.d1 = B.d2 = INFINITY;
  B.i0 = B.i1 = B.i2 = -1;
  B.k0 = B.k1 = B.k2 = 0;
}

// compare-and-shift insert; a candidate that ties with a kept one goes behind it; a distance that does not compare is dropped
__host__ __device__ __forceinline__ void sc_offer(Sc3 &B, double d, int i, int k) {
  if (!(d < B.d2)) return;
  if (d < B.d1) {
    B.d2 = B.d1; B.i2 = B.i1; B.k2 = B.k1;
    if (d < B.d0) {
      B.d1 = B.d0; B.i1 = B.i0; B.k1 = B.k0;
      B.d0 = d; B.i0 = i; B.k0 = k;
    } else {
      B.d1 = d; B.i1 = i; B.k1 = k;
    }
  } else {
    B.d2 = d; B.i2 = i; B.k2 = k;
  }
}

// The three nearest points of (qx, qy) among the nodes (COLUMNS false), or of (qx, qy, qz) among node x level at zcor [node][L]
// (COLUMNS true).  Returns the number of tree nodes whose distance was formed.
template <bool COLUMNS>
__host__ __device__ __forceinline__ int sc_search(const UmIndex &T, const float *__restrict__ zcor, int L, double qx, double qy, double qz,
                                                  Sc3 &B) {
  const int n = T.n;
  int cur = 0, prev = -1, seen = 0;
  sc_clear(B);
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
      const double h = um_dist2(qx, qy, p.x, p.y);
      ++seen;
      if (!COLUMNS) sc_offer(B, h, cur, 0);
      else if (h < B.d2) {      // no level of the column can be nearer than its node is in the plane
        const int node = T.id[cur];
        const float *col = zcor + (long long)node * L;
        for (int k = 0; k < L; ++k) {
          const double dz = __dsub_rn((double)col[k], qz);      // (a NaN level, or a NaN depth, never compares)
          sc_offer(B, __dadd_rn(h, __dmul_rn(dz, dz)), node, k);
        }
      }
    }
    const double s = (um_depth(cur) & 1) ? __dsub_rn(qy, p.y) : __dsub_rn(qx, p.x);
    const int right = s > 0 ? 1 : 0;
    const int near = 2 * cur + 1 + right, far = 2 * cur + 2 - right;
    int next = parent;
    if (down) next = near;
    else if (prev == near && __dmul_rn(s, s) <= B.d2) next = far;
    prev = cur;
    cur = next;
  }
  if (!COLUMNS) {      // tree nodes -> the nodes' own indices
    if (B.i0 >= 0) B.i0 = T.id[B.i0];
    if (B.i1 >= 0) B.i1 = T.id[B.i1];
    if (B.i2 >= 0) B.i2 = T.id[B.i2];
  }
  return seen;
}

// Where the three are in a data plane ([node] or [node][L]) and their weights 1 / max(distance, DMIN); fs = (f0 + f1) + f2.
// a0 < 0: the search found fewer than three points (a query that is not finite): the value is missing.
struct ScW {
  double f0, f1, f2, fs;
  long long a0, a1, a2;
};

__host__ __device__ __forceinline__ double sc_fac(double d2) {
  double r = sc_sqrt(d2);
  if (r < SCHISM_DMIN) r = SCHISM_DMIN;
  return sc_div(1.0, r);
}

__host__ __device__ __forceinline__ void sc_none(ScW &W) {
  W.a0 = W.a1 = W.a2 = -1;
  W.f0 = W.f1 = W.f2 = W.fs = NAN;
}

__host__ __device__ __forceinline__ void sc_weights(const Sc3 &B, int L /* 0: a 2-D search */, ScW &W) {
  if (B.i2 < 0) {
    sc_none(W);
    return;
  }
  W.a0 = L ? (long long)B.i0 * L + B.k0 : B.i0;
  W.a1 = L ? (long long)B.i1 * L + B.k1 : B.i1;
  W.a2 = L ? (long long)B.i2 * L + B.k2 : B.i2;
  W.f0 = sc_fac(B.d0);
  W.f1 = sc_fac(B.d1);
  W.f2 = sc_fac(B.d2);
  W.fs = __dadd_rn(__dadd_rn(W.f0, W.f1), W.f2);
}

// (fac * data.take(i)).sum(-1) / fac.sum(-1): float32 data promoted, the sums in neighbour order; a NaN neighbour gives NaN
__host__ __device__ __forceinline__ double sc_value(const float *__restrict__ data, const ScW &W) {
  if (W.a0 < 0) return NAN;
  const double t0 = __dmul_rn(W.f0, (double)data[W.a0]), t1 = __dmul_rn(W.f1, (double)data[W.a1]), t2 = __dmul_rn(W.f2, (double)data[W.a2]);
  return sc_div(__dadd_rn(__dadd_rn(t0, t1), t2), W.fs);
}

// env_before * (1 - weight_after) + env_after * weight_after (:628-630)
__host__ __device__ __forceinline__ double sc_blend(double before, double after, double w) {
  return __dadd_rn(__dmul_rn(before, __dsub_rn(1.0, w)), __dmul_rn(after, w));
}

// rotate_vectors :104-107 on the components as the reference holds them there: a blended value has been stored as float32 by then
// (a masked array, __check_variable_array__, variables.py:637-639), the value of a single level is still float64.  For float32
// components this is um_rotate.
__host__ __device__ __forceinline__ void sc_rotate(double &u, double &v, double cs, double sn) {
  const double uu = u, vv = v;
  u = __dsub_rn(__dmul_rn(uu, cs), __dmul_rn(vv, sn));
  v = __dadd_rn(__dmul_rn(uu, sn), __dmul_rn(vv, cs));
}

// Coverage: inside the convex hull of the nodes -- the shape unit's predicate over the hull's ring (its grid G)
__host__ __device__ __forceinline__ bool sc_covers(const ShGrid &G, double x, double y) {
  return sh_covers(G, x, y) && sh_contains(G, x, y) != 0;
}

// The index the reference's 3-D tree gives point (node, k): its position in the flattened [node][L] array with the masked
// entries removed (:415, :434-436).  off[node]: finite levels in front of the node.
__host__ __device__ __forceinline__ long long sc_ref_index(const float *zcor, const long long *off, int L, int node, int k) {
  const float *col = zcor + (long long)node * L;
  long long at = off[node];
  for (int j = 0; j < k; ++j) at += col[j] == col[j] ? 1 : 0;
  return at;
}

// off [n + 1] of sc_ref_index; returns the number of points of the cloud
inline long long sc_offsets(int n, int L, const float *zcor, long long *off) {
  long long at = 0;
  for (int i = 0; i < n; ++i) {
    off[i] = at;
    for (int k = 0; k < L; ++k) at += zcor[(long long)i * L + k] == zcor[(long long)i * L + k] ? 1 : 0;
  }
  off[n] = at;
  return at;
}

// the search of one query and what the bare entry point reports: idx (the reference's numbering) and the distances
__host__ __device__ __forceinline__ int sc_nearest3(const UmIndex &T, const float *zcor, const long long *off, int L, double qx, double qy, double qz,
                                                    long long *idx, double *dist) {
  Sc3 B;
  const int seen = zcor ? sc_search<true>(T, zcor, L, qx, qy, qz, B) : sc_search<false>(T, nullptr, 0, qx, qy, 0.0, B);
  idx[0] = B.i0 < 0 ? -1 : zcor ? sc_ref_index(zcor, off, L, B.i0, B.k0) : B.i0;
  idx[1] = B.i1 < 0 ? -1 : zcor ? sc_ref_index(zcor, off, L, B.i1, B.k1) : B.i1;
  idx[2] = B.i2 < 0 ? -1 : zcor ? sc_ref_index(zcor, off, L, B.i2, B.k2) : B.i2;
  dist[0] = sc_sqrt(B.d0);
  dist[1] = sc_sqrt(B.d1);
  dist[2] = sc_sqrt(B.d2);
  return seen;
}

#ifndef ODR_SCHISM_HOST
struct ScMesh {
  UmIndex node;
  ShGrid hull;      // the convex hull of the nodes: one ring behind the shape unit's grid (lon_mode as UmMesh's)
  int n_levels, pad;
};
// b / a: the variable's plane of the time level before / after ([node], or [node][L] when levels != 0); a is read only when the
// launch blends.  pair: this variable is the x component and the next one of the launch its y component.
struct ScVar { const float *b, *a; float *out; int levels, first, pair, pad; };
struct ScLaunch {
  int nvars, need2, need3, blend;      // blend 0: the values of the level `before` alone
  double w;                            // weight_after
  const float *zb, *za;                // zcor of the two levels
  ScVar v[UMESH_MAXV];
};

__global__ __launch_bounds__(BLOCK) void k_schism_nearest3(UmIndex T, const float *__restrict__ zcor, const long long *__restrict__ off, int L,
                                                           long long n, const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, long long *__restrict__ idx, double *__restrict__ dist,
                                                           int *__restrict__ visits) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  long long a[3];
  double d[3];
  const int seen = sc_nearest3(T, zcor, off, L, x[i], y[i], zcor ? z[i] : 0.0, a, d);
  idx[3 * i] = a[0]; idx[3 * i + 1] = a[1]; idx[3 * i + 2] = a[2];
  dist[3 * i] = d[0]; dist[3 * i + 1] = d[1]; dist[3 * i + 2] = d[2];
  if (visits) visits[i] = seen;
}

// One element per lane: position -> mesh coordinates -> hull test -> one 2-D search if a 2-D variable is asked, one 3-D search
// per time level if a 3-D variable is asked -> per variable the weighted mean at either level and the blend -> rotation of vector
// pairs -> merge into the environment slot.
__global__ __launch_bounds__(BLOCK) void k_schism_sample(DevProj P, ScMesh M, ScLaunch L, long long n, const double *__restrict__ lon,
                                                         const double *__restrict__ lat, const double *__restrict__ zs) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double x, y;
  if (P.kind == PROJ_LATLONG) {      // get_variables_interpolated: modulate_longitude, then lonlat2xy is the identity
    x = lon[i];
    y = lat[i];
    if (M.hull.lon_mode == 1) x = np_mod(x + 180.0, 360.0) - 180.0;
    else if (M.hull.lon_mode == 2) x = np_mod(x, 360.0);
  } else proj_fwd(P, lon[i], lat[i], x, y);
  if (!sc_covers(M.hull, x, y)) return;      // keeps what it has
  const double z = zs[i];
  ScW W2, W3b, W3a;
  Sc3 B;
  sc_none(W2);
  sc_none(W3b);
  sc_none(W3a);
  if (L.need2) {
    sc_search<false>(M.node, nullptr, 0, x, y, 0.0, B);
    sc_weights(B, 0, W2);
  }
  if (L.need3) {
    sc_search<true>(M.node, L.zb, M.n_levels, x, y, z, B);
    sc_weights(B, M.n_levels, W3b);
    if (L.blend) {      // the cloud of the other level is another cloud: zcor moves with the surface
      sc_search<true>(M.node, L.za, M.n_levels, x, y, z, B);
      sc_weights(B, M.n_levels, W3a);
    }
  }
  double val[UMESH_MAXV];
#pragma unroll
  for (int k = 0; k < UMESH_MAXV; ++k) {
    val[k] = NAN;
    if (k >= L.nvars) continue;
    const ScVar &V = L.v[k];
    double v = sc_value(V.b, V.levels ? W3b : W2);
    if (L.blend) v = (double)(float)sc_blend(v, sc_value(V.a, V.levels ? W3a : W2), L.w);
    val[k] = v;
  }
  bool rotates = false;
#pragma unroll
  for (int k = 0; k + 1 < UMESH_MAXV; ++k) rotates |= k + 1 < L.nvars && L.v[k].pair;
  if (rotates && P.kind != PROJ_LATLONG) {      // (a geographic mesh is not rotated, variables.py:800-802)
    double cs, sn;
    rotation_cs(P, x, y, cs, sn);
#pragma unroll
    for (int k = 0; k + 1 < UMESH_MAXV; ++k)
      if (k + 1 < L.nvars && L.v[k].pair) sc_rotate(val[k], val[k + 1], cs, sn);
  }
#pragma unroll
  for (int k = 0; k < UMESH_MAXV; ++k)
    if (k < L.nvars) L.v[k].out[i] = um_merge((float)val[k], L.v[k].out[i], L.v[k].first);
}
#endif  // ODR_SCHISM_HOST

}  // namespace odr
