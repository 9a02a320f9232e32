// Projected density maps and radionuclide concentration maps of a finished run.
//
//   get_density_array_proj           models/basemodel/__init__.py:4148-4245   conc_moved, k_conc_bin<CONC_MASKS / CONC_MASKS_W>
//   get_radionuclide_density_array   models/radionuclides.py:1425-1492        conc_layer, conc_species_class, k_conc_bin<CONC_SPECIES>
//   horizontal_smooth                models/radionuclides.py:1518-1551        conc_box_sum, k_conc_box
//   +proj=moll (PROJ's moll: the sphere of radius a)                          conc_moll_fwd, conc_moll_inv
//
// get_density_array_proj takes an entry out of a map by MOVING it to (outsidex, outsidey) = 1.5 * (max(x_array), max(y_array))
// (:4186, :4207-4220): from H when z < 0, from H_submerged when z >= 0, from H_stranded when status != the 'stranded' number -- so a
// NaN z stays in H and H_submerged, a NaN status is moved, and a moved entry counts in the bin of that point WHEN THE POINT IS INSIDE
// THE GRID (both maxima negative), whatever its own position was (NaN included).  The host finds that one bin (or that there is
// none); the kernel adds the moved entries of every output time to it.
//
// get_radionuclide_density_array moves nothing: an entry counts in [time, sp, zi] iff specie == sp and z_array[zi] < z <=
// z_array[zi + 1], compared in float64; a NaN z or specie matches nothing.
//
// Bin: np.histogram2d's on the edge arrays themselves, density_bin of odr_density.hip.h.
//
// Compiled for the CPU by tests/conc_host.cpp (ODR_CONC_HOST): everything above the kernels is plain C++.
#pragma once
#include "odr_density.hip.h"

namespace odr {

constexpr int PROJ_MOLL = 11;      // ODR_PROJ_MOLL (include/odrift.h): only the entry points of odr_conc.hip take it

enum { CONC_MOVED_SURFACE = 1, CONC_MOVED_SUBMERGED = 2, CONC_MOVED_STRANDED = 4 };

// the maps an entry is MOVED out of (stranded_code < 0: no such category, bit 2 stays clear)
__host__ __device__ __forceinline__ int conc_moved(float z, float status, int stranded_code) {
  int m = 0;
  if (z < 0.f) m |= CONC_MOVED_SURFACE;
  if (z >= 0.f) m |= CONC_MOVED_SUBMERGED;
  if (stranded_code >= 0 && status != (float)stranded_code) m |= CONC_MOVED_STRANDED;
  return m;
}

// layer zi in 0 .. nb - 2 with zb[zi] < z <= zb[zi + 1], or -1 (NaN, outside).  zb: nb strictly increasing finite bounds
__host__ __device__ __forceinline__ int conc_layer(double z, const double *zb, int nb) {
  if (!(z > zb[0] && z <= zb[nb - 1])) return -1;
  int lo = 0, hi = nb - 1;      // invariant: zb[lo] < z <= zb[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (zb[mid] < z) lo = mid; else hi = mid;
  }
  return lo;
}

// species * n_layers + layer of an entry, or -1: specie == sp for an sp in 0 .. n_species - 1 (-0.0 is species 0)
__host__ __device__ __forceinline__ int conc_species_class(float specie, float z, int n_species, const double *zb, int nb) {
  if (!(specie >= 0.f && specie < (float)n_species)) return -1;
  const int sp = (int)specie;
  if ((float)sp != specie) return -1;
  const int zi = conc_layer((double)z, zb, nb);
  return zi < 0 ? -1 : sp * (nb - 1) + zi;
}

// ---- Mollweide on the sphere of radius a (Snyder 31-1 .. 31-8): x = (2 sqrt 2 / pi) a lam cos th, y = sqrt 2 a sin th with
// 2 th + sin 2 th = pi sin phi.  Solved for eps = pi - 2 |th|, eps - sin eps = pi (1 - sin |phi|) = 2 pi sin^2((pi/2 - |phi|) / 2): the
// right-hand side is formed from the colatitude without cancellation and the derivative 1 - cos eps vanishes at the pole only, where
// eps = 0 is returned at once.  Near the equator (|sin phi| < 1/2) Newton runs on t = 2 th itself, t + sin t = pi sin phi, so that
// th does not come out of a difference.
constexpr double kConcPi = 3.14159265358979323846264338327950288;
constexpr double kConcDeg = kConcPi / 180.0;
constexpr double kConcSqrt2 = 1.41421356237309504880168872420969808;

// eps - sin eps without cancellation at small eps
__host__ __device__ __forceinline__ double conc_eps_minus_sin(double e) {
  if (e < 0.25) {
    const double q = e * e;      // the next term is below 2^-53 of the first
    return e * q * (1.0 / 6 - q * (1.0 / 120 - q * (1.0 / 5040 - q * (1.0 / 362880 - q * (1.0 / 39916800 - q * (1.0 / 6227020800.0))))));
  }
  return e - ::sin(e);
}

// sin th, cos th of the auxiliary angle of latitude lat_deg (NaN: NaN)
__host__ __device__ __forceinline__ void conc_moll_theta(double lat_deg, double &sin_th, double &cos_th) {
  const double alat = ::fabs(lat_deg);
  if (!(alat <= 90.0)) { sin_th = cos_th = __builtin_nan(""); return; }      // NaN, and what PROJ refuses
  double th;
  if (alat < 30.0) {
    const double k = kConcPi * ::sin(alat * kConcDeg);
    double t = 0.5 * k;
    for (int it = 0; it < 12; ++it) {
      const double d = (t + ::sin(t) - k) / (1.0 + ::cos(t));
      t -= d;
      if (::fabs(d) <= 1e-16) break;
    }
    th = 0.5 * t;
    sin_th = ::sin(th); cos_th = ::cos(th);
  } else {
    const double sh = ::sin(0.5 * (90.0 - alat) * kConcDeg);
    const double c = 2.0 * kConcPi * sh * sh;
    double e = ::cbrt(6.0 * c);
    if (c > 0.0) {
      for (int it = 0; it < 12; ++it) {
        const double se = ::sin(0.5 * e);
        const double d = (conc_eps_minus_sin(e) - c) / (2.0 * se * se);
        e -= d;
        if (::fabs(d) <= 1e-16 * e) break;
      }
    }
    sin_th = ::cos(0.5 * e); cos_th = ::sin(0.5 * e);      // th = pi/2 - eps/2
  }
  if (lat_deg < 0) sin_th = -sin_th;
}

// lam: longitude from the central meridian, wrapped to [-pi, pi], radians.  X, Y in units of a
__host__ __device__ __forceinline__ void conc_moll_fwd_unit(double lam, double lat_deg, double &X, double &Y) {
  double s, c;
  conc_moll_theta(lat_deg, s, c);
  X = (2.0 * kConcSqrt2 / kConcPi) * lam * c;
  Y = kConcSqrt2 * s;
}

__host__ __device__ __forceinline__ double conc_wrap_pi(double lam) {
  if (::fabs(lam) <= kConcPi + 1e-12) return lam;      // (as wrap_pi of odr_field.hip.h)
  lam += kConcPi;
  lam -= 2 * kConcPi * ::floor(lam / (2 * kConcPi));
  lam -= kConcPi;
  return lam;
}

__host__ __device__ __forceinline__ void conc_moll_fwd(double a, double lon0_rad, double x0, double y0, double lon_deg, double lat_deg,
                                                       double &x, double &y) {
  double X, Y;
  conc_moll_fwd_unit(conc_wrap_pi(lon_deg * kConcDeg - lon0_rad), lat_deg, X, Y);
  x = a * X + x0;
  y = a * Y + y0;
}

// Closed form.  Outside the ellipse (|Y| > sqrt 2, or a longitude beyond +-180 degrees from the central meridian): NaN.
// sin th = Y / sqrt 2; eps = pi - 2 |th| from atan2 of (cos th, |sin th|); 1 - sin |phi| = (eps - sin eps) / pi gives the colatitude
// by an arc sine of its half, so that no latitude comes from an arc sine near 1.  y itself fixes eps only to sqrt(rounding) next to
// a pole (y is stationary there): that is the map's, not the formula's.
__host__ __device__ __forceinline__ void conc_moll_inv(double a, double lon0_rad, double x0, double y0, double x, double y,
                                                       double &lon_deg, double &lat_deg) {
  const double X = (x - x0) / a, Y = (y - y0) / a / kConcSqrt2;
  const double aY = ::fabs(Y);
  if (!(aY <= 1.0 + 1e-12)) { lon_deg = lat_deg = __builtin_nan(""); return; }
  const double sy = aY < 1.0 ? aY : 1.0;
  const double cos_th = ::sqrt((1.0 - sy) * (1.0 + sy));
  const double eps = 2.0 * ::atan2(cos_th, sy);
  const double c = conc_eps_minus_sin(eps);
  const double sh = ::sqrt(c / (2.0 * kConcPi));
  const double colat = 2.0 * ::asin(sh < 1.0 ? sh : 1.0);
  lat_deg = 90.0 - colat / kConcDeg;
  if (Y < 0) lat_deg = -lat_deg;
  double lam = 0.0;
  if (cos_th > 0.0) lam = kConcPi * X / (2.0 * kConcSqrt2 * cos_th);
  else if (X != 0.0) lam = __builtin_nan("");
  if (!(::fabs(lam) <= kConcPi * (1.0 + 1e-12))) { lon_deg = lat_deg = __builtin_nan(""); return; }
  if (::fabs(lam) > kConcPi) lam = lam < 0 ? -kConcPi : kConcPi;
  lon_deg = conc_wrap_pi(lam + lon0_rad) / kConcDeg;
}

// ---- horizontal_smooth: the integer sum of a window of 2 n + 1 values of a row of `len` values `stride` apart, centred on k, the
// part of the window outside the row counting as zero (the reference pads with n zeros)
template <typename T>
__host__ __device__ __forceinline__ long long conc_box_sum(const T *row, long long len, long long stride, long long k, long long n) {
  const long long lo = k - n < 0 ? 0 : k - n, hi = k + n > len - 1 ? len - 1 : k + n;
  long long s = 0;
  for (long long j = lo; j <= hi; ++j) s += (long long)row[j * stride];
  return s;
}

#ifndef ODR_CONC_HOST
enum { CONC_MASKS = 0, CONC_MASKS_W = 1, CONC_SPECIES = 2 };
constexpr int CONC_MAX_BOUNDS = 256;      // z_array values of odr_species_layer_map (they sit in LDS behind the edges)

struct ConcArgs {
  const float *lon, *lat, *z, *aux, *weight;      // [trajectory][time] of the slab; aux: status (masks) or specie
  const double *x_edges, *y_edges, *z_bounds;     // device copies
  DensityAxis ax, ay;
  long long n;                                    // entries of the slab: trajectories * n_times
  size_t cells;                                   // of one map (masks): n_times * plane
  int n_times, stranded_code, outside_bin;        // outside_bin: the bin of (outsidex, outsidey) inside a plane, or -1
  int n_species, n_bounds;
};

// (x, y) = density_proj(lon, lat) in float64 from the float32 result arrays
__device__ __forceinline__ void conc_project(const DevProj &P, float lon, float lat, double &x, double &y) {
  if (P.kind == PROJ_MOLL) conc_moll_fwd(P.a, P.lon0, P.x0, P.y0, (double)lon, (double)lat, x, y);
  else proj_fwd<false, true>(P, (double)lon, (double)lat, x, y);
}

// One entry per lane in the [trajectory][time] order of k_density (odr_density.hip.h), with its lane combining: lanes a multiple of
// n_times apart hold the same output time, the lowest of those with the same destination adds the count of all of them.
//   CONC_MASKS    H: unsigned [3][time][x_bin][y_bin].  An entry adds to its own bin in the maps it stays in and to outside_bin in
//                 the maps it is moved out of (a second combining pass, run only when there is such a bin).
//   CONC_MASKS_W  H: double, same layout; every lane adds its own weight to its own bin; the weights moved to outside_bin are summed
//                 over the combined lanes first (a NaN weight makes that bin NaN, as np.histogram2d does).
//   CONC_SPECIES  H: unsigned [time][species][layer][x_bin][y_bin]; classes * plane <= 2^28 (odr_species_layer_map).
// Dynamic LDS: the edge arrays when LDS_EDGES (at most DENSITY_LDS_EDGES values), then the z bounds (CONC_SPECIES).
template <int MODE, bool LDS_EDGES, typename T>
__global__ __launch_bounds__(BLOCK) void k_conc_bin(ConcArgs A, DevProj P, T *__restrict__ H) {
  extern __shared__ double s_conc[];
  const double *ex = A.x_edges, *ey = A.y_edges;
  const int n_lds_edges = LDS_EDGES ? A.ax.n + A.ay.n : 0;
  if (LDS_EDGES) {
    for (int k = threadIdx.x; k < A.ax.n; k += BLOCK) s_conc[k] = A.x_edges[k];
    for (int k = threadIdx.x; k < A.ay.n; k += BLOCK) s_conc[A.ax.n + k] = A.y_edges[k];
    ex = s_conc; ey = s_conc + A.ax.n;
  }
  if (MODE == CONC_SPECIES)
    for (int k = threadIdx.x; k < A.n_bounds; k += BLOCK) s_conc[n_lds_edges + k] = A.z_bounds[k];
  if (LDS_EDGES || MODE == CONC_SPECIES) __syncthreads();
  const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned ny = (unsigned)(A.ay.n - 1), plane = (unsigned)(A.ax.n - 1) * ny;
  unsigned key = 0, okey = 0;      // masks: bin << 3 | maps; species: class * plane + bin + 1; 0: the entry counts nowhere
  int t = 0;
  if (e < A.n) {
    double x, y;
    conc_project(P, A.lon[e], A.lat[e], x, y);
    const int ix = density_bin(x, A.ax, ex);
    const int iy = ix >= 0 ? density_bin(y, A.ay, ey) : -1;
    const unsigned own = (unsigned)ix * ny + (unsigned)iy;
    if constexpr (MODE == CONC_SPECIES) {
      if (iy >= 0) {
        const int cls = conc_species_class(A.aux[e], A.z[e], A.n_species, s_conc + n_lds_edges, A.n_bounds);
        if (cls >= 0) key = (unsigned)cls * plane + own + 1u;
      }
    } else {
      const int valid = A.stranded_code >= 0 ? 7 : 3;
      const int moved = conc_moved(A.z[e], A.aux[e], A.stranded_code);
      if (iy >= 0 && (valid & ~moved)) key = own << 3 | (unsigned)(valid & ~moved);
      if (A.outside_bin >= 0 && moved) okey = (unsigned)A.outside_bin << 3 | (unsigned)moved;
    }
    t = (int)((unsigned)e % (unsigned)A.n_times);      // a slab has fewer than 2^31 entries
  }
  const int lane = (int)__lane_id();
  if constexpr (MODE == CONC_SPECIES) {
    unsigned c = key != 0;
    bool lead = key != 0;
    for (int s = A.n_times; s < 64; s += A.n_times) {      // wave-uniform
      const unsigned up = __shfl(key, (lane + s) & 63), down = __shfl(key, (lane - s) & 63);
      if (lane + s < 64 && up == key) ++c;
      if (lane - s >= 0 && down == key) lead = false;
    }
    if (lead) atomicAdd(&H[(size_t)t * ((size_t)A.n_species * (size_t)(A.n_bounds - 1) * plane) + (key - 1u)], c);
  } else {
    const size_t dst = (size_t)t * plane + (key >> 3), odst = (size_t)t * plane + (okey >> 3);
    if constexpr (MODE == CONC_MASKS_W) {
      const double w = (key | okey) ? (double)A.weight[e] : 0.0;
      if (key & 1) unsafeAtomicAdd(&H[dst], w);
      if (key & 2) unsafeAtomicAdd(&H[A.cells + dst], w);
      if (key & 4) unsafeAtomicAdd(&H[2 * A.cells + dst], w);
      if (A.outside_bin >= 0) {      // kernel-uniform
        const double mine = okey ? w : 0.0;      // (the lanes hand out their own weight, never a partial sum)
        double w0 = okey & 1 ? w : 0.0, w1 = okey & 2 ? w : 0.0, w2 = okey & 4 ? w : 0.0;
        unsigned m = okey & 7;
        bool lead = okey != 0;
        for (int s = A.n_times; s < 64; s += A.n_times) {
          const unsigned up = __shfl(okey, (lane + s) & 63), down = __shfl(okey, (lane - s) & 63);
          const double u = __shfl(mine, (lane + s) & 63);
          if (lane + s < 64 && up != 0) {      // (the sums take the lanes above in the order of the loop: lane + s, + 2 s ...)
            if (up & 1) w0 += u;
            if (up & 2) w1 += u;
            if (up & 4) w2 += u;
            m |= up & 7;
          }
          if (lane - s >= 0 && down != 0) lead = false;
        }
        if (lead) {
          if (m & 1) unsafeAtomicAdd(&H[odst], w0);
          if (m & 2) unsafeAtomicAdd(&H[A.cells + odst], w1);
          if (m & 4) unsafeAtomicAdd(&H[2 * A.cells + odst], w2);
        }
      }
    } else {
      unsigned c0 = key & 1, c1 = (key >> 1) & 1, c2 = (key >> 2) & 1;
      bool lead = key != 0;
      for (int s = A.n_times; s < 64; s += A.n_times) {      // wave-uniform; lanes s apart hold the same output time
        const unsigned up = __shfl(key, (lane + s) & 63), down = __shfl(key, (lane - s) & 63);
        if (lane + s < 64 && (up >> 3) == (key >> 3)) { c0 += up & 1; c1 += (up >> 1) & 1; c2 += (up >> 2) & 1; }
        if (lane - s >= 0 && down != 0 && (down >> 3) == (key >> 3)) lead = false;
      }
      if (lead) {
        if (c0) atomicAdd(&H[dst], c0);
        if (c1) atomicAdd(&H[A.cells + dst], c1);
        if (c2) atomicAdd(&H[2 * A.cells + dst], c2);
      }
      if (A.outside_bin >= 0) {      // kernel-uniform: every moved entry of an output time has the same destination
        unsigned o0 = okey & 1, o1 = (okey >> 1) & 1, o2 = (okey >> 2) & 1;
        bool olead = okey != 0;
        for (int s = A.n_times; s < 64; s += A.n_times) {
          const unsigned up = __shfl(okey, (lane + s) & 63), down = __shfl(okey, (lane - s) & 63);
          if (lane + s < 64) { o0 += up & 1; o1 += (up >> 1) & 1; o2 += (up >> 2) & 1; }
          if (lane - s >= 0 && down != 0) olead = false;
        }
        if (olead) {
          if (o0) atomicAdd(&H[odst], o0);
          if (o1) atomicAdd(&H[A.cells + odst], o1);
          if (o2) atomicAdd(&H[2 * A.cells + odst], o2);
        }
      }
    }
  }
}

// Extremes of the finite projected positions: out[block] = (min x, max x, min y, max y) of the entries the workgroup took
// (+inf / -inf where it had none); a position counts when both of its coordinates are finite.  Grid-stride; wave reduction by
// shuffles, the waves of a workgroup combined through dynamic LDS (4 doubles per wave).  No atomics: the host finishes.
__global__ __launch_bounds__(BLOCK) void k_conc_extent(DevProj P, const float *__restrict__ lon, const float *__restrict__ lat, long long n,
                                                       double *__restrict__ out) {
  extern __shared__ double s_ext[];
  double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < n; e += (long long)gridDim.x * BLOCK) {
    double x, y;
    conc_project(P, lon[e], lat[e], x, y);
    if (isfinite(x) && isfinite(y)) { v[0] = fmin(v[0], x); v[1] = fmax(v[1], x); v[2] = fmin(v[2], y); v[3] = fmax(v[3], y); }
  }
  for (int s = 32; s > 0; s >>= 1) {
    v[0] = fmin(v[0], __shfl_xor(v[0], s)); v[1] = fmax(v[1], __shfl_xor(v[1], s));
    v[2] = fmin(v[2], __shfl_xor(v[2], s)); v[3] = fmax(v[3], __shfl_xor(v[3], s));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_ext[4 * wave] = v[0]; s_ext[4 * wave + 1] = v[1]; s_ext[4 * wave + 2] = v[2]; s_ext[4 * wave + 3] = v[3]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / 64; ++w) {
      v[0] = fmin(v[0], s_ext[4 * w]); v[1] = fmax(v[1], s_ext[4 * w + 1]);
      v[2] = fmin(v[2], s_ext[4 * w + 2]); v[3] = fmax(v[3], s_ext[4 * w + 3]);
    }
    out[4 * (size_t)blockIdx.x] = v[0]; out[4 * (size_t)blockIdx.x + 1] = v[1];
    out[4 * (size_t)blockIdx.x + 2] = v[2]; out[4 * (size_t)blockIdx.x + 3] = v[3];
  }
}

// density_proj(X, Y, inverse=True) of np.meshgrid(y_array, x_array): point k0 + k of the grid is (x[i], y[j]), i = (k0 + k) / ny
__global__ __launch_bounds__(BLOCK) void k_conc_grid(DevProj P, const double *__restrict__ xs, const double *__restrict__ ys, int ny,
                                                     long long k0, long long count, double *__restrict__ lon, double *__restrict__ lat) {
  const long long k = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  const long long i = (k0 + k) / ny;
  const int j = (int)((k0 + k) - i * ny);
  double lo, la;
  if (P.kind == PROJ_MOLL) conc_moll_inv(P.a, P.lon0, P.x0, P.y0, xs[i], ys[j], lo, la);
  else proj_inv<true>(P, xs[i], ys[j], lo, la);
  lon[k] = lo; lat[k] = la;
}

// horizontal_smooth in two passes over planes [n0][n1]: ROWS: tmp = the window sum along the last axis of (long long)in;
// then along the first axis of tmp, divided by (2 n + 1)^2 in float64.  The sums are of integers: no order of summation shows.
template <bool ROWS, typename TIN, typename TOUT>
__global__ __launch_bounds__(BLOCK) void k_conc_box(const TIN *__restrict__ in, TOUT *__restrict__ out, long long cells, long long n0,
                                                    long long n1, long long n, double divisor) {
  const long long k = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= cells) return;
  const long long j = k % n1, i = (k / n1) % n0;
  if constexpr (ROWS) out[k] = (TOUT)conc_box_sum(in + (k - j), n1, 1, j, n);
  else out[k] = (TOUT)((double)conc_box_sum(in + (k - i * n1), n0, n1, i, n) / divisor);
}
#endif  // ODR_CONC_HOST

}  // namespace odr
