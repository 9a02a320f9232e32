// Density maps: the three 2-D histograms per output time of OpenDriftSimulation.get_density_array.
//
//   get_density_array    models/basemodel/__init__.py:4091-4146    density_classes, density_bin, k_density
//   np.histogram2d       (numpy/lib/_histograms_impl.py, histogramdd)  density_bin
//
// Classes (:4114-4117, :4123-4125), literally from the masks -- an entry is REMOVED from a histogram by overwriting its position
// with 1000, so whatever a comparison with NaN leaves in stays in:
//   H            unless z < 0        (z = -0.0 and a NaN z count)
//   H_submerged  unless z >= 0       (a NaN z counts here too)
//   H_stranded   when status == the number of the 'stranded' category (a NaN status never is)
//
// Bin: np.histogram2d widens the float32 lon / lat to float64 and takes searchsorted(edges, v, side='right') - 1 on the edge array
// itself, with a value EQUAL to the last edge moved into the last bin; NaN and everything outside [edges[0], edges[n - 1]] is
// dropped.  density_bin gives exactly that index for ANY strictly increasing edge array: a first guess from the mean bin width, kept
// when edges[g] <= v < edges[g + 1] holds on the actual edges, else a binary search on them.  np.arange edges (start + i * step in
// float64) are not equidistant to the last bit, so the guess alone would misplace values next to an edge.
//
// Compiled for the CPU by tests/density_host.cpp: everything above the kernels is plain C++.
#pragma once

namespace odr {

enum { DENSITY_SURFACE = 1, DENSITY_SUBMERGED = 2, DENSITY_STRANDED = 4 };

// the histograms an entry counts in, as far as z and status decide (stranded_code < 0: no such category)
__host__ __device__ __forceinline__ int density_classes(float z, float status, int stranded_code) {
  int c = 0;
  if (!(z < 0.f)) c |= DENSITY_SURFACE;
  if (!(z >= 0.f)) c |= DENSITY_SUBMERGED;
  if (stranded_code >= 0 && status == (float)stranded_code) c |= DENSITY_STRANDED;
  return c;
}

// What the guess needs: edges[0], edges[n - 1] and (n - 1) / (edges[n - 1] - edges[0])
struct DensityAxis {
  double first, last, inv_width;
  int n;      // edges, >= 2
};

__host__ __device__ __forceinline__ DensityAxis density_axis(const double *edges, int n) {
  DensityAxis a;
  a.first = edges[0]; a.last = edges[n - 1]; a.n = n;
  a.inv_width = (double)(n - 1) / (edges[n - 1] - edges[0]);
  return a;
}

// bin of v in 0 .. n - 2, or -1 (NaN, outside).  edges: n strictly increasing finite values
__host__ __device__ __forceinline__ int density_bin(double v, const DensityAxis &a, const double *edges) {
  if (!(v >= a.first && v <= a.last)) return -1;
  const int top = a.n - 2;
  const double f = (v - a.first) * a.inv_width;      // 0 .. n - 1 and a rounding
  int g = f < (double)top ? (int)f : top;
  if (edges[g] <= v && (g == top || v < edges[g + 1])) return g;
  int lo = 0, hi = a.n - 1;      // invariant: edges[lo] <= v, and v < edges[hi] or hi == n - 1
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

#ifndef ODR_DENSITY_HOST
constexpr int DENSITY_LDS_EDGES = 4096;      // both edge arrays together, 32 KB of float64: above that they are read from memory

struct DensityArgs {
  const float *lon, *lat, *z, *status, *weight;      // [trajectory][time] of the slab
  const double *lon_edges, *lat_edges;               // device copies
  DensityAxis ax_lon, ax_lat;
  long long n;                                       // entries of the slab: trajectories * n_times
  int n_times, stranded_code;
};

// One entry per lane: entry e = trajectory * n_times + time of the slab, so a wave reads 256 contiguous bytes of each array and no
// transposition is needed.  The lanes of a wave then hold different output times of a few trajectories -- different planes of the
// histograms -- so that even a plume that falls into one bin spreads a wave's adds over min(64, n_times) addresses.  Lanes that can
// still share a destination are those a multiple of n_times apart (n_times < 64): they are combined, the lowest of them adds the
// count of all of them with ONE atomic per histogram.  WEIGHTED: every lane adds its own weight (float64 atomic).
// H*: [time][lon_bin][lat_bin]; a plane has at most 2^28 bins (odr_density_map).
template <bool WEIGHTED, bool LDS_EDGES, typename T>
__global__ __launch_bounds__(BLOCK) void k_density(DensityArgs A, T *__restrict__ H, T *__restrict__ Hsub, T *__restrict__ Hstr) {
  extern __shared__ double s_edges[];
  const double *elon = A.lon_edges, *elat = A.lat_edges;
  if (LDS_EDGES) {
    for (int k = threadIdx.x; k < A.ax_lon.n; k += BLOCK) s_edges[k] = A.lon_edges[k];
    for (int k = threadIdx.x; k < A.ax_lat.n; k += BLOCK) s_edges[A.ax_lon.n + k] = A.lat_edges[k];
    __syncthreads();
    elon = s_edges; elat = s_edges + A.ax_lon.n;
  }
  const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned nlat = (unsigned)(A.ax_lat.n - 1), plane = (unsigned)(A.ax_lon.n - 1) * nlat;
  unsigned key = 0;      // bin inside the plane << 3 | classes; 0: the entry counts nowhere
  int t = 0;
  if (e < A.n) {
    const int ilon = density_bin((double)A.lon[e], A.ax_lon, elon);
    const int ilat = ilon >= 0 ? density_bin((double)A.lat[e], A.ax_lat, elat) : -1;
    if (ilat >= 0) {
      const int cls = density_classes(A.z[e], A.status[e], A.stranded_code);
      if (cls) key = ((unsigned)ilon * nlat + (unsigned)ilat) << 3 | (unsigned)cls;
      t = (int)((unsigned)e % (unsigned)A.n_times);      // a slab has fewer than 2^31 entries
    }
  }
  const size_t dst = (size_t)t * plane + (key >> 3);
  if constexpr (WEIGHTED) {
    if (key) {
      const double w = (double)A.weight[e];
      if (key & DENSITY_SURFACE) unsafeAtomicAdd(&H[dst], w);
      if (key & DENSITY_SUBMERGED) unsafeAtomicAdd(&Hsub[dst], w);
      if (key & DENSITY_STRANDED) unsafeAtomicAdd(&Hstr[dst], w);
    }
  } else {
    unsigned c0 = key & 1, c1 = (key >> 1) & 1, c2 = (key >> 2) & 1;
    bool lead = key != 0;
    const int lane = (int)__lane_id();
    for (int s = A.n_times; s < 64; s += A.n_times) {      // wave-uniform; lanes s apart hold the same output time
      const unsigned up = __shfl(key, (lane + s) & 63), down = __shfl(key, (lane - s) & 63);
      if (lane + s < 64 && (up >> 3) == (key >> 3)) { c0 += up & 1; c1 += (up >> 1) & 1; c2 += (up >> 2) & 1; }
      if (lane - s >= 0 && down != 0 && (down >> 3) == (key >> 3)) lead = false;
    }
    if (lead) {
      if (c0) atomicAdd(&H[dst], c0);
      if (c1) atomicAdd(&Hsub[dst], c1);
      if (c2) atomicAdd(&Hstr[dst], c2);
    }
  }
}
#endif  // ODR_DENSITY_HOST

}  // namespace odr
