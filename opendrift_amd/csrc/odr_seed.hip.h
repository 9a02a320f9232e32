// Seeding geometry on the device: the points of a cone's centre line, and N points evenly placed within a polygon.
//
//   seed_cone / seed_repeated_segment   models/basemodel/__init__.py:1240-1353, :1402-1456   pyproj.Geod.npts: k_npts_line, k_npts_points
//   points_within_polygon               models/basemodel/__init__.py:1487-1558               seed_plan, seed_grid_point, k_seed_*
//   matplotlib.path.Path.contains_points (the crossing rule of its point_in_path)             pip_edge, pip_walk, k_pip_points
//
// points_within_polygon lays a regular grid over the polygon in an equal-area projection and keeps the grid points that
// matplotlib finds inside the ring.  The projection it asks PROJ for names +R=6370997 next to +ellps=WGS84, and R wins: the
// SPHERICAL Albers of Snyder (Map projections: a working manual, 1987, eqs. 14-1 .. 14-11), in the operation order of PROJ.
//
// Rounding points, all float64: the four projection parameters go through '%f' (6 decimals); the shoelace area is summed in the
// reference's loop order; deltax = sqrt(area / number); nx, ny truncate; the grid is numpy.linspace's start + i * step with the
// last element the stop itself; every grid point is inverse-projected and tested in lon / lat against the closed ring.
//
// The device and the host build (tests/seed_host.cpp) give the SAME BITS: everything above the kernels is plain C++ on + - * /
// sqrt and fma, sin / cos / atan2 are the polynomial kernels of odr_geodinv.hip.h, both builds use -ffp-contract=off and each fma is
// written out.  The O(m) set-up (seed_plan) runs on the host in both, so nx and ny are decided once.
#pragma once
#ifndef ODR_GEODINV_HOST
#define ODR_GEODINV_NO_KERNELS 1      // k_geod_inverse and the trajectory kernels belong to odr_geodinv.hip's translation unit
#endif
#include "odr_geodinv.hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace odr {

constexpr double kSeedR = 6370997.0;                  // +R of the reference's projection string
constexpr double kSeedHalfPi = 1.57079632679489661923;
constexpr double kSeedTwoPi = 6.28318530717958647692;

// Spherical Albers equal-area on the unit sphere (PROJ's aea set-up for es = 0), scaled by R at the ends
struct Albers { double n, c, rho0, lam0; };

// 0, or 1 when the cone constant vanishes (standard parallels symmetric about the equator: PROJ refuses those too)
__host__ __device__ __forceinline__ int aea_setup(double lat1, double lat2, double lat0, double lon0, Albers &A) {
  double s1, c1, s2, c2, s0, c0;
  gi_sincos(lat1 * kDeg, s1, c1);
  gi_sincos(lat2 * kDeg, s2, c2);
  gi_sincos(lat0 * kDeg, s0, c0);
  double n = s1;
  if (fabs(lat1 * kDeg - lat2 * kDeg) >= 1e-10) n = 0.5 * (n + s2);
  if (!(fabs(n) >= 1e-10)) return 1;
  A.n = n;
  A.c = c1 * c1 + (n + n) * s1;
  A.rho0 = sqrt(A.c - (n + n) * s0) / n;
  A.lam0 = lon0 * kDeg;
  return 0;
}
__host__ __device__ __forceinline__ void aea_forward(const Albers &A, double lon, double lat, double &x, double &y) {
  double dl = lon * kDeg - A.lam0;
  if (fabs(dl) > kGiPi) dl = dl - kSeedTwoPi * rint(dl / kSeedTwoPi);      // into [-pi, pi]
  double sp, cp, st, ct;
  gi_sincos(lat * kDeg, sp, cp);
  const double rho = sqrt(A.c - (A.n + A.n) * sp) / A.n;
  gi_sincos(dl * A.n, st, ct);
  x = kSeedR * (rho * st);
  y = kSeedR * (A.rho0 - rho * ct);
}
__host__ __device__ __forceinline__ void aea_inverse(const Albers &A, double x, double y, double &lon, double &lat) {
  x = x / kSeedR;
  y = A.rho0 - y / kSeedR;
  double rho = sqrt(x * x + y * y);
  double phi, lam = 0;
  if (rho != 0) {
    if (A.n < 0) { rho = -rho; x = -x; y = -y; }
    const double t = rho * A.n;
    const double v = (A.c - t * t) / (A.n + A.n);
    phi = fabs(v) <= 1 ? gi_atan2(v, sqrt((1 - v) * (1 + v))) : (v < 0 ? -kSeedHalfPi : kSeedHalfPi);
    lam = gi_atan2(x, y) / A.n;
  } else {
    phi = A.n > 0 ? kSeedHalfPi : -kSeedHalfPi;
  }
  lon = (lam + A.lam0) * kRad2Deg;
  lat = phi * kRad2Deg;
}

// One edge (vx0, vy0) -> (vx1, vy1) of matplotlib's crossing rule for the point (tx, ty); yflag0 is (vy0 >= ty).  Returns yflag1.
__host__ __device__ __forceinline__ bool pip_edge(double tx, double ty, double vx0, double vy0, bool yflag0, double vx1, double vy1,
                                                  unsigned &inside) {
  const bool yflag1 = vy1 >= ty;
  if (yflag0 != yflag1 && (((vy1 - ty) * (vx0 - vx1) >= (vx1 - tx) * (vy0 - vy1)) == yflag1)) inside ^= 1U;
  return yflag1;
}

// What seed_plan hands to the kernels: the projection and the two numpy.linspace parameter sets
struct SeedPlan {
  Albers A;
  double x0, xstep, xstop, y0, ystep, ystop;
  int nx, ny;
};

// Grid point idx = j * nx + i (meshgrid ravelled row-major, x fastest), inverse-projected
__host__ __device__ __forceinline__ void seed_grid_point(const SeedPlan &P, long long idx, double &lon, double &lat) {
  const int j = (int)(idx / P.nx), i = (int)(idx - (long long)j * P.nx);
  const double x = (i == P.nx - 1 && P.nx > 1) ? P.xstop : P.x0 + (double)i * P.xstep;
  const double y = (j == P.ny - 1 && P.ny > 1) ? P.ystop : P.y0 + (double)j * P.ystep;
  aea_inverse(P.A, x, y, lon, lat);
}

// ------------------------------------------------------------------ the O(m) set-up, on the host in both builds
enum { SEED_OK = 0, SEED_NO_CONE = 1, SEED_NO_AREA = 2, SEED_TOO_MANY = 3 };

// float('%f' % v): the reference formats the projection parameters with 6 decimals
inline double seed_round6(double v) {
  char buf[400];
  snprintf(buf, sizeof buf, "%f", v);
  return strtod(buf, nullptr);
}

// Closes the ring (rx, ry: the first vertex again unless the last one equals it), sets the projection up from the extremes of
// the caller's vertices, projects the ring, sums the area and lays the grid out.  nx * ny may be 0 (the centre branch).
inline int seed_plan(int m, const double *lons, const double *lats, long long number, SeedPlan &P, std::vector<double> &rx,
                     std::vector<double> &ry) {
  rx.assign(lons, lons + m);
  ry.assign(lats, lats + m);
  if (lons[0] != lons[m - 1] || lats[0] != lats[m - 1]) { rx.push_back(lons[0]); ry.push_back(lats[0]); }
  double lomin = lons[0], lomax = lons[0], lamin = lats[0], lamax = lats[0];
  for (int k = 1; k < m; ++k) {
    lomin = fmin(lomin, lons[k]); lomax = fmax(lomax, lons[k]);
    lamin = fmin(lamin, lats[k]); lamax = fmax(lamax, lats[k]);
  }
  if (aea_setup(seed_round6(lamin), seed_round6(lamax), seed_round6((lamin + lamax) / 2), seed_round6((lomin + lomax) / 2), P.A))
    return SEED_NO_CONE;
  const int mc = (int)rx.size();
  std::vector<double> x(mc), y(mc);
  for (int k = 0; k < mc; ++k) aea_forward(P.A, rx[k], ry[k], x[k], y[k]);
  // for i in range(-1, len(x) - 1): area += x[i] * (y[i + 1] - y[i - 1])
  double area = 0.0;
  for (int i = -1; i < mc - 1; ++i) area += x[(i + mc) % mc] * (y[i + 1] - y[(i - 1 + 2 * mc) % mc]);
  area = fabs(area) / 2;
  if (!(area > 0) || !(area < 1e300)) return SEED_NO_AREA;
  const double deltax = sqrt(area / (double)number);
  double xmin = x[0], xmax = x[0], ymin = y[0], ymax = y[0];
  for (int k = 1; k < mc; ++k) {
    xmin = fmin(xmin, x[k]); xmax = fmax(xmax, x[k]);
    ymin = fmin(ymin, y[k]); ymax = fmax(ymax, y[k]);
  }
  const double fx = (xmax - xmin) / deltax, fy = (ymax - ymin) / deltax;      // int() truncates
  if (!(fx < 2147483648.0) || !(fy < 2147483648.0)) return SEED_TOO_MANY;
  P.nx = (int)fx; P.ny = (int)fy;
  if ((long long)P.nx * P.ny >= (1ll << 31)) return SEED_TOO_MANY;
  // numpy.linspace(start, stop, num): start + i * ((stop - start) / (num - 1)), the last element the stop; num = 1: [start]
  P.x0 = xmin + deltax / 2; P.xstop = xmax - deltax / 2;
  P.y0 = ymin + deltax / 2; P.ystop = ymax - deltax / 2;
  P.xstep = P.nx > 1 ? (P.xstop - P.x0) / (double)(P.nx - 1) : 0.0;
  P.ystep = P.ny > 1 ? (P.ystop - P.y0) / (double)(P.ny - 1) : 0.0;
  return SEED_OK;
}

// Element k of the result is src[k mod L]: the reference's truncate-then-duplicate loop.  out[0 .. min(L, number)) is filled.
inline void seed_cyclic(double *out, long long L, long long number) {
  for (long long k = L; k < number; ++k) out[k] = out[k - L];
}
// The branches that need no grid: the centre (grid empty) and the border (no grid point inside)
inline void seed_centre(int m, const double *lons, const double *lats, long long number, double *out_lon, double *out_lat) {
  double slon = 0, slat = 0;
  for (int k = 0; k < m; ++k) { slon += lons[k]; slat += lats[k]; }
  for (long long k = 0; k < number; ++k) { out_lon[k] = slon / m; out_lat[k] = slat / m; }
}
inline void seed_border(int m, const double *lons, const double *lats, long long number, double *out_lon, double *out_lat) {
  const long long L = number < m ? number : m;
  for (long long k = 0; k < L; ++k) { out_lon[k] = lons[k]; out_lat[k] = lats[k]; }
  seed_cyclic(out_lon, L, number);
  seed_cyclic(out_lat, L, number);
}

#ifndef ODR_SEED_HOST
constexpr int SEED_BLOCK = 256;                       // lanes of a workgroup: four waves
constexpr int SEED_WAVES = SEED_BLOCK / 64;
constexpr int PIP_TILE = 256;                         // ring vertices staged in LDS at a time

// The crossing rule for one point per lane against a ring of m vertices (the edge from the last vertex back to the first
// included).  Tile t holds the END vertices of edges t * PIP_TILE .. : vertices 1 + t * PIP_TILE + s, the index m meaning 0; the
// start vertex of an edge is the one the lane carries from the edge before.  Every lane of the workgroup walks every tile -- also
// a lane that has no point -- so that all of them meet at the barriers.
__device__ __forceinline__ unsigned pip_walk(double tx, double ty, int m, const double *__restrict__ vx, const double *__restrict__ vy,
                                             double *s_x, double *s_y) {
  double x0 = vx[0], y0 = vy[0];
  bool yflag0 = y0 >= ty;
  unsigned inside = 0;
  for (int e0 = 0; e0 < m; e0 += PIP_TILE) {
    __syncthreads();      // the tile before has been read by everyone
    for (int s = threadIdx.x; s < PIP_TILE; s += SEED_BLOCK) {
      const int k = e0 + 1 + s;
      if (k <= m) {
        const int kk = k == m ? 0 : k;
        s_x[s] = vx[kk];
        s_y[s] = vy[kk];
      }
    }
    __syncthreads();
    const int cnt = min(PIP_TILE, m - e0);
    for (int s = 0; s < cnt; ++s) {
      const double x1 = s_x[s], y1 = s_y[s];      // the same address in every lane: a broadcast
      yflag0 = pip_edge(tx, ty, x0, y0, yflag0, x1, y1, inside);
      x0 = x1; y0 = y1;
    }
  }
  return inside;
}

// n points (x, y) against the ring: inside[i] = 1 or 0
__global__ __launch_bounds__(SEED_BLOCK) void k_pip_points(long long n, const double *__restrict__ x, const double *__restrict__ y, int m,
                                                           const double *__restrict__ vx, const double *__restrict__ vy,
                                                           unsigned char *__restrict__ inside) {
  __shared__ double s_x[PIP_TILE], s_y[PIP_TILE];
  const long long i = (long long)blockIdx.x * SEED_BLOCK + threadIdx.x;
  const bool live = i < n;
  const unsigned in = pip_walk(live ? x[i] : 0.0, live ? y[i] : 0.0, m, vx, vy, s_x, s_y);
  if (live) inside[i] = (unsigned char)in;
}

// One lane per grid point of the plan: the point is inverse-projected and tested against the closed ring (mc vertices, lon / lat).
// masks[4 * workgroup + wave]: the wave's ballot of inside points; counts[workgroup]: how many the workgroup has.
__global__ __launch_bounds__(SEED_BLOCK) void k_seed_edges(SeedPlan P, long long n, int mc, const double *__restrict__ vx,
                                                           const double *__restrict__ vy, unsigned long long *__restrict__ masks,
                                                           unsigned *__restrict__ counts) {
  __shared__ double s_x[PIP_TILE], s_y[PIP_TILE];
  __shared__ unsigned s_cnt[SEED_WAVES];
  const long long i = (long long)blockIdx.x * SEED_BLOCK + threadIdx.x;
  const bool live = i < n;
  double lon = 0, lat = 0;
  if (live) seed_grid_point(P, i, lon, lat);
  const unsigned in = pip_walk(lon, lat, mc, vx, vy, s_x, s_y);
  const unsigned long long mask = __ballot(live && in);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    masks[(size_t)blockIdx.x * SEED_WAVES + wave] = mask;
    s_cnt[wave] = (unsigned)__popcll(mask);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0;
    for (int w = 0; w < SEED_WAVES; ++w) c += s_cnt[w];
    counts[blockIdx.x] = c;
  }
}

// offsets[g] = counts[0] + ... + counts[g - 1], offsets[nwg] the total: ONE workgroup walks the counts in tiles of 256 with a
// running carry (launch with a single workgroup of SEED_BLOCK lanes)
__global__ __launch_bounds__(SEED_BLOCK) void k_seed_scan(const unsigned *__restrict__ counts, long long nwg, unsigned *__restrict__ offsets) {
  __shared__ unsigned s[2][SEED_BLOCK];
  unsigned carry = 0;
  for (long long g0 = 0; g0 < nwg; g0 += SEED_BLOCK) {
    const long long g = g0 + threadIdx.x;
    const unsigned mine = g < nwg ? counts[g] : 0U;
    int cur = 0;
    s[0][threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < SEED_BLOCK; d <<= 1) {      // inclusive Hillis-Steele scan, double-buffered
      const unsigned v = s[cur][threadIdx.x] + ((int)threadIdx.x >= d ? s[cur][threadIdx.x - d] : 0U);
      s[cur ^ 1][threadIdx.x] = v;
      cur ^= 1;
      __syncthreads();
    }
    if (g < nwg) offsets[g] = carry + s[cur][threadIdx.x] - mine;
    carry += s[cur][SEED_BLOCK - 1];
    __syncthreads();      // s is written again by the next tile
  }
  if (threadIdx.x == 0) offsets[nwg] = carry;
}

// The inside points in grid order: the rank of a point is its workgroup's offset, the inside points of the waves before its own
// and those of the lower lanes of its wave.  Ranks from `limit` on are cut (the reference's truncation).  No atomics.
__global__ __launch_bounds__(SEED_BLOCK) void k_seed_compact(SeedPlan P, long long n, const unsigned long long *__restrict__ masks,
                                                             const unsigned *__restrict__ offsets, long long limit,
                                                             double *__restrict__ out_lon, double *__restrict__ out_lat) {
  const long long i = (long long)blockIdx.x * SEED_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long *wm = masks + (size_t)blockIdx.x * SEED_WAVES;
  const unsigned long long mask = wm[wave];
  if (!((mask >> lane) & 1ULL)) return;
  long long rank = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) rank += __popcll(wm[w]);
  rank += __popcll(mask & ((1ULL << lane) - 1ULL));
  if (rank >= limit) return;
  double lon, lat;
  seed_grid_point(P, i, lon, lat);
  out_lon[rank] = lon;
  out_lat[rank] = lat;
}

// pyproj.Geod.npts: the line from point 1 to point 2, line[0] = s12 [m], line[1] = azi1 [deg] (one lane of one wave)
__global__ void k_npts_line(double lon1, double lat1, double lon2, double lat2, double *__restrict__ line) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s12, azi1, azi2;
  geod_inverse(lat1, lon1, lat2, lon2, s12, azi1, azi2);
  line[0] = s12;
  line[1] = azi1;
}
// ... and its npts points at i * s12 / (npts + 1), i = 1 .. npts: both ends excluded.  One direct solve per lane.
__global__ __launch_bounds__(SEED_BLOCK) void k_npts_points(double lon1, double lat1, const double *__restrict__ line, long long npts,
                                                     double *__restrict__ out_lon, double *__restrict__ out_lat) {
  const long long i = (long long)blockIdx.x * SEED_BLOCK + threadIdx.x;
  if (i >= npts) return;
  const double del = line[0] / (double)(npts + 1);
  const GeodOrigin o = geod_origin(lat1, lon1);
  double lat, lon;
  geod_direct_from(o, line[1], (double)(i + 1) * del, lat, lon);
  out_lon[i] = lon;
  out_lat[i] = lat;
}
#endif  // ODR_SEED_HOST

}  // namespace odr
