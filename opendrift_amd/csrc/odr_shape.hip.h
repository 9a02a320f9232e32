// Land mask from coastline polygons: an exact point-in-polygon-set test behind a uniform grid.
//
//   Reader._on_land, get_variables (shapely.contains_xy of the union)   readers/reader_shape.py:106-130   sh_contains, k_shape_sample
//   covers_positions_xy                                                 readers/basereader/variables.py:229-257   um_covers' rule
//
// THE DEFINITION (shape_contains_all_edges): per polygon the parity of its edges, all rings, with
//     (y1 > py) != (y2 > py)   and   x1 + (py - y1) * (x2 - x1) / (y2 - y1) < px
// (the crossings of the ray from the point towards -x, half-open in y); land is the OR of the parities over the polygons, so
// polygons may overlap, a hole is one more ring of its polygon and an island in a lake is a polygon of its own.
//
// THE INDEX: a uniform grid over the box of the rings; vertical lines x = sh_line(x0, dx, i), horizontal ones y = sh_line(y0, dy, j),
// none of them through a vertex (the origin sits a fraction of the pitch outside the box and is shifted until that holds).  The
// list of a cell holds, sorted by polygon,
//   * an edge entry for every edge that comes near the closed cell: per row band the edge's x-range within the band, widened by
//     one cell on either side (a superset; rounding of the crossing abscissae cannot carry a crossing out of it);
//   * a toggle entry for every polygon whose parity, by the definition, is odd at the cell's lower-left corner (xL, yB).
// A query in the cell walks the list once: from the corner up the line x = xL to (xL, py), then along y = py to (px, py).  A
// toggle flips the parity of its polygon; an edge flips it when it crosses the vertical leg, (x1 > xL) != (x2 > xL) with
// yB < yc <= py, and when it crosses the horizontal leg, the definition's y test with xL <= xc < px -- xc formed exactly as the
// definition forms it.  The cost of a query is the length of its cell's list: the local density of edges, not the size of the
// coastline.  An empty list is water; a cell deep inside one polygon holds one toggle.
//
// Every float64 operation is rounded on its own (no fused multiply-add), divisions are IEEE: a host build gives the device's bits.
// Everything above the kernels is plain C++ and is compiled for the CPU by tests/shape_host.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace odr {

struct alignas(16) ShEdge { double x1, y1, x2, y2; };      // 32 bytes: two 16-byte loads
constexpr int SHAPE_MAXPOLY = 1 << 30;                      // a list entry's tag: polygon << 1 | (1: toggle, 0: edge)

// the grid and its lists; ent / tag / off live where the query runs (device memory for the kernels, host memory for sh_build's caller)
struct ShGrid {
  double x0, y0, dx, dy;                 // line i: sh_line(x0, dx, i)
  double xmin, xmax, ymin, ymax;         // the box of the rings: the reader's coverage
  const long long *off;                  // [nx * ny + 1], cell = j * nx + i
  const ShEdge *ent;                     // [entries]; unused at a toggle
  const int *tag;                        // [entries]
  int nx, ny, invert, lon_mode;
};

// one rounding per operation: the device intrinsics in device code; on the host the plain operators, which the build keeps
// uncontracted (-ffp-contract=off) -- the index is built by host code that forms the lines as the kernels do
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double sh_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double sh_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double sh_mul(double a, double b) { return __dmul_rn(a, b); }
#else
inline double sh_add(double a, double b) { return a + b; }
inline double sh_sub(double a, double b) { return a - b; }
inline double sh_mul(double a, double b) { return a * b; }
#endif

__host__ __device__ __forceinline__ double sh_line(double o, double d, int i) { return sh_add(o, sh_mul((double)i, d)); }

// the index c in 0 .. n - 1 with line(c) <= p < line(c + 1), corrected after the floor; clamped at the ends
__host__ __device__ __forceinline__ int sh_cell(double p, double o, double d, int n) {
  double t = floor(sh_sub(p, o) / d);
  t = t < 0.0 ? 0.0 : t;
  t = t > (double)(n - 1) ? (double)(n - 1) : t;
  int c = (int)t;
  while (c > 0 && p < sh_line(o, d, c)) --c;
  while (c < n - 1 && p >= sh_line(o, d, c + 1)) ++c;
  return c;
}

// the abscissa at which the edge's line meets y = py, as the definition forms it
__host__ __device__ __forceinline__ double sh_xc(const ShEdge &e, double py) {
  return sh_add(e.x1, sh_mul(sh_sub(py, e.y1), sh_sub(e.x2, e.x1)) / sh_sub(e.y2, e.y1));
}

// the definition's crossing test of one edge for the ray from (px, py) towards -x
__host__ __device__ __forceinline__ bool sh_ray_crosses(const ShEdge &e, double px, double py) {
  if ((e.y1 > py) == (e.y2 > py)) return false;
  return sh_xc(e, py) < px;
}

// 1 when the edge crosses the path (xL, yB) -> (xL, py) -> (px, py) an odd number of times
__host__ __device__ __forceinline__ int sh_edge_flip(const ShEdge &e, double xL, double yB, double px, double py) {
  int f = 0;
  if ((e.x1 > xL) != (e.x2 > xL)) {
    double yc = sh_add(e.y1, sh_mul(sh_sub(xL, e.x1), sh_sub(e.y2, e.y1)) / sh_sub(e.x2, e.x1));
    yc = fmin(fmax(yc, fmin(e.y1, e.y2)), fmax(e.y1, e.y2));      // stays within the edge: the edge is in the lists of its own bands only
    f ^= (yB < yc && yc <= py) ? 1 : 0;
  }
  if ((e.y1 > py) != (e.y2 > py)) {
    const double xc = sh_xc(e, py);
    f ^= (xL <= xc && xc < px) ? 1 : 0;
  }
  return f;
}

// contains_xy(unary_union(polys), px, py) for a point inside the box of the rings
__host__ __device__ __forceinline__ int sh_contains(const ShGrid &G, double px, double py) {
  const int i = sh_cell(px, G.x0, G.dx, G.nx), j = sh_cell(py, G.y0, G.dy, G.ny);
  const double xL = sh_line(G.x0, G.dx, i), yB = sh_line(G.y0, G.dy, j);
  const long long cell = (long long)j * G.nx + i;
  const long long a = G.off[cell], b = G.off[cell + 1];
  int par = 0, cur = -1;
  for (long long k = a; k < b; ++k) {
    const int t = G.tag[k], poly = t >> 1;
    if (poly != cur) {
      if (par) return 1;      // (OR over the polygons: one odd parity decides)
      cur = poly;
    }
    if (t & 1) par ^= 1;
    else {
      const ShEdge e = G.ent[k];
      par ^= sh_edge_flip(e, xL, yB, px, py);
    }
  }
  return par;
}

// covers_positions_xy with the reader's default zmin / zmax: the box of the rings, ends included; x + y not finite is outside
__host__ __device__ __forceinline__ bool sh_covers(const ShGrid &G, double x, double y) {
  return std::isfinite(x + y) && x >= G.xmin && x <= G.xmax && y >= G.ymin && y <= G.ymax;
}

// land_binary_mask of the reader at (x, y) in its own coordinates: NaN outside the box, else contains or, inverted, 1 - contains
__host__ __device__ __forceinline__ float sh_mask(const ShGrid &G, double x, double y) {
  if (!sh_covers(G, x, y)) return NAN;
  const int in = sh_contains(G, x, y);
  return (float)(G.invert ? 1 - in : in);
}

// the priority-list rule for a reader outside the device's own lists (as um_merge)
__host__ __device__ __forceinline__ float sh_merge(float val, float cur, int first) {
  return std::isfinite(val) && (first || !std::isfinite(cur)) ? val : cur;
}

// ---- the definition, over all edges (tests, and the toggles of the index are formed by the same test)
inline int shape_contains_all_edges(long long n_edges, const ShEdge *e, const int *poly, int n_poly, double px, double py) {
  std::vector<unsigned char> par((size_t)n_poly, 0);
  for (long long k = 0; k < n_edges; ++k)
    if (sh_ray_crosses(e[k], px, py)) par[(size_t)poly[k]] ^= 1;
  for (unsigned char p : par) if (p) return 1;
  return 0;
}

// ---- the index, built once on the host
struct ShIndex {
  ShGrid g;                          // off / ent / tag point into the vectors below
  std::vector<long long> off;
  std::vector<ShEdge> ent;
  std::vector<int> tag;
  int nudges = 0;                    // times the origin was shifted because a line passed through a vertex
  long long longest = 0, nonempty = 0;
};

constexpr double SHAPE_ORIGIN_FRACTION = 0.381966011250105;      // of the pitch, outside the box; < SHAPE_SPARE
constexpr double SHAPE_SPARE = 0.75;                             // the grid is this fraction of a pitch wider than the box
constexpr long long SHAPE_MAXCELLS = 1ll << 28;

// Edges of zero length must have been dropped; poly[k] in 0 .. n_poly - 1.  nx, ny: 0 = automatic (about two cells per edge,
// shaped as the box).  Returns "" or what is wrong.
inline std::string sh_build(long long n, const ShEdge *e, const int *poly, int n_poly, int nx, int ny, int invert, ShIndex &I) {
  if (n < 1) return "no edges";
  if (n_poly < 1 || n_poly >= SHAPE_MAXPOLY) return "bad polygon count";
  double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  for (long long k = 0; k < n; ++k) {
    if (!std::isfinite(e[k].x1 + e[k].y1 + e[k].x2 + e[k].y2)) return "a vertex is not finite";
    if (e[k].x1 == e[k].x2 && e[k].y1 == e[k].y2) return "an edge of zero length";
    if (poly[k] < 0 || poly[k] >= n_poly) return "an edge of a polygon that does not exist";
    xmin = fmin(xmin, fmin(e[k].x1, e[k].x2)); xmax = fmax(xmax, fmax(e[k].x1, e[k].x2));
    ymin = fmin(ymin, fmin(e[k].y1, e[k].y2)); ymax = fmax(ymax, fmax(e[k].y1, e[k].y2));
  }
  const double w = xmax > xmin ? xmax - xmin : 1.0, h = ymax > ymin ? ymax - ymin : 1.0;
  if (nx < 0 || ny < 0) return "a negative grid size";
  if (nx == 0 || ny == 0) {
    const double cells = 2.0 * (double)n;
    int ax = (int)fmin(fmax(ceil(sqrt(cells * w / h)), 1.0), 32768.0), ay = (int)fmin(fmax(ceil(sqrt(cells * h / w)), 1.0), 32768.0);
    if (nx == 0) nx = ax;
    if (ny == 0) ny = ay;
  }
  if ((long long)nx * ny > SHAPE_MAXCELLS) return "more than 2^28 cells";
  ShGrid &G = I.g;
  G.xmin = xmin; G.xmax = xmax; G.ymin = ymin; G.ymax = ymax;
  G.nx = nx; G.ny = ny; G.invert = invert != 0; G.lon_mode = 0;
  G.dx = w / ((double)nx - SHAPE_SPARE);
  G.dy = h / ((double)ny - SHAPE_SPARE);
  // the origin: no line through a vertex (a vertex on a line would sit on a leg's end for every query of the row or column)
  I.nudges = 0;
  for (;; ++I.nudges) {
    if (I.nudges > 64) return "no grid origin keeps the lines off the vertices";
    double f = SHAPE_ORIGIN_FRACTION + 0.0918273645 * I.nudges;
    f -= floor(f / 0.7) * 0.7;      // stays in (0, 0.7): below SHAPE_SPARE
    if (f < 0.01) f += 0.0123;
    G.x0 = xmin - f * G.dx;
    G.y0 = ymin - f * G.dy;
    if (!(G.x0 < xmin && sh_line(G.x0, G.dx, nx) > xmax && G.y0 < ymin && sh_line(G.y0, G.dy, ny) > ymax)) return "the grid does not cover the box";
    bool hit = false;
    for (long long k = 0; k < n && !hit; ++k) {
      const double vx[2] = {e[k].x1, e[k].x2}, vy[2] = {e[k].y1, e[k].y2};
      for (int v = 0; v < 2; ++v)
        hit |= sh_line(G.x0, G.dx, sh_cell(vx[v], G.x0, G.dx, nx)) == vx[v] || sh_line(G.y0, G.dy, sh_cell(vy[v], G.y0, G.dy, ny)) == vy[v];
    }
    if (!hit) break;
  }
  const long long ncell = (long long)nx * ny;
  // toggles: per row of corners, the polygons whose parity is odd at (line i, line j), swept along the row
  struct Ev { int i, poly; };
  std::vector<std::vector<Ev>> row_ev((size_t)ny);
  for (long long k = 0; k < n; ++k) {
    const double ylo = fmin(e[k].y1, e[k].y2), yhi = fmax(e[k].y1, e[k].y2);
    const int j0 = sh_cell(ylo, G.y0, G.dy, ny), j1 = std::min(ny - 1, sh_cell(yhi, G.y0, G.dy, ny) + 1);
    for (int j = j0; j <= j1; ++j) {
      const double yB = sh_line(G.y0, G.dy, j);
      if ((e[k].y1 > yB) == (e[k].y2 > yB)) continue;
      const double xc = sh_xc(e[k], yB);
      // the first corner of the row with xc < its x
      int i;
      if (xc < G.x0) i = 0;
      else {
        i = sh_cell(xc, G.x0, G.dx, nx);
        if (!(xc < sh_line(G.x0, G.dx, i))) ++i;
      }
      if (i < nx) row_ev[(size_t)j].push_back({i, poly[k]});
    }
  }
  // two passes over the same enumeration: count, then fill
  I.off.assign((size_t)ncell + 1, 0);
  std::vector<long long> fill;
  auto enumerate = [&](auto &&emit) {
    for (long long k = 0; k < n; ++k) {
      const ShEdge &E = e[k];
      const double ylo = fmin(E.y1, E.y2), yhi = fmax(E.y1, E.y2);
      const int j0 = sh_cell(ylo, G.y0, G.dy, ny), j1 = sh_cell(yhi, G.y0, G.dy, ny);
      for (int j = j0; j <= j1; ++j) {
        double xa, xb;
        if (j0 == j1 || E.y1 == E.y2) { xa = E.x1; xb = E.x2; }
        else {      // the part of the edge within the band
          const double ya = fmax(ylo, sh_line(G.y0, G.dy, j)), yb = fmin(yhi, sh_line(G.y0, G.dy, j + 1));
          xa = E.x1 + (ya - E.y1) * (E.x2 - E.x1) / (E.y2 - E.y1);
          xb = E.x1 + (yb - E.y1) * (E.x2 - E.x1) / (E.y2 - E.y1);
        }
        const double xl = fmax(fmin(xa, xb), fmin(E.x1, E.x2)), xh = fmin(fmax(xa, xb), fmax(E.x1, E.x2));
        const int i0 = std::max(0, sh_cell(xl, G.x0, G.dx, nx) - 1), i1 = std::min(nx - 1, sh_cell(xh, G.x0, G.dx, nx) + 1);
        for (int i = i0; i <= i1; ++i) emit((long long)j * nx + i, poly[k] << 1, &E);
      }
    }
    std::vector<int> odd;      // sorted
    for (int j = 0; j < ny; ++j) {
      std::vector<Ev> &ev = row_ev[(size_t)j];
      std::sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) { return a.i < b.i || (a.i == b.i && a.poly < b.poly); });
      odd.clear();
      size_t at = 0;
      for (int i = 0; i < nx; ++i) {
        for (; at < ev.size() && ev[at].i == i; ++at) {
          auto it = std::lower_bound(odd.begin(), odd.end(), ev[at].poly);
          if (it != odd.end() && *it == ev[at].poly) odd.erase(it);
          else odd.insert(it, ev[at].poly);
        }
        for (int p : odd) emit((long long)j * nx + i, (p << 1) | 1, (const ShEdge *)nullptr);
      }
    }
  };
  enumerate([&](long long cell, int, const ShEdge *) { ++I.off[(size_t)cell + 1]; });
  for (long long c = 0; c < ncell; ++c) I.off[(size_t)c + 1] += I.off[(size_t)c];
  const long long total = I.off[(size_t)ncell];
  I.ent.assign((size_t)total, ShEdge{0.0, 0.0, 0.0, 0.0});
  I.tag.assign((size_t)total, 0);
  fill.assign(I.off.begin(), I.off.end() - 1);
  enumerate([&](long long cell, int tag, const ShEdge *E) {
    const long long at = fill[(size_t)cell]++;
    I.tag[(size_t)at] = tag;
    if (E) I.ent[(size_t)at] = *E;
  });
  // each list sorted by polygon (stable: the order within a polygon does not matter to a parity)
  std::vector<std::pair<int, ShEdge>> tmp;
  I.longest = 0; I.nonempty = 0;
  for (long long c = 0; c < ncell; ++c) {
    const long long a = I.off[(size_t)c], b = I.off[(size_t)c + 1];
    if (b > a) ++I.nonempty;
    I.longest = std::max(I.longest, b - a);
    if (b - a < 2) continue;
    bool sorted = true;
    for (long long k = a + 1; k < b && sorted; ++k) sorted = (I.tag[(size_t)k - 1] >> 1) <= (I.tag[(size_t)k] >> 1);
    if (sorted) continue;
    tmp.clear();
    for (long long k = a; k < b; ++k) tmp.push_back({I.tag[(size_t)k], I.ent[(size_t)k]});
    std::stable_sort(tmp.begin(), tmp.end(), [](const std::pair<int, ShEdge> &p, const std::pair<int, ShEdge> &q) { return (p.first >> 1) < (q.first >> 1); });
    for (long long k = a; k < b; ++k) { I.tag[(size_t)k] = tmp[(size_t)(k - a)].first; I.ent[(size_t)k] = tmp[(size_t)(k - a)].second; }
  }
  G.off = I.off.data();
  G.ent = I.ent.data();
  G.tag = I.tag.data();
  return "";
}

#ifndef ODR_SHAPE_HOST
// The bare query on given reader coordinates: out[i] = land_binary_mask (NaN outside the box of the rings)
__global__ __launch_bounds__(BLOCK) void k_shape_contains(ShGrid G, long long n, const double *__restrict__ x, const double *__restrict__ y,
                                                          float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = sh_mask(G, x[i], y[i]);
}

// One element per lane: position -> reader coordinates -> coverage box -> list walk -> invert -> merge into the land_binary_mask slot
__global__ __launch_bounds__(BLOCK) void k_shape_sample(DevProj P, ShGrid G, int first, long long n, const double *__restrict__ lon,
                                                        const double *__restrict__ lat, float *__restrict__ out) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double x, y;
  if (P.kind == PROJ_LATLONG) {      // get_variables_interpolated: modulate_longitude, then lonlat2xy is the identity
    x = lon[i];
    y = lat[i];
    if (G.lon_mode == 1) x = np_mod(x + 180.0, 360.0) - 180.0;
    else if (G.lon_mode == 2) x = np_mod(x, 360.0);
  } else proj_fwd(P, lon[i], lat[i], x, y);
  const float val = sh_mask(G, x, y);
  if (!std::isfinite(val)) return;      // outside the box: keeps what it has (the next reader, or the fallback)
  out[i] = sh_merge(val, out[i], first);
}
#endif  // ODR_SHAPE_HOST

}  // namespace odr
