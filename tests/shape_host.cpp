// TEST INFRASTRUCTURE: the grid index, the list walk, the definition over all edges, the coverage test and the merge of
// opendrift_amd/csrc/odr_shape.hip.h (the device code of readers.ShapeReader) compiled for the CPU with g++ -ffp-contract=off, so
// that they can be compared with each other and with the reference's mask without a GPU (tests/test_shape_device_arithmetic.py).
// tests/hostshim stands in for <hip/hip_runtime.h>; the kernels are excluded by ODR_SHAPE_HOST.  The loops do what the kernels do
// with one element.  With SHAPE_HOST_MAIN it is a program of its own: `shape_host FILE` reads edges and queries from a binary file
// (int64 n_edges, n_poly, n_queries; float64 x1 y1 x2 y2 [n_edges]; int32 poly [n_edges]; float64 qx qy [n_queries]), builds the
// index, answers the queries both ways and prints how many differ.
#include <hip/hip_runtime.h>

#include <cstdio>

#define ODR_SHAPE_HOST 1
#include "../opendrift_amd/csrc/odr_shape.hip.h"

struct shh_shape {
  odr::ShIndex I;
  std::vector<odr::ShEdge> e;
  std::vector<int> poly;
  int n_poly;
  std::string err;
};

extern "C" shh_shape *shh_build(long long n, const double *x1, const double *y1, const double *x2, const double *y2, const int *poly,
                                int n_poly, int nx, int ny, int invert) {
  shh_shape *S = new shh_shape();
  S->e.resize((size_t)(n > 0 ? n : 0));
  for (long long k = 0; k < n; ++k) S->e[(size_t)k] = odr::ShEdge{x1[k], y1[k], x2[k], y2[k]};
  S->poly.assign(poly, poly + (n > 0 ? n : 0));
  S->n_poly = n_poly;
  S->err = odr::sh_build(n, S->e.data(), S->poly.data(), n_poly, nx, ny, invert, S->I);
  return S;
}
extern "C" const char *shh_error(const shh_shape *S) { return S->err.c_str(); }
extern "C" void shh_free(shh_shape *S) { delete S; }

// stats[0 .. 9]: cells, entries, longest list, mean list of the non-empty cells, nudges, nx, ny, x0, y0, dx;  stats[10]: dy
extern "C" void shh_stats(const shh_shape *S, double *stats) {
  const odr::ShGrid &G = S->I.g;
  stats[0] = (double)G.nx * G.ny;
  stats[1] = (double)S->I.tag.size();
  stats[2] = (double)S->I.longest;
  stats[3] = S->I.nonempty ? (double)S->I.tag.size() / (double)S->I.nonempty : 0.0;
  stats[4] = S->I.nudges;
  stats[5] = G.nx; stats[6] = G.ny; stats[7] = G.x0; stats[8] = G.y0; stats[9] = G.dx; stats[10] = G.dy;
}

// per cell of the grid: the number of edge entries and of toggle entries
extern "C" void shh_cell_counts(const shh_shape *S, int *edges, int *toggles) {
  const odr::ShGrid &G = S->I.g;
  for (long long c = 0; c < (long long)G.nx * G.ny; ++c) {
    edges[c] = toggles[c] = 0;
    for (long long k = S->I.off[(size_t)c]; k < S->I.off[(size_t)c + 1]; ++k) ((S->I.tag[(size_t)k] & 1) ? toggles : edges)[c]++;
  }
}

// k_shape_contains: the mask through the index (NaN outside the box)
extern "C" void shh_contains(const shh_shape *S, long long n, const double *x, const double *y, float *out) {
  for (long long i = 0; i < n; ++i) out[i] = odr::sh_mask(S->I.g, x[i], y[i]);
}

// the definition over all edges, with the same box and inversion
extern "C" void shh_all_edges(const shh_shape *S, long long n, const double *x, const double *y, float *out) {
  const odr::ShGrid &G = S->I.g;
  for (long long i = 0; i < n; ++i) {
    if (!odr::sh_covers(G, x[i], y[i])) { out[i] = NAN; continue; }
    const int in = odr::shape_contains_all_edges((long long)S->e.size(), S->e.data(), S->poly.data(), S->n_poly, x[i], y[i]);
    out[i] = (float)(G.invert ? 1 - in : in);
  }
}

// the merge of k_shape_sample on reader coordinates
extern "C" void shh_sample(const shh_shape *S, long long n, const double *x, const double *y, int first, float *out) {
  for (long long i = 0; i < n; ++i) {
    const float v = odr::sh_mask(S->I.g, x[i], y[i]);
    if (std::isfinite(v)) out[i] = odr::sh_merge(v, out[i], first);
  }
}

#ifdef SHAPE_HOST_MAIN
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  long long hdr[3];
  if (fread(hdr, 8, 3, f) != 3) return 2;
  const size_t n = (size_t)hdr[0], q = (size_t)hdr[2];
  std::vector<double> c[4], qx(q), qy(q);
  std::vector<int> poly(n);
  for (auto &a : c) { a.resize(n); if (fread(a.data(), 8, n, f) != n) return 2; }
  if (fread(poly.data(), 4, n, f) != n || fread(qx.data(), 8, q, f) != q || fread(qy.data(), 8, q, f) != q) return 2;
  fclose(f);
  int bad = 0;
  for (int grid : {0, 1, 7}) {
    shh_shape *S = shh_build((long long)n, c[0].data(), c[1].data(), c[2].data(), c[3].data(), poly.data(), (int)hdr[1], grid, grid, 0);
    if (!S->err.empty()) { printf("build: %s\n", S->err.c_str()); return 1; }
    std::vector<float> a(q), b(q);
    shh_contains(S, (long long)q, qx.data(), qy.data(), a.data());
    shh_all_edges(S, (long long)q, qx.data(), qy.data(), b.data());
    long long differ = 0, land = 0;
    for (size_t i = 0; i < q; ++i) {
      differ += !((a[i] == b[i]) || (std::isnan(a[i]) && std::isnan(b[i])));
      land += a[i] == 1.0f;
    }
    double st[11];
    shh_stats(S, st);
    printf("grid %d x %d: %zu edges, %.0f entries, longest list %.0f, %zu queries, %lld on land, %lld differ from the definition\n", (int)st[5],
           (int)st[6], n, st[1], st[2], q, land, differ);
    bad += differ != 0;
    shh_free(S);
  }
  return bad ? 1 : 0;
}
#endif
