// TEST INFRASTRUCTURE: the seeding geometry of opendrift_amd/csrc/odr_seed.hip.h (the device code of seed_within_polygon)
// compiled for the CPU with g++ -ffp-contract=off, so that it can be compared with the reference's values and with matplotlib
// without a GPU (tests/test_seed_host.py) and with the device bit for bit (tests/test_gpu_seed.py).  tests/hostshim stands in
// for <hip/hip_runtime.h>; the kernels are excluded by ODR_SEED_HOST.  The loops do what the kernels do: one grid point at a
// time in grid order, the inside points kept in that order.
#include <hip/hip_runtime.h>

#define ODR_GEODINV_HOST 1
#define ODR_SEED_HOST 1
#include "../opendrift_amd/csrc/odr_seed.hip.h"

extern "C" void seedh_points_in_polygon(long long n, const double *x, const double *y, int m, const double *vx, const double *vy,
                                        unsigned char *inside) {
  for (long long i = 0; i < n; ++i) {
    unsigned in = 0;
    double x0 = vx[0], y0 = vy[0];
    bool yflag0 = y0 >= y[i];
    for (int e = 0; e < m; ++e) {
      const int k = e + 1 == m ? 0 : e + 1;
      yflag0 = odr::pip_edge(x[i], y[i], x0, y0, yflag0, vx[k], vy[k], in);
      x0 = vx[k]; y0 = vy[k];
    }
    inside[i] = (unsigned char)in;
  }
}

// The signature of odr_polygon_points and its return values (0, or -1 where that one returns ODR_ERR_INVALID).  mask (may be
// NULL): room for the inside flag of every grid point; the caller sizes it from a first call with mask NULL.
extern "C" int seedh_polygon_points(int m, const double *lons, const double *lats, long long number, double *out_lon, double *out_lat,
                                    long long *n_inside, int *nx, int *ny, unsigned char *mask) {
  if (m < 3 || number < 1) return -1;
  for (int k = 0; k < m; ++k) if (!std::isfinite(lons[k]) || !std::isfinite(lats[k])) return -1;
  odr::SeedPlan P;
  std::vector<double> rx, ry;
  if (odr::seed_plan(m, lons, lats, number, P, rx, ry) != odr::SEED_OK) return -1;
  *nx = P.nx; *ny = P.ny; *n_inside = 0;
  const long long n = (long long)P.nx * P.ny;
  if (n == 0) {
    odr::seed_centre(m, lons, lats, number, out_lon, out_lat);
    return 0;
  }
  const int mc = (int)rx.size();
  long long L = 0;
  for (long long i = 0; i < n; ++i) {
    double lon, lat;
    odr::seed_grid_point(P, i, lon, lat);
    unsigned char in;
    seedh_points_in_polygon(1, &lon, &lat, mc, rx.data(), ry.data(), &in);
    if (mask) mask[i] = in;
    if (in) {
      if (L < number) { out_lon[L] = lon; out_lat[L] = lat; }
      ++L;
    }
  }
  *n_inside = L;
  if (L == 0) {
    odr::seed_border(m, lons, lats, number, out_lon, out_lat);
    return 0;
  }
  odr::seed_cyclic(out_lon, L < number ? L : number, number);
  odr::seed_cyclic(out_lat, L < number ? L : number, number);
  return 0;
}

// The projection alone, for the tests of its round trip: forward != 0 projects (lon, lat) to (x, y), else back
extern "C" int seedh_albers(double lat1, double lat2, double lat0, double lon0, long long n, const double *a, const double *b, double *u,
                            double *v, int forward) {
  odr::Albers A;
  if (odr::aea_setup(lat1, lat2, lat0, lon0, A)) return -1;
  for (long long i = 0; i < n; ++i) {
    if (forward) odr::aea_forward(A, a[i], b[i], u[i], v[i]);
    else odr::aea_inverse(A, a[i], b[i], u[i], v[i]);
  }
  return 0;
}
