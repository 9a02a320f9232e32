// TEST INFRASTRUCTURE: the bin search and the classification of opendrift_amd/csrc/odr_density.hip.h (the device code of
// OpenDriftSimulation.get_density_array) compiled for the CPU with g++ -ffp-contract=off, so that they can be compared with the
// reference's maps without a GPU (tests/test_density_device_arithmetic.py).  tests/hostshim stands in for <hip/hip_runtime.h>; the
// kernel itself is excluded by ODR_DENSITY_HOST.  The loop does what the kernel does with an entry; the sums are float64 additions in
// the order of the entries (trajectory by trajectory), where the kernel's arrive in any order.
#include <hip/hip_runtime.h>

#define ODR_DENSITY_HOST 1
#include "../opendrift_amd/csrc/odr_density.hip.h"

// bin[i] of v[i] on `edges` (-1: dropped)
extern "C" void densh_bin(long long n, const double *v, int n_edges, const double *edges, int *bin) {
  const odr::DensityAxis a = odr::density_axis(edges, n_edges);
  for (long long i = 0; i < n; ++i) bin[i] = odr::density_bin(v[i], a, edges);
}

extern "C" void densh_classes(long long n, const float *z, const float *status, int stranded_code, int *cls) {
  for (long long i = 0; i < n; ++i) cls[i] = odr::density_classes(z[i], status[i], stranded_code);
}

// inputs [trajectory][time] float32 (weight NULL: counts); H* [time][lon_bin][lat_bin] float64, zeroed by the caller
extern "C" void densh_map(long long n_trajectories, int n_times, const float *lon, const float *lat, const float *z, const float *status,
                          const float *weight, int stranded_code, int n_lon_edges, const double *lon_edges, int n_lat_edges,
                          const double *lat_edges, double *H, double *Hsub, double *Hstr) {
  const odr::DensityAxis ax = odr::density_axis(lon_edges, n_lon_edges), ay = odr::density_axis(lat_edges, n_lat_edges);
  const size_t nlat = (size_t)(n_lat_edges - 1), plane = (size_t)(n_lon_edges - 1) * nlat;
  for (long long e = 0; e < n_trajectories * n_times; ++e) {
    const int ilon = odr::density_bin((double)lon[e], ax, lon_edges);
    const int ilat = ilon >= 0 ? odr::density_bin((double)lat[e], ay, lat_edges) : -1;
    if (ilat < 0) continue;
    const int cls = odr::density_classes(z[e], status[e], stranded_code);
    const size_t dst = (size_t)(e % n_times) * plane + (size_t)ilon * nlat + (size_t)ilat;
    const double w = weight ? (double)weight[e] : 1.0;
    if (cls & odr::DENSITY_SURFACE) H[dst] += w;
    if (cls & odr::DENSITY_SUBMERGED) Hsub[dst] += w;
    if (cls & odr::DENSITY_STRANDED) Hstr[dst] += w;
  }
}
