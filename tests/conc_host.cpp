// TEST INFRASTRUCTURE: the arithmetic above the kernels of opendrift_amd/csrc/odr_conc.hip.h (the device code of get_density_array_proj,
// get_radionuclide_density_array and horizontal_smooth) compiled for the CPU with g++ -ffp-contract=off, so that it can be compared
// with NumPy, the reference's output and known answers without a GPU (tests/test_conc_device_arithmetic.py).  tests/hostshim stands in
// for <hip/hip_runtime.h>; the kernels are excluded by ODR_CONC_HOST / ODR_DENSITY_HOST.
#include <hip/hip_runtime.h>

#define ODR_DENSITY_HOST 1
#define ODR_CONC_HOST 1
#include "../opendrift_amd/csrc/odr_conc.hip.h"

extern "C" void conch_moved(long long n, const float *z, const float *status, int stranded_code, int *moved) {
  for (long long i = 0; i < n; ++i) moved[i] = odr::conc_moved(z[i], status[i], stranded_code);
}

extern "C" void conch_layer(long long n, const double *z, int nb, const double *zb, int *layer) {
  for (long long i = 0; i < n; ++i) layer[i] = odr::conc_layer(z[i], zb, nb);
}

extern "C" void conch_species_class(long long n, const float *specie, const float *z, int n_species, int nb, const double *zb, int *cls) {
  for (long long i = 0; i < n; ++i) cls[i] = odr::conc_species_class(specie[i], z[i], n_species, zb, nb);
}

// lon0 in degrees, as the descriptor has it
extern "C" void conch_moll(long long n, int inverse, double a, double lon0_deg, double x0, double y0, const double *u, const double *v,
                           double *p, double *q) {
  for (long long i = 0; i < n; ++i) {
    if (inverse) odr::conc_moll_inv(a, lon0_deg * odr::kConcDeg, x0, y0, u[i], v[i], p[i], q[i]);
    else odr::conc_moll_fwd(a, lon0_deg * odr::kConcDeg, x0, y0, u[i], v[i], p[i], q[i]);
  }
}

// horizontal_smooth of one plane a[n0][n1] in the two passes of k_conc_box
extern "C" void conch_box(long long n0, long long n1, long long n, const double *a, long long *tmp, double *out) {
  for (long long i = 0; i < n0; ++i)
    for (long long j = 0; j < n1; ++j) tmp[i * n1 + j] = odr::conc_box_sum(a + i * n1, n1, 1, j, n);
  const double w = 2.0 * (double)n + 1.0;
  for (long long i = 0; i < n0; ++i)
    for (long long j = 0; j < n1; ++j) out[i * n1 + j] = (double)odr::conc_box_sum(tmp + j, n0, n1, i, n) / (w * w);
}
