// TEST INFRASTRUCTURE: the gradient stencil and the cell function of opendrift_amd/csrc/odr_ftle.hip.h (the device code of
// OpenDriftSimulation.calculate_ftle) compiled for the CPU with g++ -ffp-contract=off, so that they can be compared with the
// reference's physics_methods.ftle and with np.gradient without a GPU (tests/test_ftle_device_arithmetic.py).  tests/hostshim stands
// in for <hip/hip_runtime.h>; the kernels themselves are excluded by ODR_FTLE_HOST.  The loops do what k_ftle_cell does with a cell.
#include <hip/hip_runtime.h>
#include <cstddef>

#define ODR_FTLE_HOST 1
#include "../opendrift_amd/csrc/odr_ftle.hip.h"

// np.gradient(f) of a [ny][nx] float64 plane with unit spacing: g0 along axis 0 (rows), g1 along axis 1
extern "C" void ftleh_gradient(int nx, int ny, const double *f, double *g0, double *g1) {
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {
      const size_t e = (size_t)j * (size_t)nx + (size_t)i;
      g0[e] = odr::ftle_gradient(f + i, (size_t)nx, j, ny);
      g1[e] = odr::ftle_gradient(f + (size_t)j * (size_t)nx, 1, i, nx);
    }
}

// physics_methods.ftle(dX, dY, delta, duration) of [ny][nx] float64 displacement planes: out [ny][nx] float32
extern "C" void ftleh_map(int nx, int ny, const double *dX, const double *dY, double delta, double duration_seconds, float *out) {
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i)
      out[(size_t)j * (size_t)nx + (size_t)i] = odr::ftle_cell(dX, dY, nx, ny, i, j, 2 * delta, std::fabs(duration_seconds));
}
