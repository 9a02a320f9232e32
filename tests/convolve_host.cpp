// TEST INFRASTRUCTURE: the routines of opendrift_amd/csrc/odr_convolve.hip.h (the device code of
// StructuredReader.set_convolution_kernel) compiled for the CPU with g++ -ffp-contract=off, so that they can be compared with the
// reference's __convolve_block__ without a GPU (tests/test_convolve_device_arithmetic.py).  tests/hostshim stands in for
// <hip/hip_runtime.h>; the kernels themselves are excluded by ODR_CONVOLVE_HOST.  The loops below do what the kernels do with a
// workgroup and a thread: the same tiles, regions, strips and calls.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <vector>

#define ODR_CONVOLVE_HOST 1
#include "../opendrift_amd/csrc/odr_convolve.hip.h"

using namespace odr;

extern "C" int convh_max_edge() { return CONV_MAX; }
extern "C" int convh_tile_edge() { return CONV_T; }
extern "C" int convh_strip() { return CONV_STRIP; }

// k_blk_convolve: one 2-D variable [ny][nx]
extern "C" void convh_2d(const float *in, float *out, int ny, int nx, int ky, int kx, const double *weights) {
  ConvKernel K;
  conv_kernel_init(K, ky, kx, weights);
  std::vector<float> region((size_t)CONV_REGION * CONV_REGION);
  const int rh = CONV_T + K.ky - 1, rw = CONV_T + K.kx - 1, dy = CONV_T / CONV_ROWS;
  for (int y0 = 0; y0 < ny; y0 += CONV_T)
    for (int x0 = 0; x0 < nx; x0 += CONV_T) {
      for (int i = 0; i < rh * rw; ++i) region[(size_t)i] = conv_region_value(in, ny, nx, y0, x0, K, i / rw, i % rw);
      for (int t = 0; t < 256; ++t) {
        const int tx = t & (CONV_T - 1), ty = t / CONV_T;
        double acc[CONV_ROWS];
        conv_tile_cells<CONV_ROWS>(region.data(), rw, ty, dy, tx, K, acc);
        for (int j = 0; j < CONV_ROWS; ++j) {
          const int y = y0 + ty + j * dy, x = x0 + tx;
          if (y < ny && x < nx) out[(size_t)y * (size_t)nx + (size_t)x] = (float)acc[j];
        }
      }
    }
}

// k_blk_convolve_zy: one 3-D variable [nz][ny][nx]
extern "C" void convh_3d(const float *in, float *out, int nz, int ny, int nx, int ky, int kx, const double *weights) {
  ConvKernel K;
  conv_kernel_init(K, ky, kx, weights);
  const size_t plane = (size_t)ny * (size_t)nx;
  for (int y0 = 0; y0 < ny; y0 += CONV_STRIP)
    for (int z = 0; z < nz; ++z)
      for (int x = 0; x < nx; ++x) {
        double acc[CONV_STRIP];
        conv_column<CONV_STRIP>(in + x, plane, (size_t)nx, nz, ny, z, y0, K, acc);
        for (int r = 0; r < CONV_STRIP; ++r)
          if (y0 + r < ny) out[(size_t)z * plane + (size_t)(y0 + r) * (size_t)nx + (size_t)x] = (float)acc[r];
      }
}
