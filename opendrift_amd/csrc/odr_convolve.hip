// libodrift_hip.so, a translation unit of its own: reader blocks convolved in front of their preparation
// (StructuredReader.set_convolution_kernel / __convolve_block__, readers/basereader/structured.py:163-192).  See odrift.hip for the
// rest: stage_block calls odr_i_blk_convolve per variable on the upload stream.
#include "odr_host.h"
#include "odr_convolve.hip.h"

// reader.convolve of one grid source: weights[ky][kx] as the reference hands them to scipy.ndimage.convolve; ky = kx = 0 clears.
// In force for the levels uploaded afterwards; resident levels stay as they are.
int odr_source_set_convolution(odr_ctx *c, int32_t sid, int32_t ky, int32_t kx, const double *weights, int32_t n3d, const int32_t *vars3d) {
  REQUIRE(c, "NULL context");
  REQUIRE(sid >= 0 && sid < c->nsrc && !c->src_free[sid] && c->hw.src[sid].kind == SRC_GRID, "source %d is not a grid source", sid);
  if (ky == 0 && kx == 0) {
    c->conv_ky[sid] = c->conv_kx[sid] = 0;
    c->conv_3d[sid] = 0;
    c->conv_w[sid].clear();
    return 0;
  }
  REQUIRE(ky >= 1 && kx >= 1, "convolution kernel of %d x %d weights", (int)ky, (int)kx);
  REQUIRE(ky <= CONV_MAX && kx <= CONV_MAX, "convolution kernel of %d x %d weights: at most %d x %d fit", (int)ky, (int)kx, CONV_MAX, CONV_MAX);
  REQUIRE(weights, "NULL weights");
  REQUIRE(n3d >= 0 && (n3d == 0 || vars3d), "bad list of 3-D variables");
  unsigned mask = 0;
  for (int k = 0; k < n3d; ++k) {
    REQUIRE(vars3d[k] >= 0 && vars3d[k] < NVAR, "bad variable id %d", (int)vars3d[k]);
    mask |= 1u << vars3d[k];
  }
  c->conv_ky[sid] = ky; c->conv_kx[sid] = kx;
  c->conv_3d[sid] = mask;
  c->conv_w[sid].assign(weights, weights + (size_t)ky * (size_t)kx);
  return 0;
}

bool odr_i_source_convolves(const odr_ctx *c, int32_t sid) { return c->conv_ky[sid] > 0; }

// dst <- src convolved: variable `var`, [nzv][ny][nx], of a level of source sid.  Over (z, y) when it has several layers or was
// declared a 3-D array of one layer, else over (y, x).  src != dst.
int odr_i_blk_convolve(odr_ctx *c, int32_t sid, int var, const float *src, float *dst, int nzv, int ny, int nx, hipStream_t st) {
  ConvKernel K;
  conv_kernel_init(K, c->conv_ky[sid], c->conv_kx[sid], c->conv_w[sid].data());
  if (nzv <= 1 && !((c->conv_3d[sid] >> var) & 1u)) {
    const unsigned gx = (unsigned)((nx + CONV_T - 1) / CONV_T), gy = (unsigned)((ny + CONV_T - 1) / CONV_T);
    REQUIRE(gy < 65536, "a convolved level of %d rows", ny);
    hipLaunchKernelGGL(k_blk_convolve, dim3(gx, gy), dim3(256), 0, st, src, dst, ny, nx, K);
  } else {
    const int nz = nzv > 1 ? nzv : 1;
    const unsigned gx = (unsigned)((nx + 255) / 256), gz = (unsigned)((ny + CONV_STRIP - 1) / CONV_STRIP);
    REQUIRE(nz < 65536 && gz < 65536, "a convolved level of %d layers and %d rows", nz, ny);
    hipLaunchKernelGGL(k_blk_convolve_zy, dim3(gx, (unsigned)nz, gz), dim3(256), 0, st, src, dst, nz, ny, nx, K);
  }
  HIPCHK(hipGetLastError());
  return 0;
}
