// Reader blocks convolved before they are prepared (StructuredReader.set_convolution_kernel).
//
//   set_convolution_kernel   readers/basereader/structured.py:163-165   odr_source_set_convolution
//   __convolve_block__       readers/basereader/structured.py:167-192   k_blk_convolve (2-D variables), k_blk_convolve_zy (3-D)
//   applied to a block       readers/basereader/structured.py:278-306   first pass of stage_block, in front of k_blk_mask_fill
//
// The reference calls scipy.ndimage.convolve(array, kernel, mode='nearest'); what that computes, restated:
//   * a correlation with the kernel flipped along both axes (ConvKernel::w holds the flipped weights), whose centre sits at
//     size / 2 along an axis of odd size and one cell less along an axis of even size (ConvKernel::cy, cx);
//   * indices outside the array are clamped to its edge;
//   * one double accumulator per output cell, the terms added in C order of the flipped kernel, each (double)value * weight
//     rounded and then added (no fused multiply-add: conv_acc), the sum rounded once to float32;
//   * weights with |w| <= DBL_EPSILON are no part of the footprint (conv_in_footprint): a NaN under a zero weight does not spread.
// A 2-D variable [ny][nx] is convolved over (y, x).  A 3-D variable [nz][ny][nx] is convolved with kernel[:, :, None], i.e. over
// (z, y): the kernel's first axis runs over the layers, its second over y, and x is not smoothed -- the reference's behaviour, kept.
//
// Compiled for the CPU by tests/convolve_host.cpp: everything above the kernels is plain C++.
#pragma once

namespace odr {

constexpr int CONV_MAX = 15;                      // largest kernel edge
constexpr int CONV_T = 32;                        // 2-D: output cells of one workgroup along y and along x
constexpr int CONV_REGION = CONV_T + CONV_MAX - 1;   // 2-D: edge of the largest staged region, tile + halo (46)
constexpr int CONV_ROWS = 4;                      // 2-D: output cells per thread, CONV_T / CONV_ROWS rows apart
constexpr int CONV_STRIP = 8;                     // 3-D: output cells per thread along y

struct ConvKernel {
  int ky, kx, cy, cx;                 // extent along the first / second axis; centre of the flipped kernel
  double w[CONV_MAX * CONV_MAX];      // flipped weights, [ky][kx]
};

// the flipped kernel of scipy.ndimage.convolve and its centre from the kernel as the caller gave it ([ky][kx], C order)
__host__ __device__ inline void conv_kernel_init(ConvKernel &K, int ky, int kx, const double *weights) {
  K.ky = ky; K.kx = kx;
  K.cy = ky / 2 - (ky % 2 == 0 ? 1 : 0);
  K.cx = kx / 2 - (kx % 2 == 0 ? 1 : 0);
  for (int a = 0; a < ky; ++a)
    for (int b = 0; b < kx; ++b) K.w[a * kx + b] = weights[(ky - 1 - a) * kx + (kx - 1 - b)];
}

__host__ __device__ __forceinline__ int conv_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__host__ __device__ __forceinline__ bool conv_in_footprint(double w) { return fabs(w) > 2.220446049250313e-16; }
__host__ __device__ __forceinline__ double conv_acc(double acc, float v, double w) { return __dadd_rn(acc, __dmul_rn((double)v, w)); }

// 2-D: the value of region cell (ry, rx) of the tile whose first output cell is (y0, x0): the region starts cy rows above and
// cx columns left of it
__host__ __device__ __forceinline__ float conv_region_value(const float *in, int ny, int nx, int y0, int x0, const ConvKernel &K,
                                                            int ry, int rx) {
  return in[(size_t)conv_clamp(y0 - K.cy + ry, ny) * (size_t)nx + (size_t)conv_clamp(x0 - K.cx + rx, nx)];
}

// 2-D: J output cells of column tx of a staged region (row stride `stride`), in the tile's rows ty, ty + dy, ...
template <int J>
__host__ __device__ __forceinline__ void conv_tile_cells(const float *region, int stride, int ty, int dy, int tx, const ConvKernel &K,
                                                         double (&acc)[J]) {
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = 0.0;
  for (int a = 0; a < K.ky; ++a)
    for (int b = 0; b < K.kx; ++b) {
      const double w = K.w[a * K.kx + b];
      if (!conv_in_footprint(w)) continue;
#pragma unroll
      for (int j = 0; j < J; ++j) acc[j] = conv_acc(acc[j], region[(ty + j * dy + a) * stride + tx + b], w);
    }
}

// 3-D: R output cells (z, y0 .. y0 + R - 1) of one column x.  `col` points at in[0][0][x]; layers are `layer` floats apart, rows
// `row`.  Layer by layer of the footprint the column's values y0 - cy .. y0 - cy + R + kx - 2 are read once, R at a time, and each
// goes to every output whose footprint holds it -- for one output in ascending b, layer after layer: the C order of the kernel.
template <int R>
__host__ __device__ __forceinline__ void conv_column(const float *col, size_t layer, size_t row, int nz, int ny, int z, int y0,
                                                     const ConvKernel &K, double (&acc)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  for (int a = 0; a < K.ky; ++a) {
    const float *lay = col + (size_t)conv_clamp(z + a - K.cy, nz) * layer;
    const double *wa = K.w + a * K.kx;
    for (int j0 = 0; j0 < R + K.kx - 1; j0 += R) {
      float v[R];
#pragma unroll
      for (int jj = 0; jj < R; ++jj) v[jj] = lay[(size_t)conv_clamp(y0 - K.cx + j0 + jj, ny) * row];
#pragma unroll
      for (int jj = 0; jj < R; ++jj)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int b = j0 + jj - r;
          if (b >= 0 && b < K.kx) {
            const double w = wa[b];
            if (conv_in_footprint(w)) acc[r] = conv_acc(acc[r], v[jj], w);
          }
        }
    }
  }
}

#ifndef ODR_CONVOLVE_HOST
// One 2-D variable: a workgroup stages the region of its 32 x 32 output cells -- tile plus halo, (31 + ky) x (31 + kx) cells,
// clamped at the array's edges -- in LDS, then a thread forms the four cells of its column that lie eight rows apart.  The lanes of a
// wave half read consecutive LDS words: no bank conflict.  8 464 bytes of LDS per workgroup.
__global__ __launch_bounds__(256) void k_blk_convolve(const float *__restrict__ in, float *__restrict__ out, int ny, int nx, ConvKernel K) {
  __shared__ float region[CONV_REGION * CONV_REGION];
  const int y0 = (int)blockIdx.y * CONV_T, x0 = (int)blockIdx.x * CONV_T;
  const int rh = CONV_T + K.ky - 1, rw = CONV_T + K.kx - 1;
  for (int i = (int)threadIdx.x; i < rh * rw; i += 256) {
    const int ry = i / rw, rx = i - ry * rw;
    region[i] = conv_region_value(in, ny, nx, y0, x0, K, ry, rx);
  }
  __syncthreads();
  const int tx = (int)threadIdx.x & (CONV_T - 1), ty = (int)threadIdx.x / CONV_T;
  double acc[CONV_ROWS];
  conv_tile_cells<CONV_ROWS>(region, rw, ty, CONV_T / CONV_ROWS, tx, K, acc);
  const int x = x0 + tx;
  if (x >= nx) return;
#pragma unroll
  for (int j = 0; j < CONV_ROWS; ++j) {
    const int y = y0 + ty + j * (CONV_T / CONV_ROWS);
    if (y < ny) out[(size_t)y * (size_t)nx + (size_t)x] = (float)acc[j];
  }
}

// One 3-D variable: the footprint is (z, y), so the lanes of a wave hold neighbouring x and every access is coalesced without a tile.
// A thread forms eight cells of its column along y (conv_column).  Workgroups are numbered along x first, then z, then the strips
// along y: the ones in flight together share the rows they read through the caches.
__global__ __launch_bounds__(256) void k_blk_convolve_zy(const float *__restrict__ in, float *__restrict__ out, int nz, int ny, int nx,
                                                         ConvKernel K) {
  const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, z = (int)blockIdx.y, y0 = (int)blockIdx.z * CONV_STRIP;
  if (x >= nx) return;
  const size_t plane = (size_t)ny * (size_t)nx;
  double acc[CONV_STRIP];
  conv_column<CONV_STRIP>(in + x, plane, (size_t)nx, nz, ny, z, y0, K, acc);
  float *o = out + (size_t)z * plane + (size_t)x;
#pragma unroll
  for (int r = 0; r < CONV_STRIP; ++r)
    if (y0 + r < ny) o[(size_t)(y0 + r) * (size_t)nx] = (float)acc[r];
}
#endif  // ODR_CONVOLVE_HOST

}  // namespace odr
