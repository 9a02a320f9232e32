// FTLE maps: finite-time Lyapunov exponents of a grid of elements, one per cell (OpenDriftSimulation.calculate_ftle).
//
//   calculate_ftle       models/basemodel/__init__.py:4844-4923    k_ftle_displacement (b_x1 - X, b_y1 - Y of :4900-4902, :4913-4915)
//   physics_methods.ftle models/physics_methods.py:458-484         ftle_gradient, ftle_cell, k_ftle_cell
//   np.gradient          (numpy/lib/_function_base_impl.py, unit spacing, edge_order 1)   ftle_gradient
//
// The arithmetic restates the reference's, quirks included:
//   * what is differentiated is the DISPLACEMENT b_x1 - X, not the flow map b_x1 (:4902) -- the Jacobian is that of the flow map
//     minus the identity;
//   * np.gradient is called without a spacing, i.e. with unit spacing, so its interior values are already halved differences
//     (f[k + 1] - f[k - 1]) / 2 and its end values plain differences; the reference divides them by 2 * delta once more (:471-474).
// Per cell: the four gradient values in float64, each divided by 2 * delta in float64 and rounded to float32 once (J is a float32
// array, :463); D = J^T J in float32, one multiply and one add per term in the order written below (the unit is compiled with
// -ffp-contract=off, as tests/ftle_host.cpp is); its largest eigenvalue by the closed form of a symmetric 2 x 2 matrix in float64,
// rounded to float32 (the reference asks LAPACK: np.linalg.eigvals of the float32 D); log(sqrt(lambda)) / |T| in float64, rounded
// to float32 once.  lambda == 0 gives -inf (np.log(0.)); a NaN anywhere in the stencil gives NaN -- the one deviation: the reference's
// LAPACK call raises on a NaN, here the cell is NaN and the caller masks it.
//
// Compiled for the CPU by tests/ftle_host.cpp: everything above the kernels is plain C++.
#pragma once

namespace odr {

// np.gradient(f, axis) with unit spacing at index k of an axis of n >= 2 values `stride` apart; f points at index 0 of the axis
__host__ __device__ __forceinline__ double ftle_gradient(const double *f, size_t stride, int k, int n) {
  if (k == 0) return f[stride] - f[0];
  if (k == n - 1) return f[(size_t)(n - 1) * stride] - f[(size_t)(n - 2) * stride];
  return (f[(size_t)(k + 1) * stride] - f[(size_t)(k - 1) * stride]) / 2.0;
}

// FTLE of cell (row j, column i) of the [ny][nx] displacement planes dX, dY; two_delta = 2 * delta, abs_T = |duration|
__host__ __device__ __forceinline__ float ftle_cell(const double *dX, const double *dY, int nx, int ny, int i, int j, double two_delta,
                                                    double abs_T) {
  const size_t row = (size_t)j * (size_t)nx, col = (size_t)i;
  // np.gradient returns [along axis 0 (rows, y), along axis 1 (columns, x)]
  const double gx0 = ftle_gradient(dX + col, (size_t)nx, j, ny), gx1 = ftle_gradient(dX + row, 1, i, nx);
  const double gy0 = ftle_gradient(dY + col, (size_t)nx, j, ny), gy1 = ftle_gradient(dY + row, 1, i, nx);
  const float J00 = (float)(gx0 / two_delta), J10 = (float)(gy0 / two_delta);
  const float J01 = (float)(gx1 / two_delta), J11 = (float)(gy1 / two_delta);
  // D = np.dot(np.transpose(J), J): D[r][s] = J[0][r] J[0][s] + J[1][r] J[1][s]
  const float a = J00 * J00 + J10 * J10;
  const float b = J00 * J01 + J10 * J11;
  const float c = J01 * J01 + J11 * J11;
  const double h = ((double)a - (double)c) / 2.0;
  const float lambda = (float)(((double)a + (double)c) / 2.0 + sqrt(h * h + (double)b * (double)b));
  if (lambda == 0.f) return -INFINITY;
  return (float)(log(sqrt((double)lambda)) / abs_T);
}

#ifndef ODR_FTLE_HOST
constexpr int FTLE_TILE_X = 64, FTLE_TILE_Y = 4;      // cells of one workgroup: a wave is 64 cells of one row

// One element per lane, flat: e = j * nx + i is the element seeded at (xs[i], ys[j]); 8 B read, 16 B written per element.
// A position that is not finite (an element that never existed) gives a NaN displacement.
__global__ __launch_bounds__(BLOCK) void k_ftle_displacement(DevProj P, const float *__restrict__ lon, const float *__restrict__ lat,
                                                             const double *__restrict__ xs, const double *__restrict__ ys, int nx,
                                                             long long n, double *__restrict__ dX, double *__restrict__ dY) {
  const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n) return;
  const double lo = (double)lon[e], la = (double)lat[e];
  double bx = NAN, by = NAN;
  if (isfinite(lo) && isfinite(la)) proj_fwd(P, lo, la, bx, by);
  const long long j = e / nx;
  dX[e] = bx - xs[e - j * nx];
  dY[e] = by - ys[j];
}

// One cell per lane, lanes along x: a wave reads 64 contiguous doubles of each of the rows j - 1, j, j + 1 of both planes (the rows
// above and below are shared with the neighbouring waves of the workgroup through the cache); 4 B written per cell.  The
// workgroups are numbered along x first (a flat grid: rows are not limited by the 65 535 of a grid's y dimension).
__global__ __launch_bounds__(FTLE_TILE_X * FTLE_TILE_Y) void k_ftle_cell(const double *__restrict__ dX, const double *__restrict__ dY,
                                                                         int nx, int ny, unsigned tiles_x, double two_delta, double abs_T,
                                                                         float *__restrict__ out) {
  const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const long long i = (long long)tx * FTLE_TILE_X + (threadIdx.x & (FTLE_TILE_X - 1));
  const long long j = (long long)ty * FTLE_TILE_Y + (threadIdx.x / FTLE_TILE_X);
  if (i >= nx || j >= ny) return;
  out[(size_t)j * (size_t)nx + (size_t)i] = ftle_cell(dX, dY, nx, ny, (int)i, (int)j, two_delta, abs_T);
}
#endif  // ODR_FTLE_HOST

}  // namespace odr
