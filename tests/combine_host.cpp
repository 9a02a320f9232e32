// TEST INFRASTRUCTURE: the evaluator of opendrift_amd/csrc/odr_combine.hip.h (the device code of the reader operators) compiled for
// the CPU with g++ -ffp-contract=off, so that it can be compared with NumPy and the reference's answers without a GPU
// (tests/test_reader_ops_device_arithmetic.py).  tests/hostshim stands in for <hip/hip_runtime.h>; the device part is excluded by
// ODR_COMBINE_HOST.  A leaf is a row of `values` with its dtype class; the loop does what the kernel does with one element.
#include <hip/hip_runtime.h>

#include <cstring>

#define ODR_GEODINV_HOST 1
#define ODR_COMBINE_HOST 1
#include "../opendrift_amd/csrc/odr_combine.hip.h"

namespace {
struct HostLeaf {
  const double *values;      // [leaf][n]
  const unsigned char *f32;  // [leaf]
  long long n, i;
  void operator()(int leaf, double (&val)[1], bool (&cls)[1]) const {
    val[0] = values[(long long)leaf * n + i];
    cls[0] = f32[leaf] != 0;
  }
};
}  // namespace

// ops: n_ops x (kind, index, d0, d1, d2) as doubles.  Returns 0, or -1 with `why` when the program is refused.
extern "C" int combh_run(int n_ops, const double *ops, int n_leaves, long long n, const double *values, const unsigned char *f32,
                         const double *uniform, const double *lon, const double *lat, double *out, unsigned char *out_f32, char *why) {
  odr::CombOp op[odr::COMB_MAXOPS];
  if (n_ops > odr::COMB_MAXOPS) { std::strcpy(why, "a program has 1 .. 32 operations"); return -1; }
  for (int k = 0; k < n_ops; ++k) {
    op[k].kind = (int)ops[5 * k];
    op[k].index = (int)ops[5 * k + 1];
    for (int j = 0; j < 3; ++j) op[k].d[j] = ops[5 * k + 2 + j];
  }
  if (const char *e = odr::comb_check(op, n_ops, n_leaves)) { std::strncpy(why, e, 127); why[127] = 0; return -1; }
  HostLeaf leaf{values, f32, n, 0};
  for (long long i = 0; i < n; ++i) {
    leaf.i = i;
    odr::CombVal res[1];
    odr::comb_program<1>(op, n_ops, uniform, leaf, lon[i], lat[i], res);
    out[i] = res[0].v;
    out_f32[i] = res[0].f32 ? 1 : 0;
  }
  return 0;
}

extern "C" void combh_gauss_weight(long long n, const double *lon, const double *lat, double lon_c, double lat_c, double std, double *f,
                                   double *distance) {
  for (long long i = 0; i < n; ++i) {
    f[i] = odr::comb_gauss_weight(lon[i], lat[i], lon_c, lat_c, std);
    double a1, a2;
    odr::geod_inverse(lat[i], lon[i], lat_c, lon_c, distance[i], a1, a2);
  }
}

extern "C" void combh_take(long long n, const float *val, const float *cur, int first, unsigned char *take) {
  for (long long i = 0; i < n; ++i) take[i] = odr::comb_take(val[i], cur[i], first) ? 1 : 0;
}
