// Reader operators on the device: sums of readers, a reader combined with a number, Gaussian blends towards point measurements.
//
//   Combine.__add__ / __mul__ / __truediv__ / __sub__         readers/operators/ops.py:14-50          the host flattens the expression
//   readerops.Combined.get_variables_interpolated             readers/operators/readerops.py:78-133   comb_add, comb_blend, comb_program
//   numops.Combined.get_variables_interpolated                readers/operators/numops.py:52-71       comb_num
//   combine_gaussian's gaussian_factor                        readers/operators/ops.py:52-96          comb_gauss_weight
//   the priority-list merge of get_environment                environment.py:597-762                  comb_take
//
// THE PROGRAM.  The host flattens the expression tree to postfix: a leaf pushes its value, COMB_ADD replaces the two topmost values by
// their sum, a Gaussian blend is its model operand followed by one COMB_GAUSS_TERM per measurement reader and a COMB_GAUSS_END, and a
// number-op works on the top value (it is the root: numops.Combined has no operators of its own).  The stack is three named values
// that are shifted by a push and a pop -- no indexed register array; the program is the same for every lane, so every branch on it is
// uniform.  Three values hold (a + b) + (c + d), any left-deep chain of any length, and what lies between; odr_combined_create
// refuses a program that would need a fourth.
//
// THE DTYPE CLASS.  The reference's operand arrays keep their NumPy dtype (float32: a 2-D block level, interpolated in time or not,
// of a reader that covers every position of the call; float64: everything else), and NumPy computes float32 + float32 in float32.
// A value here is a double with that class next to it; a float32-class value is always exactly a float.
//
// Every operation is rounded on its own (no fused multiply-add).  Everything above the device part is
// plain C++ and is compiled for the CPU by tests/combine_host.cpp (ODR_COMBINE_HOST).
#pragma once
#ifndef ODR_GEODINV_HOST
#ifndef ODR_GEODINV_NO_KERNELS
#define ODR_GEODINV_NO_KERNELS 1
#endif
#endif
#include "odr_geodinv.hip.h"

namespace odr {

enum { COMB_SOURCE = 0, COMB_UNIFORM = 1, COMB_ADD = 2, COMB_GAUSS_TERM = 3, COMB_GAUSS_END = 4, COMB_NUM_ADD = 5, COMB_NUM_MUL = 6,
       COMB_NUM_DIV = 7, COMB_NKINDS = 8 };
constexpr int COMB_MAXOPS = 32;      // of one program
constexpr int COMB_MAXUNI = 8;       // uniform leaves (timeseries readers) of one program
constexpr int COMB_MAXVARS = 8;      // variables of one launch
constexpr int COMB_STACK = 3;        // values a program may hold at once

// kind; index: the source id (COMB_SOURCE) or the uniform leaf (COMB_UNIFORM, COMB_GAUSS_TERM);
// d: the number (COMB_NUM_*), or the centre's longitude, latitude and the standard deviation in metres (COMB_GAUSS_TERM)
struct CombOp { int kind, index; double d[3]; };

struct CombVal { double v; bool f32; };
// (member by member: a struct copy would carry the padding bytes along, which keeps the value out of registers)
__host__ __device__ __forceinline__ void cb_copy(CombVal &d, const CombVal &s) { d.v = s.v; d.f32 = s.f32; }

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float cb_addf(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double cb_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double cb_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double cb_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double cb_div(double a, double b) { return __ddiv_rn(a, b); }
#else
inline float cb_addf(float a, float b) { return a + b; }
inline double cb_add(double a, double b) { return a + b; }
inline double cb_sub(double a, double b) { return a - b; }
inline double cb_mul(double a, double b) { return a * b; }
inline double cb_div(double a, double b) { return a / b; }
#endif

// a + b of two operand arrays (readerops.py:107): float32 when both are
__host__ __device__ __forceinline__ void comb_add(const CombVal &a, const CombVal &b, CombVal &r) {
  const bool f32 = a.f32 && b.f32;
  const double v = f32 ? (double)cb_addf((float)a.v, (float)b.v) : cb_add(a.v, b.v);
  r.v = v; r.f32 = f32;
}

// n + x, n * x, x / n with a python number n (numops.py:28-42): float64 whatever x's class is -- the operand is a
// np.ma.MaskedArray, whose arithmetic makes a 0-d float64 array of the number before NumPy's promotion sees it
__host__ __device__ __forceinline__ void comb_num(int kind, double n, CombVal &x) {
  x.v = kind == COMB_NUM_ADD ? cb_add(n, x.v) : kind == COMB_NUM_MUL ? cb_mul(n, x.v) : cb_div(x.v, n);
  x.f32 = false;
}

// exp(-(d / std)^2 / 2), d the WGS84 distance from the element to the centre (ops.py:92-94)
__host__ __device__ __forceinline__ double comb_gauss_weight(double lon, double lat, double lon_c, double lat_c, double std) {
  double s12, a1, a2;
  geod_inverse(lat, lon, lat_c, lon_c, s12, a1, a2);
  const double q = cb_div(s12, std);
  return exp(cb_div(-cb_mul(q, q), 2.0));
}

// a (1 - sum f) + sum b f (readerops.py:115,123): float64 whatever a's class is
__host__ __device__ __forceinline__ void comb_blend(CombVal &a, double fsum, double bfsum) {
  a.v = cb_add(cb_mul(a.v, cb_sub(1.0, fsum)), bfsum);
  a.f32 = false;
}

// The merge of one reader's value into the environment slot, as the mesh and polygon launches do it: a finite value replaces what
// is there when the reader heads the variable's list; elsewhere it fills only what is missing.
__host__ __device__ __forceinline__ bool comb_take(float val, float cur, int first) {
  return isfinite(val) && (first || !isfinite(cur));
}

// One program for NV variables that are sampled together (the kernel: one).  leaf(source id, val, f32):
// the values of the source at this element, NaN where it has none.  uni: [NV][COMB_MAXUNI] values of the uniform leaves.
// A program that odr_combined_create accepted never holds more than COMB_STACK values and ends with one.
template <int NV, class Leaf>
__host__ __device__ __forceinline__ void comb_program(const CombOp *ops, int n_ops, const double *uni, Leaf &leaf, double lon, double lat,
                                                      CombVal (&out)[NV]) {
  CombVal s0[NV], s1[NV], s2[NV];      // s0: the top
  double fsum = 0, bf[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    s0[v].v = s1[v].v = s2[v].v = NAN;
    s0[v].f32 = s1[v].f32 = s2[v].f32 = false;
    bf[v] = 0;
  }
  for (int k = 0; k < n_ops; ++k) {
    const CombOp &o = ops[k];
    if (o.kind == COMB_SOURCE || o.kind == COMB_UNIFORM) {
      double val[NV];
      bool f32[NV];
      if (o.kind == COMB_SOURCE) {
        leaf(o.index, val, f32);
      } else {
#pragma unroll
        for (int v = 0; v < NV; ++v) { val[v] = uni[v * COMB_MAXUNI + o.index]; f32[v] = false; }
      }
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        cb_copy(s2[v], s1[v]); cb_copy(s1[v], s0[v]);
        s0[v].v = val[v]; s0[v].f32 = f32[v];
      }
    } else if (o.kind == COMB_ADD) {
#pragma unroll
      for (int v = 0; v < NV; ++v) { comb_add(s1[v], s0[v], s0[v]); cb_copy(s1[v], s2[v]); }
    } else if (o.kind == COMB_GAUSS_TERM) {
      const double f = comb_gauss_weight(lon, lat, o.d[0], o.d[1], o.d[2]);
      fsum = cb_add(fsum, f);
#pragma unroll
      for (int v = 0; v < NV; ++v) bf[v] = cb_add(bf[v], cb_mul(uni[v * COMB_MAXUNI + o.index], f));
    } else if (o.kind == COMB_GAUSS_END) {
#pragma unroll
      for (int v = 0; v < NV; ++v) { comb_blend(s0[v], fsum, bf[v]); bf[v] = 0; }
      fsum = 0;
    } else {
#pragma unroll
      for (int v = 0; v < NV; ++v) comb_num(o.kind, o.d[0], s0[v]);
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) cb_copy(out[v], s0[v]);
}

// What odr_combined_create checks: the kinds, the stack discipline, that a blend's terms follow its model operand directly and that
// a number-op is the last operation.  Returns NULL or the reason.
inline const char *comb_check(const CombOp *ops, int n_ops, int n_sources) {
  if (n_ops < 1 || n_ops > COMB_MAXOPS) return "a program has 1 .. 32 operations";
  int depth = 0;
  bool in_blend = false;
  for (int k = 0; k < n_ops; ++k) {
    const CombOp &o = ops[k];
    if (o.kind < 0 || o.kind >= COMB_NKINDS) return "unknown kind of operation";
    if (in_blend && o.kind != COMB_GAUSS_TERM && o.kind != COMB_GAUSS_END) return "a Gaussian blend's terms are followed by its end";
    switch (o.kind) {
      case COMB_SOURCE:
        if (o.index < 0 || o.index >= n_sources) return "a source leaf names no source of the context";
        ++depth;
        break;
      case COMB_UNIFORM:
        if (o.index < 0 || o.index >= COMB_MAXUNI) return "a uniform leaf beyond the eight a program may have";
        ++depth;
        break;
      case COMB_ADD:
        if (depth < 2) return "a sum without two operands";
        --depth;
        break;
      case COMB_GAUSS_TERM:
        if (depth < 1) return "a Gaussian blend without its model operand";
        if (o.index < 0 || o.index >= COMB_MAXUNI) return "a measurement beyond the eight a program may have";
        if (!(std::isfinite(o.d[0]) && std::fabs(o.d[1]) <= 90 && o.d[2] > 0 && std::isfinite(o.d[2])))
          return "a Gaussian blend needs a finite centre and a standard deviation above zero";
        in_blend = true;
        break;
      case COMB_GAUSS_END:
        if (!in_blend) return "the end of a Gaussian blend without a term";
        in_blend = false;
        break;
      default:
        if (depth < 1) return "a number-op without its operand";
        if (k != n_ops - 1) return "a reader combined with a number is the root of its expression";
        if (!std::isfinite(o.d[0])) return "a number that is not finite";
    }
    if (depth > COMB_STACK) return "the expression needs more than two saved temporaries";
  }
  if (in_blend) return "a Gaussian blend without its end";
  if (depth != 1) return "the program leaves more than one value";
  return nullptr;
}

}  // namespace odr

#ifndef ODR_COMBINE_HOST
// ------------------------------------------------------------------------------------------------------------------ device part
namespace odr {

// The second half of source_sample() of odr_field.hip.h -- the values at a position that the front door (k_combined_front) has
// already brought into the reader's own coordinates and found covered -- with the dtype class of every value next to it (f32c:
// the reference's array is float32), and WITHOUT the rotation of vector pairs: readerops.Combined.get_variables_interpolated calls
// its operands without `rotate_to_proj` (readerops.py:84-101), so the reference adds the components of a projected grid along the
// grid's own axes, and a 2-D level stays float32.  One reader.get_variables_interpolated for one element (variables.py:860-920).
template <int NV>
__device__ __forceinline__ void source_values_cls(const DevSource &s, const int (&vars)[NV], double x, double y, double z, double t,
                                                  double (&val)[NV], bool (&f32c)[NV], int f32pos) {
#pragma unroll
  for (int v = 0; v < NV; ++v) f32c[v] = false;      // constant and analytic readers: value * np.ones(...), float64
  if (s.kind == SRC_CONSTANT) {
#pragma unroll
    for (int v = 0; v < NV; ++v) val[v] = s.const_val[vars[v]];
  } else if (s.kind == SRC_OSCILLATING) {
    const double phase = ((t - s.params[3]) / s.params[2]) * kPi;
    const double value = s.params[1] * sin(phase);
#pragma unroll
    for (int v = 0; v < NV; ++v) val[v] = value;
  } else if (s.kind == SRC_LANDMASK) {
    const double land = landmask_contains(s, x, y) ? 1.0 : 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) val[v] = vars[v] == VAR_LAND ? land : __builtin_nan("");
  } else if (s.kind == SRC_DOUBLE_GYRE) {
    const double A = s.params[0], eps = s.params[1], om = s.params[2], tt = t - s.params[3];
    const double sn = sin(om * tt);
    const double a = eps * sn, b = 1 - 2 * eps * sn;
    const double f = a * x * x + b * x, dfdx = 2 * a * x + b;
    double sf, cf, sy, cy;
    sincos(kPi * f, &sf, &cf);
    sincos(kPi * y, &sy, &cy);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (vars[v] == VAR_U) val[v] = -kPi * A * sf * cy;
      else if (vars[v] == VAR_V) val[v] = kPi * A * cf * sy * dfdx;
      else val[v] = 0.0;
    }
  } else {
    if (s.mod360_x) x = np_mod(x, 360.0);
    const int f32idx = (f32pos && s.proj.kind == PROJ_LATLONG) ? s.xy_f32 : 0;
    int ib, ia;
    bracket(s, t, ib, ia);
    bool all_static = true;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (vars[v] != VAR_LAND && vars[v] != VAR_DEPTH) all_static = false;
    if (all_static || s.always_valid) ia = -1;
    const DevBlock &bb = s.slot[ib];
    if (ia < 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) val[v] = block_value(bb, s, vars[v], x, y, z, f32c[v], 0, f32idx);
    } else {
      const DevBlock &ba = s.slot[ia];
      const double w = __ddiv_rn(t - bb.t, ba.t - bb.t);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        bool fb, fa;
        const double vb = block_value(bb, s, vars[v], x, y, z, fb, 0, f32idx);
        const double va = block_value(ba, s, vars[v], x, y, z, fa, 0, f32idx);
        f32c[v] = fb && fa;
        if (f32c[v]) val[v] = __fadd_rn(__fmul_rn((float)vb, (float)(1 - w)), __fmul_rn((float)va, (float)w));
        else val[v] = __dadd_rn(__dmul_rn(vb, 1 - w), __dmul_rn(va, w));
      }
    }
  }
}

// one call: the program, the uniform leaves' values and the variables
struct CombLaunch {
  int n_ops, n_vars;
  CombOp op[COMB_MAXOPS];
  double uni[COMB_MAXVARS * COMB_MAXUNI];      // [variable][uniform leaf]
  int var[COMB_MAXVARS], first[COMB_MAXVARS];
  float *out[COMB_MAXVARS];
};

// The leaves of one element.  xy: what k_combined_front left for it, [source leaf in program order][x, y][n]; x is NaN where the
// reader does not cover the element.  The leaves are asked for in program order: `slot` counts them.
struct CombLeaf {
  const DevWorld *W;
  const int *partial;      // [MAXSRC], written by k_combined_front
  const double *xy;
  long long n, i;
  int vars[1];
  double z, t;
  int f32pos, slot;
  __device__ __forceinline__ void operator()(int sid, double (&val)[1], bool (&f32)[1]) {
    const double x = xy[(size_t)(2 * slot) * (size_t)n + (size_t)i], y = xy[(size_t)(2 * slot + 1) * (size_t)n + (size_t)i];
    ++slot;
    f32[0] = false;
    val[0] = __builtin_nan("");
    if (x == x) source_values_cls<1>(W->src[sid], vars, x, y, z, t, val, f32, f32pos);
    // A reader that does not cover EVERY position of the call hands its values out in a masked float64 array
    // (np.ma.masked_all, variables.py:840-858): its float32 values widen, and the operations on them are float64 operations.
    if (partial[sid]) f32[0] = false;
  }
};

// The reader front door, once per source leaf and element whatever the number of variables (variables.py:860-914: the time
// coverage, modulate_longitude, lonlat2xy, covers_positions_xy): the position in the reader's own coordinates goes to xy
// ([source leaf in program order][x, y][n]; x = NaN: not covered), and partial[sid] = 1 when source `sid` does not cover some
// element of the set -- decided over the whole call before a value is formed, as the reference decides the dtype of a reader's
// arrays.  One element per lane.
__global__ __launch_bounds__(BLOCK) void k_combined_front(const DevWorld *__restrict__ W, CombLaunch L, long long n,
                                                          const double *__restrict__ lon, const double *__restrict__ lat,
                                                          const double *__restrict__ z, double t, int *__restrict__ partial,
                                                          double *__restrict__ xy) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double lo = lon[i], la = lat[i], zz = z[i];
  int slot = 0;
  for (int k = 0; k < L.n_ops; ++k) {
    if (L.op[k].kind != COMB_SOURCE) continue;
    const DevSource &s = W->src[L.op[k].index];
    double x, y;
    const bool covered = (s.always_valid || (t >= s.tmin && t <= s.tmax)) && source_covers_xyz(s, lo, la, zz, x, y, W->f32pos & 1);
    if (!covered) partial[L.op[k].index] = 1;      // (every writer stores the same value)
    xy[(size_t)(2 * slot) * (size_t)n + (size_t)i] = covered ? x : __builtin_nan("");
    xy[(size_t)(2 * slot + 1) * (size_t)n + (size_t)i] = y;
    ++slot;
  }
}

// Combined.get_variables_interpolated + the priority-list merge for every element of the set, ONE launch behind the front door;
// one element per lane, one variable after the other (the operands are not rotated, so the components of a vector pair do not
// meet): the leaves' values at the positions of k_combined_front, the program, the float32 cast, the merge.
__global__ __launch_bounds__(BLOCK, 2) void k_combined_sample(const DevWorld *__restrict__ W, CombLaunch L, long long n,
                                                              const double *__restrict__ lon, const double *__restrict__ lat,
                                                              const double *__restrict__ z, double t, const int *__restrict__ partial,
                                                              const double *__restrict__ xy) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  CombLeaf leaf;
  leaf.W = W;
  leaf.partial = partial;
  leaf.xy = xy; leaf.n = n; leaf.i = i;
  leaf.z = z[i]; leaf.t = t;
  leaf.f32pos = W->f32pos & 1;      // (the main-loop call of a run's first step: DevWorld::f32pos)
  const double lo = lon[i], la = lat[i];      // (the Gaussian weights take the element's own longitude and latitude)
  for (int k = 0; k < L.n_vars; ++k) {
    leaf.vars[0] = L.var[k];
    leaf.slot = 0;
    CombVal res[1];
    comb_program<1>(L.op, L.n_ops, L.uni + k * COMB_MAXUNI, leaf, lo, la, res);
    float *o = L.out[k];
    const float val = (float)res[0].v;      // environment.py:695
    if (comb_take(val, o[i], L.first[k])) o[i] = L.var[k] == VAR_TEMP ? kelvin_to_celsius(val) : val;
  }
}

}  // namespace odr
#endif  // !ODR_COMBINE_HOST
