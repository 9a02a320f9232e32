// RadionuclideDrift: every element carries a discrete species that changes stochastically from a transfer-rate matrix; a
// change of species can put the element on the sea bed or take it off, and redraws its diameter.
//
//   RadionuclideDrift.update_transfer_rates     models/radionuclides.py:728-756        radio_probabilities
//   RadionuclideDrift.update_speciation         models/radionuclides.py:760-810        radio_target, radio_apply
//   RadionuclideDrift.update_radionuclide_diameter  :866-902, set_init_diameter :281-315   radio_becomes_particle /
//                                                                                      radio_becomes_dissolved / radio_new_diameter
//   RadionuclideDrift.sorption_to_sediments     :814-830,  desorption_from_sediments :834-860   radio_apply
//   RadionuclideDrift.update_terminal_velocity  :665-721 (no profiles)                 radio_terminal_velocity_f32
//   RadionuclideDrift.bottom_interaction        :912-942                               radio_settle_species (+ the sea-floor
//                                               action ODR_SEAFLOOR_SETTLE_SPECIES inside the mixing kernels, odr_kernels.hip.h)
//   RadionuclideDrift.resuspension              :946-997                               radio_resuspend
//
// Rounding contract.  The transfer rates are float64.  LMM -> particle reversible is rate * conc3 / 1e-3 with the float32 conc3
// promoted: two IEEE double operations.  The distance to the sea bed is z - Zmin with Zmin = -1.*depth (float32) promoted: one
// double subtraction.  p = 1 - exp(-k dt): the exponential is the platform's (NumPy's, libm's and the device's agree to an ulp,
// not bit for bit); a zero rate is skipped (1 - exp(-0) is exactly 0).  psum adds p in species order (np.sum over fewer than eight
// contiguous values is the plain loop), the cumulative sum adds p / psum in species order, the target is the number of cumulative
// values below u2 (np.searchsorted, side left).  Rounding can leave every cumulative value below u2: the reference then stores
// the species number `nspecies` and fails on it in the next step; here the target is the last species with p > 0.
// Zmin + resuspension_depth and -depth + desorption_depth are float32 additions (NumPy 2: a float32 array and a Python float)
// stored into the float64 z, the noise is added to that in float64.  The new diameter is float64 (diameter + noise, or
// diameter * noise) rounded once to float32.  Terminal velocity: the float32 chain of the egg model's Stokes branch with the
// element's own density; W * moving is exact.
//
// Compiled for the CPU by tests/radio_host.cpp (the rounding intrinsics are its own there): includes nothing but the sea-water
// chains.
#pragma once
#include "odr_seawater.hip.h"

namespace odr {

constexpr int RADIO_MAXSP = 7, RADIO_MAXSAL = 4, RADIO_NBINS = RADIO_MAXSP * RADIO_MAXSP;

// the model's configuration without the rate table (a launch argument; the table is read through a pointer: LDS on the device)
struct RadioSetup {
  double dt, layer_thick, dia_part, dia_diss, dia_uncert, desorb_std, resusp_std;
  float desorb_depth, resusp_depth, critvel;
  int nspecies, nsal, lognormal;
  // species numbers, -1 where the setup has none
  int lmm, lmmcation, lmmanion, polymer, prev, srev, psrev, ssrev, pirrev, sirrev;
};

// np.searchsorted([0, 1, 10, 20], S) - 1, the index -1 (S <= 0, and NaN sorts last: 4 - 1) taken from the end as NumPy does
__device__ __forceinline__ int radio_salinity_interval(float S) {
  if (S != S) return 3;
  const int k = (0.f < S ? 1 : 0) + (1.f < S ? 1 : 0) + (10.f < S ? 1 : 0) + (20.f < S ? 1 : 0) - 1;
  return k < 0 ? 3 : k;
}

// p[j] = 1 - exp(-k_j dt) of the element's row (radionuclides.py:728-756, :771-772); returns psum.  table: [nsal][7][7]
__device__ __forceinline__ double radio_probabilities(const RadioSetup &S, const double *table, int specie, float sal, float depth,
                                                      float conc3, double z, double (&p)[RADIO_MAXSP]) {
  const int sali = S.nsal > 1 ? radio_salinity_interval(sal) : 0;
  const double *row = table + (sali * RADIO_MAXSP + specie) * RADIO_MAXSP;
  const bool lmm = S.lmm >= 0 && specie == S.lmm;
  // an LMM element further than layer_thick above the sea bed has no rate to the sediment (:735-742)
  const bool far = lmm && __dsub_rn(z, (double)__fmul_rn(-1.f, depth)) > S.layer_thick;
  double psum = 0.0;
#pragma unroll
  for (int j = 0; j < RADIO_MAXSP; ++j) {
    double k = row[j];
    if (far && j == S.srev) k = 0.0;
    if (lmm && j == S.prev) k = __ddiv_rn(__dmul_rn(k, (double)conc3), 1.e-3);   // scaled by the suspended matter at the element (:744-750)
    p[j] = k == 0.0 ? 0.0 : __dsub_rn(1.0, exp(__dmul_rn(-k, S.dt)));
    psum = __dadd_rn(psum, p[j]);
  }
  return psum;
}

// np.searchsorted(np.cumsum(p / psum), u2) (:789), clamped to the last species with p > 0 (see the rounding contract)
__device__ __forceinline__ int radio_target(const double (&p)[RADIO_MAXSP], double psum, double u2, int nspecies) {
  double c = 0.0;
  int below = 0, last = 0;
#pragma unroll
  for (int j = 0; j < RADIO_MAXSP; ++j) {
    if (j < nspecies) {
      c = j == 0 ? __ddiv_rn(p[0], psum) : __dadd_rn(c, __ddiv_rn(p[j], psum));
      below += c < u2 ? 1 : 0;
      if (p[j] > 0.0) last = j;
    }
  }
  return below < nspecies ? below : last;
}

// update_radionuclide_diameter (:875-880): the element becomes a particle
__device__ __forceinline__ bool radio_becomes_particle(const RadioSetup &S, int in, int out) {
  if (out == S.prev && in != S.prev) return true;
  if (S.psrev >= 0 && out == S.psrev && in == S.ssrev) return true;
  if (S.pirrev >= 0 && out == S.pirrev && in == S.sirrev) return true;
  return false;
}
// (:888-899): the element becomes dissolved.  'Humic colloid' is NOT among them: the reference tests the name 'Humic_colloid',
// which no setup has (and 'Colloid', which none has either)
__device__ __forceinline__ bool radio_becomes_dissolved(const RadioSetup &S, int in, int out) {
  if (in == out) return false;
  if (S.lmm >= 0) return out == S.lmm;
  return out == S.lmmcation || out == S.lmmanion || out == S.polymer;
}

// set_init_diameter (:281-315) for one element.  noise_is_final: `noise` is the value the reference drew (normal(0, uncert) or
// lognormal(0, 3 uncert / diam)); else it is a standard normal and is scaled here.  A diameter of 0 has no noise; the clipping
// to the minimum and maximum diameter assigns into a copy in the reference (:311-312) and does nothing
__device__ __forceinline__ float radio_new_diameter(const RadioSetup &S, double diam, double noise, bool noise_is_final) {
  if (!(diam > 0)) return (float)diam;     // uncert = uncert_ln = 0: normal(0, 0) is 0, lognormal(0, 0) is 1
  const double uncert = S.dia_uncert;
  const double uncert_ln = __dmul_rn(__ddiv_rn(uncert, diam), 3.);
  double t = noise;
  if (!noise_is_final) t = S.lognormal ? exp(__dmul_rn(uncert_ln, noise)) : __dmul_rn(uncert, noise);
  return (float)(S.lognormal ? __dmul_rn(diam, t) : __dadd_rn(diam, t));
}

// the standard normal of the depth noise scaled like np.random.normal(0, std)
__device__ __forceinline__ double radio_depth_noise(double std, double noise, bool noise_is_final) {
  return noise_is_final ? noise : __dmul_rn(std, noise);
}

// what a change of species in -> out does to the element (:808-810): diameter, sorption (z = -depth, moving = 0), desorption
// (z = -depth + desorption_depth + N(0, std), moving = 1).  z > 0 -> 0 is the caller's (it holds for every element)
__device__ __forceinline__ void radio_apply(const RadioSetup &S, int in, int out, float depth, double diam_noise, double depth_noise,
                                            bool noise_is_final, int &moving, double &z, float &diameter) {
  if (radio_becomes_particle(S, in, out)) diameter = radio_new_diameter(S, S.dia_part, diam_noise, noise_is_final);
  else if (radio_becomes_dissolved(S, in, out)) diameter = radio_new_diameter(S, S.dia_diss, diam_noise, noise_is_final);
  const int diss = S.lmm >= 0 ? S.lmm : S.lmmcation;
  if (out == S.srev && in == diss) {          // sorption_to_sediments (:814-830)
    z = (double)__fmul_rn(-1.f, depth);
    moving = 0;
  } else if (out == diss && in == S.srev) {   // desorption_from_sediments (:834-860)
    z = (double)__fadd_rn(__fmul_rn(-1.f, depth), S.desorb_depth);
    moving = 1;
    if (S.desorb_std > 0) z = __dadd_rn(z, radio_depth_noise(S.desorb_std, depth_noise, noise_is_final));
  }
}

// update_terminal_velocity without profiles (:665-721): Stokes' law with the element's density, times moving
__device__ __forceinline__ float radio_terminal_velocity_f32(float T, float Sal, float d, float density, int moving) {
  const float dr = __fsub_rn(oil_sea_water_density_f32(T, Sal), density);   // DENSw - DENSpart
  const float mu = oil_water_viscosity_f32(T, Sal);
  // W = (1.0/my_w)*(1.0/18.0)*g*partsize**2 * dr                      (left to right)
  float W = __fmul_rn(__fdiv_rn(1.0f, mu), (float)(1.0 / 18.0));
  W = __fmul_rn(W, (float)9.81);
  W = __fmul_rn(W, __fmul_rn(d, d));
  W = __fmul_rn(W, dr);
  return __fmul_rn(W, (float)moving);     // (float32 * int32 is a float64 product in NumPy: exact, W or a zero of W's sign)
}

// bottom_interaction (:912-942) for an element the sea-floor action has settled (moving == 0): the sediment species of a
// particle species, else -1
__device__ __forceinline__ int radio_settle_species(const RadioSetup &S, int specie) {
  if (specie == S.prev) return S.srev;
  if (S.psrev >= 0 && specie == S.psrev) return S.ssrev;
  if (S.pirrev >= 0 && specie == S.pirrev) return S.sirrev;
  return -1;
}

// np.sqrt(x_vel*x_vel + y_vel*y_vel) on the float32 environment (:968)
__device__ __forceinline__ float radio_current_speed_f32(float u, float v) {
  return sqrtf(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)));   // IEEE sqrt (-O3 without fast-math: correctly rounded)
}

// resuspension (:946-997) of one element that lies on the sea bed where the current is fast enough (the caller's two tests):
// moving, z, and the matching particle species of a sediment species with its new diameter.  Returns true
__device__ __forceinline__ bool radio_resuspend(const RadioSetup &S, float depth, double diam_noise, double depth_noise,
                                                bool noise_is_final, int &specie, int &moving, double &z, float &diameter) {
  const float Zmin = __fmul_rn(-1.f, depth);
  moving = 1;
  z = (double)__fadd_rn(Zmin, S.resusp_depth);
  if (S.resusp_std > 0) z = __dadd_rn(z, radio_depth_noise(S.resusp_std, depth_noise, noise_is_final));
  const int in = specie;
  if (in == S.srev) specie = S.prev;
  else if (S.psrev >= 0 && in == S.ssrev) specie = S.psrev;
  else if (S.pirrev >= 0 && in == S.sirrev) specie = S.pirrev;
  if (radio_becomes_particle(S, in, specie)) diameter = radio_new_diameter(S, S.dia_part, diam_noise, noise_is_final);
  return true;
}

// the element arrays of a launch (the device's active set; tests/radio_host.cpp hands in host arrays of the same layout)
struct RadioView {
  float *specie, *diameter;
  int *moving;
  double *z;
  const float *sal, *depth, *conc3, *u, *v;
};
constexpr int RADIO_BAD_SPECIES = RADIO_NBINS;   // the counter bin of elements whose species number is outside the table

// update_transfer_rates + update_speciation for element i.  draws(which): 0 u1, 1 u2, 2 diameter noise, 3 depth noise, asked for
// only when needed (u2 and the noises of an element that transforms); noise_is_final: see radio_new_diameter.  Reads specie, z,
// depth and what the row needs of salinity and conc3; writes, for an element that changes only, specie, diameter, moving, z.
// Returns the counter bin in * 7 + out of the transformation, -1 without one, RADIO_BAD_SPECIES (nothing is touched)
template <class DRAWS>
__device__ __forceinline__ int radio_speciate_at(const RadioSetup &S, const double *table, const RadioView &V, long long i,
                                                 bool noise_is_final, DRAWS &&draws) {
  const int in = (int)V.specie[i];
  if (in < 0 || in >= S.nspecies) return RADIO_BAD_SPECIES;
  double zz = V.z[i];
  const float dep = V.depth[i];
  double p[RADIO_MAXSP];
  const double psum = radio_probabilities(S, table, in, S.nsal > 1 ? V.sal[i] : 0.f, dep, S.lmm >= 0 && in == S.lmm ? V.conc3[i] : 0.f, zz, p);
  if (!(draws(0) < psum)) {
    if (zz > 0) V.z[i] = 0.0;     // nothing stays above the surface (:828-830)
    return -1;
  }
  const int out = radio_target(p, psum, draws(1), S.nspecies);
  int m = V.moving[i];
  const int m0 = m;
  const double z0 = zz;
  float d = V.diameter[i];
  const float d0 = d;
  radio_apply(S, in, out, dep, draws(2), draws(3), noise_is_final, m, zz, d);
  if (zz > 0) zz = 0.0;
  if (out != in) V.specie[i] = (float)out;
  if (d != d0) V.diameter[i] = d;
  if (m != m0) V.moving[i] = m;
  if (zz != z0) V.z[i] = zz;
  return in * RADIO_MAXSP + out;
}

// bottom_interaction's change of species and resuspension for element i.  draws(which): 2 diameter noise, 3 depth noise.
// bins: the counter bins of the (at most two) changes of species, -1 for none.  Returns false for a species outside the table
template <class DRAWS>
__device__ __forceinline__ bool radio_resuspend_at(const RadioSetup &S, const RadioView &V, long long i, bool noise_is_final,
                                                   DRAWS &&draws, int (&bins)[2]) {
  bins[0] = bins[1] = -1;
  const int sp0 = (int)V.specie[i];
  if (sp0 < 0 || sp0 >= S.nspecies) return false;
  int sp = sp0, m = V.moving[i];
  const int m0 = m;
  // the species change of the settling: the sea-floor action of the mixing launch has set moving = 0 (bottom_interaction)
  if (m == 0) {
    const int sed = radio_settle_species(S, sp);
    if (sed >= 0) { bins[0] = sp * RADIO_MAXSP + sed; sp = sed; }
  }
  double zz = V.z[i];
  const double z0 = zz;
  const float dep = V.depth[i];
  if (zz <= (double)__fmul_rn(-1.f, dep)) {     // (an element above the sea bed reads no more)
    float d = V.diameter[i];
    const float d0 = d;
    const int from = sp;
    const float u = V.u[i], v = V.v[i];
    if (radio_current_speed_f32(u, v) >= S.critvel && radio_resuspend(S, dep, draws(2), draws(3), noise_is_final, sp, m, zz, d)) {
      if (sp != from) bins[1] = from * RADIO_MAXSP + sp;
      if (d != d0) V.diameter[i] = d;
    }
  }
  if (zz > 0) zz = 0.0;     // nothing stays above the surface (:980-983)
  if (sp != sp0) V.specie[i] = (float)sp;
  if (m != m0) V.moving[i] = m;
  if (zz != z0) V.z[i] = zz;
  return true;
}

#ifndef ODR_RADIO_HOST
// Philox offsets within a step: the speciation's uniforms (u1, u2) and normals (diameter, depth), the resuspension's normals
constexpr unsigned long long RNG_OFF_RADIO = 7000, RNG_OFF_RADIO_NORMAL = 7004, RNG_OFF_RADIO_RESUSPEND = 7008;

// the per-workgroup histogram of transformations -> one atomicAdd per non-empty bin (bin RADIO_NBINS: species outside the table)
__device__ __forceinline__ void radio_flush(const unsigned *hist, unsigned long long *counts) {
  __syncthreads();
  if (threadIdx.x <= RADIO_NBINS) {
    const unsigned h = hist[threadIdx.x];
    if (h) atomicAdd(counts + threadIdx.x, (unsigned long long)h);
  }
}

struct RadioDraws { const double *u1, *u2, *diam, *depth; };   // ODR_RNG_HOST: one number per element and distribution

// the element's draws: the caller's (ODR_RNG_HOST) or two Philox blocks of the stream (seed, ID, step), each evaluated when first
// asked for -- off_uniform: the block of u1 and u2, off_normal: the block of the two normals
struct RadioRng {
  const RadioDraws &H;
  long long i;
  int rng_mode, id;
  unsigned long long seed, step, off_uniform, off_normal;
  uint4 b;
  double2 g;
  bool have_b, have_g;
  __device__ __forceinline__ double operator()(int which) {
    if (rng_mode == 1) return which == 0 ? H.u1[i] : which == 1 ? H.u2[i] : which == 2 ? H.diam[i] : H.depth[i];
    if (which < 2) {
      if (!have_b) { b = rng_block(seed, id, step, off_uniform); have_b = true; }
      return which == 0 ? rng_u53(b.x, b.y) : rng_u53(b.z, b.w);
    }
    if (!have_g) { g = rng_normal2(rng_block(seed, id, step, off_normal)); have_g = true; }
    return which == 2 ? g.x : g.y;
  }
};

// one element per thread.  In: specie, z, depth, salinity / conc3 as the row needs them (<= 24 B); out, for the elements that
// change only: specie, diameter, z, moving.  The rate table (1568 B) is staged in LDS once per workgroup
__global__ __launch_bounds__(256) void k_radio_speciation(long long n, RadioSetup S, const double *__restrict__ table_dev, RadioView V,
                                                          const int *__restrict__ id, int rng_mode, RadioDraws H,
                                                          unsigned long long seed, unsigned long long step,
                                                          unsigned long long *__restrict__ counts) {
  __shared__ double table[RADIO_MAXSAL * RADIO_NBINS];
  __shared__ unsigned hist[RADIO_NBINS + 1];
  const int tid = threadIdx.x;
  if (tid < RADIO_MAXSAL * RADIO_NBINS) table[tid] = table_dev[tid];
  if (tid <= RADIO_NBINS) hist[tid] = 0u;
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + tid;
  if (i < n) {
    RadioRng R = {H, i, rng_mode, rng_mode == 1 ? 0 : id[i], seed, step, RNG_OFF_RADIO, RNG_OFF_RADIO_NORMAL, make_uint4(0u, 0u, 0u, 0u), make_double2(0., 0.), false, false};
    const int bin = radio_speciate_at(S, table, V, i, rng_mode == 1, R);
    if (bin >= 0) atomicAdd(&hist[bin], 1u);
  }
  radio_flush(hist, counts);
}

// one element per thread: T, S, diameter, density, moving in, the terminal velocity out (24 B per element, coalesced)
__global__ __launch_bounds__(256) void k_radio_terminal_velocity(long long n, const float *__restrict__ T, const float *__restrict__ Sal,
                                                                 const float *__restrict__ diameter, const float *__restrict__ density,
                                                                 const int *__restrict__ moving, float *__restrict__ terminal_velocity) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  terminal_velocity[i] = radio_terminal_velocity_f32(T[i], Sal[i], diameter[i], density[i], moving[i]);
}

// one element per thread: specie, moving, z, depth in (20 B), u, v and the diameter for the elements on the sea bed; out, for the
// elements that change only: specie, moving, z, diameter
__global__ __launch_bounds__(256) void k_radio_resuspend(long long n, RadioSetup S, RadioView V, const int *__restrict__ id, int rng_mode,
                                                         RadioDraws H, unsigned long long seed, unsigned long long step,
                                                         unsigned long long *__restrict__ counts) {
  __shared__ unsigned hist[RADIO_NBINS + 1];
  const int tid = threadIdx.x;
  if (tid <= RADIO_NBINS) hist[tid] = 0u;
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + tid;
  if (i < n) {
    RadioRng R = {H, i, rng_mode, rng_mode == 1 ? 0 : id[i], seed, step, RNG_OFF_RADIO_RESUSPEND, RNG_OFF_RADIO_RESUSPEND, make_uint4(0u, 0u, 0u, 0u), make_double2(0., 0.), false, false};
    int bins[2];
    if (!radio_resuspend_at(S, V, i, rng_mode == 1, R, bins)) atomicAdd(&hist[RADIO_BAD_SPECIES], 1u);
    if (bins[0] >= 0) atomicAdd(&hist[bins[0]], 1u);
    if (bins[1] >= 0) atomicAdd(&hist[bins[1]], 1u);
  }
  radio_flush(hist, counts);
}
#endif  // ODR_RADIO_HOST

}  // namespace odr
