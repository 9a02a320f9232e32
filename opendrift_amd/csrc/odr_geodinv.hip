// libodrift_hip.so, a translation unit of its own: the WGS84 inverse geodesic and the trajectory lengths of a finished run
// (OpenDriftSimulation.get_trajectory_lengths, models/basemodel/__init__.py:4614-4628).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_geodinv.hip.h"

namespace {

constexpr size_t TRAJ_SLAB_BYTES = 256u << 20;         // lon and lat of one slab of trajectories (ODR_TRAJ_SLAB_BYTES overrides)
constexpr long long TRAJ_LAUNCH_ENTRIES = 1ll << 30;   // positions of one launch
constexpr long long INVERSE_CHUNK = 1ll << 20;         // pairs of one odr_geod_inverse launch

// nrows contiguous device rows of rowlen doubles -> host rows dst_pitch doubles apart, several rows per trip through the bounce buffer
int rows_out(odr_ctx *c, double *dst, size_t dst_pitch, const double *dev, size_t nrows, size_t rowlen) {
  const size_t cap = ODR_BOUNCE_BYTES / sizeof(double);
  if (rowlen > cap) {
    for (size_t r = 0; r < nrows; ++r) D2H(dst + r * dst_pitch, dev + r * rowlen, sizeof(double) * rowlen);
    return 0;
  }
  void *b;
  if (int rc = odr_i_bounce(c, 0, &b)) return rc;
  const size_t per_trip = cap / rowlen;
  for (size_t r = 0; r < nrows; r += per_trip) {
    const size_t m = std::min(per_trip, nrows - r);
    HIPCHK(hipMemcpyAsync(b, dev + r * rowlen, sizeof(double) * m * rowlen, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < m; ++k) memcpy(dst + (r + k) * dst_pitch, (const double *)b + k * rowlen, sizeof(double) * rowlen);
  }
  return 0;
}

}  // namespace

// pyproj.Geod(ellps='WGS84').inv as get_trajectory_lengths calls it (models/basemodel/__init__.py:4618-4620), n pairs: host float64
// in and out, forward azimuths at both ends.  Synchronous.
int odr_geod_inverse(odr_ctx *c, int64_t n, const double *lon1, const double *lat1, const double *lon2, const double *lat2, double *azi1,
                     double *azi2, double *s12) {
  REQUIRE(c && lon1 && lat1 && lon2 && lat2, "NULL argument");
  REQUIRE(n >= 0, "negative size");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  const long long chunk = std::min<long long>(n, INVERSE_CHUNK);
  double *d[7];
  for (int k = 0; k < 7; ++k) if (int rc = B.alloc((void **)&d[k], sizeof(double) * (size_t)chunk)) return rc;
  const double *in[4] = {lon1, lat1, lon2, lat2};
  double *out[3] = {azi1, azi2, s12};
  for (long long o = 0; o < n; o += chunk) {
    const long long m = std::min(chunk, n - o);
    for (int k = 0; k < 4; ++k) H2D(d[k], in[k] + o, sizeof(double) * (size_t)m);
    hipLaunchKernelGGL(k_geod_inverse, dim3(nblk(m)), dim3(BLOCK), 0, c->stream, m, d[0], d[1], d[2], d[3], d[4], d[5], d[6]);
    HIPCHK(hipGetLastError());
    for (int k = 0; k < 3; ++k) if (out[k]) D2H(out[k] + o, d[4 + k], sizeof(double) * (size_t)m);
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// get_trajectory_lengths (models/basemodel/__init__.py:4614-4628).  Slabs of whole trajectories: their positions go up (host inputs)
// or are used in place (device inputs), k_traj_segments writes the slab's distances [interval][trajectory] (and speeds) into device
// scratch, k_traj_totals sums them in time order, and what the caller asked for comes back.  Synchronous.
int odr_trajectory_lengths(odr_ctx *c, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, double dt_seconds,
                           double *total_length, double *distances, double *speeds) {
  REQUIRE(c && lon && lat && total_length, "NULL argument");
  REQUIRE(n_trajectories >= 0, "negative size");
  REQUIRE(n_times >= 2, "%d output times: a trajectory length needs two", n_times);
  REQUIRE(std::isfinite(dt_seconds) && dt_seconds != 0, "time step %g s", dt_seconds);
  size_t budget = TRAJ_SLAB_BYTES;
  if (const char *s = getenv("ODR_TRAJ_SLAB_BYTES")) {
    const long long v = atoll(s);
    REQUIRE(v > 0, "ODR_TRAJ_SLAB_BYTES=%s", s);
    budget = (size_t)v;
  }
  KernelClock &clock = c->clock[CLOCK_TRAJ_LENGTHS];
  clock.reset();
  if (n_trajectories == 0) return 0;

  HIPCHK(hipSetDevice(c->device));
  const bool dev[2] = {odr_i_on_device(lon), odr_i_on_device(lat)};
  const int n_seg = n_times - 1;
  const size_t row = 2 * sizeof(float) * (size_t)n_times;
  long long slab_traj = std::max<long long>(1, (long long)(budget / row));
  slab_traj = std::min<long long>(slab_traj, std::max<long long>(1, TRAJ_LAUNCH_ENTRIES / n_times));
  slab_traj = std::min<long long>(slab_traj, n_trajectories);
  const size_t slab_floats = (size_t)slab_traj * (size_t)n_times, slab_seg = (size_t)slab_traj * (size_t)n_seg;

  DevScope B;      // released on every way out
  float *up[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) if (!dev[k]) if (int rc = B.alloc((void **)&up[k], sizeof(float) * slab_floats)) return rc;
  double *d_dist, *d_speed = nullptr, *d_total;
  if (int rc = B.alloc((void **)&d_dist, sizeof(double) * slab_seg)) return rc;
  if (speeds) if (int rc = B.alloc((void **)&d_speed, sizeof(double) * slab_seg)) return rc;
  if (int rc = B.alloc((void **)&d_total, sizeof(double) * (size_t)slab_traj)) return rc;

  const float *in[2] = {lon, lat};
  const unsigned tiles_t = (unsigned)((n_seg + TRAJ_TILE - 1) / TRAJ_TILE);
  for (long long r0 = 0; r0 < n_trajectories; r0 += slab_traj) {
    const long long nr = std::min(slab_traj, n_trajectories - r0);
    const size_t off = (size_t)r0 * (size_t)n_times;
    const float *ptr[2];
    for (int k = 0; k < 2; ++k) {
      if (dev[k]) { ptr[k] = in[k] + off; continue; }
      H2D(up[k], in[k] + off, sizeof(float) * (size_t)nr * (size_t)n_times);      // waits for the stream: the slab before is done with up[k]
      ptr[k] = up[k];
    }
    const unsigned tiles_traj = (unsigned)((nr + TRAJ_TILE - 1) / TRAJ_TILE);
    if (int rc = clock.start(c->stream)) return rc;
    hipLaunchKernelGGL(k_traj_segments, dim3(tiles_traj * tiles_t), dim3(BLOCK), 0, c->stream, ptr[0], ptr[1], nr, (int)n_times, tiles_traj,
                       dt_seconds, nr, d_dist, d_speed);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_traj_totals, dim3(nblk(nr)), dim3(BLOCK), 0, c->stream, (const double *)d_dist, nr, n_seg, nr, d_total);
    HIPCHK(hipGetLastError());
    if (int rc = clock.stop(c->stream)) return rc;
    D2H(total_length + r0, d_total, sizeof(double) * (size_t)nr);
    if (distances) if (int rc = rows_out(c, distances + r0, (size_t)n_trajectories, d_dist, (size_t)n_seg, (size_t)nr)) return rc;
    if (speeds) if (int rc = rows_out(c, speeds + r0, (size_t)n_trajectories, d_speed, (size_t)n_seg, (size_t)nr)) return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// Device time of the launches of the last odr_trajectory_lengths of this context [ms], summed over its slabs
int odr_trajectory_lengths_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_TRAJ_LENGTHS].read(ms);
}
