// libodrift_hip.so, a translation unit of its own: density maps of a finished run (OpenDriftSimulation.get_density_array,
// models/basemodel/__init__.py:4091-4146).  See odrift.hip for the rest.
#include "odr_host.h"
#include "odr_density.hip.h"

namespace {

constexpr size_t DENSITY_SLAB_BYTES = 256u << 20;      // device memory of one slab of host inputs (ODR_DENSITY_SLAB_BYTES overrides)
constexpr long long DENSITY_LAUNCH_ENTRIES = 1ll << 30;   // entries of one launch

int edges_ok(const double *e, int n, const char *what) {
  REQUIRE(n >= 2, "%s: %d edges, fewer than two", what, n);
  for (int k = 0; k < n; ++k) REQUIRE(std::isfinite(e[k]), "%s[%d] is not finite", what, k);
  for (int k = 1; k < n; ++k) REQUIRE(e[k] > e[k - 1], "%s is not strictly increasing at %d", what, k);
  return 0;
}

template <bool WEIGHTED, typename T>
int launch(odr_ctx *c, const DensityArgs &A, bool lds, T *H, T *Hsub, T *Hstr) {
  const size_t shm = lds ? sizeof(double) * (size_t)(A.ax_lon.n + A.ax_lat.n) : 0;
  if (lds) hipLaunchKernelGGL((k_density<WEIGHTED, true, T>), dim3(nblk(A.n)), dim3(BLOCK), shm, c->stream, A, H, Hsub, Hstr);
  else hipLaunchKernelGGL((k_density<WEIGHTED, false, T>), dim3(nblk(A.n)), dim3(BLOCK), 0, c->stream, A, H, Hsub, Hstr);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

// get_density_array (models/basemodel/__init__.py:4091-4146) for given bin edges: H, H_submerged, H_stranded of every output time.
// Host inputs go to the device in slabs of whole trajectories (their rows are contiguous); the histograms stay resident for all of
// them.  Synchronous.
int odr_density_map(odr_ctx *c, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, const float *z,
                    const float *status, const float *weight, int32_t stranded_code, int32_t n_lon_edges, const double *lon_edges,
                    int32_t n_lat_edges, const double *lat_edges, double *H, double *H_submerged, double *H_stranded) {
  REQUIRE(c && lon && lat && z && status && lon_edges && lat_edges && H && H_submerged, "NULL argument");
  REQUIRE(H_stranded || stranded_code < 0, "NULL H_stranded with a stranded category");
  REQUIRE(n_trajectories >= 0 && n_times >= 0, "negative size");
  REQUIRE((unsigned long long)n_trajectories < (1ull << 32), "%lld trajectories: the counts are 32-bit", (long long)n_trajectories);
  if (int rc = edges_ok(lon_edges, n_lon_edges, "lon_edges")) return rc;
  if (int rc = edges_ok(lat_edges, n_lat_edges, "lat_edges")) return rc;
  const unsigned long long plane = (unsigned long long)(n_lon_edges - 1) * (unsigned long long)(n_lat_edges - 1);
  REQUIRE(plane <= (1ull << 28), "%llu bins per output time, more than 2^28", plane);
  if (n_times == 0) return 0;
  const size_t cells = (size_t)n_times * plane;
  const int nh = stranded_code >= 0 ? 3 : 2;
  double *out[3] = {H, H_submerged, H_stranded};
  if (n_trajectories == 0) {
    for (int k = 0; k < 3; ++k) if (out[k]) std::fill(out[k], out[k] + cells, 0.0);
    return 0;
  }
  const bool weighted = weight != nullptr;
  const size_t cell_bytes = weighted ? sizeof(double) : sizeof(unsigned);

  HIPCHK(hipSetDevice(c->device));
  DevScope B;      // released on every way out
  void *hist, *slab = nullptr;
  double *edges;
  if (int rc = B.alloc(&hist, 3 * cells * cell_bytes)) return rc;      // (H_stranded's is written by nothing when there is no such category)
  HIPCHK(hipMemsetAsync(hist, 0, 3 * cells * cell_bytes, c->stream));
  if (int rc = B.alloc((void **)&edges, sizeof(double) * (size_t)(n_lon_edges + n_lat_edges))) return rc;
  H2D(edges, lon_edges, sizeof(double) * (size_t)n_lon_edges);
  H2D(edges + n_lon_edges, lat_edges, sizeof(double) * (size_t)n_lat_edges);

  // slab: whole trajectories; the arrays that are host memory take slab_bytes / n_host of device memory each
  const float *in[5] = {lon, lat, z, status, weight};
  bool dev[5];
  int n_host = 0;
  for (int k = 0; k < 5; ++k) {
    dev[k] = in[k] ? odr_i_on_device(in[k]) : true;
    if (!dev[k]) ++n_host;
  }
  long long slab_traj = std::max<long long>(1, DENSITY_LAUNCH_ENTRIES / n_times);
  if (n_host) {
    size_t budget = DENSITY_SLAB_BYTES;
    if (const char *s = getenv("ODR_DENSITY_SLAB_BYTES")) {
      const long long v = atoll(s);
      REQUIRE(v > 0, "ODR_DENSITY_SLAB_BYTES=%s", s);
      budget = (size_t)v;
    }
    const size_t row = sizeof(float) * (size_t)n_times * (size_t)n_host;
    slab_traj = std::min<long long>(slab_traj, std::max<long long>(1, (long long)(budget / row)));
  }
  slab_traj = std::min<long long>(slab_traj, n_trajectories);
  const size_t slab_floats = (size_t)slab_traj * (size_t)n_times;
  if (n_host) if (int rc = B.alloc(&slab, sizeof(float) * slab_floats * (size_t)n_host)) return rc;

  DensityArgs A;
  A.lon_edges = edges; A.lat_edges = edges + n_lon_edges;
  A.ax_lon = density_axis(lon_edges, n_lon_edges); A.ax_lat = density_axis(lat_edges, n_lat_edges);
  A.n_times = n_times; A.stranded_code = stranded_code;
  const bool lds = n_lon_edges + n_lat_edges <= DENSITY_LDS_EDGES;
  KernelClock &clock = c->clock[CLOCK_DENSITY];
  clock.reset();
  for (long long t0 = 0; t0 < n_trajectories; t0 += slab_traj) {
    const long long nt = std::min(slab_traj, n_trajectories - t0);
    const size_t off = (size_t)t0 * (size_t)n_times, count = (size_t)nt * (size_t)n_times;
    const float *ptr[5];
    int h = 0;
    for (int k = 0; k < 5; ++k) {
      if (!in[k]) { ptr[k] = nullptr; continue; }
      if (dev[k]) { ptr[k] = in[k] + off; continue; }
      float *d = (float *)slab + slab_floats * (size_t)h++;
      H2D(d, in[k] + off, sizeof(float) * count);      // waits for the stream: the launch of the slab before has read `d`
      ptr[k] = d;
    }
    A.lon = ptr[0]; A.lat = ptr[1]; A.z = ptr[2]; A.status = ptr[3]; A.weight = ptr[4];
    A.n = (long long)count;
    int rc = clock.start(c->stream);
    if (rc) return rc;
    if (weighted) {
      double *h64 = (double *)hist;
      rc = launch<true, double>(c, A, lds, h64, h64 + cells, h64 + 2 * cells);
    } else {
      unsigned *h32 = (unsigned *)hist;
      rc = launch<false, unsigned>(c, A, lds, h32, h32 + cells, h32 + 2 * cells);
    }
    if (rc) return rc;
    if ((rc = clock.stop(c->stream))) return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));

  // histograms -> float64 host arrays, through the bounce buffer
  void *b;
  if (int rc = odr_i_bounce(c, 0, &b)) return rc;
  const size_t chunk = ODR_BOUNCE_BYTES / cell_bytes;
  for (int k = 0; k < nh; ++k) {
    for (size_t o = 0; o < cells; o += chunk) {
      const size_t m = std::min(chunk, cells - o);
      HIPCHK(hipMemcpyAsync(b, (const char *)hist + ((size_t)k * cells + o) * cell_bytes, m * cell_bytes, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      if (weighted) memcpy(out[k] + o, b, m * sizeof(double));
      else for (size_t i = 0; i < m; ++i) out[k][o + i] = (double)((const unsigned *)b)[i];
    }
  }
  if (nh == 2 && H_stranded) std::fill(H_stranded, H_stranded + cells, 0.0);
  return 0;
}

// Device time of the k_density launches of the last odr_density_map of this context [ms], summed over its slabs
int odr_density_last_kernel_ms(odr_ctx *c, float *ms) {
  REQUIRE(c && ms, "NULL argument");
  return c->clock[CLOCK_DENSITY].read(ms);
}
