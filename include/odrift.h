/* odrift.h -- C ABI of libodrift_hip.so: the MI355X-native particle-advection
 * hot path behind OpenDrift's model / reader API.
 *
 * The reference (OpenDrift v1.14.10) is pure Python and has NO FFI for this
 * path; its boundary is class inheritance + duck typing.  Each entry point below
 * therefore names the reference METHOD it replaces (file:line under
 * /root/reference).  The binding a maintainer adds on the reference side is a
 * ctypes stub; it is shown in INTEGRATION.md and shipped in
 * opendrift_amd/_abi.py.
 *
 * Conventions: every function returns 0 on success, a negative odr_status on
 * error (odr_last_error() gives a thread-local message).  Opaque handles own
 * all device memory; host buffers belong to the caller and may be freed as soon
 * as the call returns.  Calls are asynchronous on the context's HIP stream
 * unless they return data to the host.  One host thread per context.  No torch
 * types, no callbacks.
 */
#ifndef ODRIFT_H
#define ODRIFT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct odr_ctx odr_ctx;
typedef struct odr_particles odr_particles;

typedef enum {
  ODR_OK = 0,
  ODR_ERR_INVALID = -1,  /* bad argument (ValueError on the Python side) */
  ODR_ERR_HIP = -2,      /* HIP runtime failure */
  ODR_ERR_CAPACITY = -3, /* particle capacity / slot / table exhausted */
  ODR_ERR_STATE = -4     /* call made in the wrong order (WrongMode analogue) */
} odr_status;

/* ---- environment variables on the path (CF standard names, OceanDrift.required_variables,
 *      opendrift/models/oceandrift.py:60-88) ---- */
enum {
  ODR_VAR_X_SEA_WATER_VELOCITY = 0,
  ODR_VAR_Y_SEA_WATER_VELOCITY = 1,
  ODR_VAR_X_WIND = 2,
  ODR_VAR_Y_WIND = 3,
  ODR_VAR_UPWARD_SEA_WATER_VELOCITY = 4,
  ODR_VAR_OCEAN_VERTICAL_DIFFUSIVITY = 5,
  ODR_VAR_STOKES_DRIFT_X_VELOCITY = 6,
  ODR_VAR_STOKES_DRIFT_Y_VELOCITY = 7,
  ODR_VAR_LAND_BINARY_MASK = 8,
  ODR_VAR_SEA_FLOOR_DEPTH = 9,
  ODR_VAR_SEA_SURFACE_HEIGHT = 10,
  ODR_VAR_HORIZONTAL_DIFFUSIVITY = 11,
  ODR_VAR_SIGNIFICANT_WAVE_HEIGHT = 12,
  ODR_VAR_WAVE_PERIOD = 13,
  ODR_VAR_MIXED_LAYER_THICKNESS = 14,
  ODR_VAR_SEA_WATER_TEMPERATURE = 15, /* OpenOil.required_variables (models/openoil/openoil.py:271-278) */
  ODR_VAR_SEA_WATER_SALINITY = 16,
  ODR_VAR_SEA_ICE_AREA_FRACTION = 17, /* OpenOil.advect_oil in ice (models/openoil/openoil.py:1179-1216) */
  ODR_VAR_SEA_ICE_X_VELOCITY = 18,    /* a vector pair: rotated from the reader's projection (basereader/consts.py:27-36) */
  ODR_VAR_SEA_ICE_Y_VELOCITY = 19,
  /* the windsea_swell Stokes profile (models/physics_methods.py:418-456, 831-841) */
  ODR_VAR_SWELL_WAVE_TO_DIRECTION = 20,
  ODR_VAR_SWELL_WAVE_PEAK_PERIOD = 21,
  ODR_VAR_SWELL_WAVE_SIGNIFICANT_HEIGHT = 22,
  ODR_VAR_WIND_WAVE_TO_DIRECTION = 23,
  ODR_VAR_WIND_WAVE_MEAN_PERIOD = 24,
  ODR_VAR_WIND_WAVE_SIGNIFICANT_HEIGHT = 25,
  ODR_NVAR = 26
};

/* ---- projections of a reader (pyproj.Proj(reader.proj4), basereader/__init__.py:119-137) ---- */
enum { ODR_PROJ_LATLONG = 0, ODR_PROJ_STERE_EQUIT_SPHERE = 1, ODR_PROJ_STERE_POLAR = 2,
       ODR_PROJ_CURVILINEAR = 3 /* set by odr_source_grid_curvilinear, not through odr_proj_desc */,
       ODR_PROJ_MERC = 4 /* +proj=merc (+lat_ts or +k_0), sphere or ellipsoid: Snyder ch. 7 */,
       ODR_PROJ_LCC = 5 /* +proj=lcc +lat_1 [+lat_2] +lat_0 +lon_0, sphere or ellipsoid: Snyder ch. 15 */,
       /* round 5 -- pyproj.Proj of variables.py:111-143 for the other projections model files carry: */
       ODR_PROJ_TMERC = 6 /* +proj=tmerc (+proj=utm: the caller resolves the zone into lon0 / k0 / x0 / y0): Krueger's series to
                             order 6 in the third flattening (Karney 2011), sphere or ellipsoid */,
       ODR_PROJ_LAEA = 7 /* +proj=laea, any aspect, sphere or ellipsoid: Snyder ch. 24 */,
       ODR_PROJ_STERE_OBLIQUE = 8 /* +proj=stere with lat_0 not a pole (oblique, equatorial), sphere or ellipsoid, +k_0: Snyder ch. 21 */,
       ODR_PROJ_OB_TRAN = 9 /* +proj=ob_tran +o_proj=longlat: the rotated pole; lat1_deg = o_lat_p, lat2_deg = o_lon_p, lon0_deg = lon_0;
                               reader coordinates are rotated longitude / latitude in DEGREES (variables.py:117-123,136-138); vector
                               pairs are rotated by the WGS84 azimuth of the 0.1-degree line along +y (variables.py:80-97) */,
       ODR_PROJ_MOLL = 11 /* +proj=moll +lon_0 +x_0 +y_0 on the sphere of radius a (PROJ's moll; es is ignored): Snyder ch. 31.  A map
                             grid only: the entry points of "projected density and concentration maps" below take it, every other
                             one refuses it (10 is taken inside the library) */ };
typedef struct {
  int32_t kind;
  double a, es;                  /* semi-major axis, eccentricity squared */
  double lat0_deg, lon0_deg, lat_ts_deg, k0, x0, y0;
  double lat1_deg, lat2_deg;     /* standard parallels (ODR_PROJ_LCC; lat2 = lat1 for the tangent cone); o_lat_p, o_lon_p (ODR_PROJ_OB_TRAN) */
} odr_proj_desc;

enum { ODR_SCHEME_EULER = 0, ODR_SCHEME_RK2 = 1, ODR_SCHEME_RK4 = 2 };
enum { ODR_RNG_DEVICE = 0, ODR_RNG_HOST = 1 }; /* Philox on device | numbers drawn by the caller (np.random parity) */
enum { ODR_COAST_NONE = 0, ODR_COAST_STRANDING = 1, ODR_COAST_PREVIOUS = 2 };
enum { ODR_ANALYTIC_DOUBLE_GYRE = 1, ODR_ANALYTIC_OSCILLATING = 2 };

/* ---------------------------------------------------------------- lifecycle */
int odr_ctx_create(int device, uint64_t seed, odr_ctx **out);
int odr_ctx_destroy(odr_ctx *ctx);
int odr_sync(odr_ctx *ctx);
int odr_set_stream(odr_ctx *ctx, void *hip_stream); /* adopt a caller-owned hipStream_t (NULL = own stream) */
const char *odr_last_error(void);
const char *odr_version(void);

/* ------------------------------------------------- particle state (SoA in HBM)
 * replaces LagrangianArray (opendrift/elements/elements.py:22-254): one array per
 * property; lon/lat/z float64, ID/status/moving int32, drift factors float32. */
int odr_particles_create(odr_ctx *ctx, int64_t capacity, odr_particles **out);
int odr_particles_destroy(odr_ctx *ctx, odr_particles *p);
/* release_elements (basemodel/__init__.py:909-934) / LagrangianArray.extend (elements.py:170-195):
 * append n elements to the active set.  NULL optional arrays take the defaults
 * moving=1, wind_drift_factor=0.02, current_drift_factor=1, terminal_velocity=0. */
int odr_particles_append(odr_ctx *ctx, odr_particles *p, int64_t n, const double *lon,
                         const double *lat, const double *z, const int32_t *id,
                         const int32_t *moving, const float *wind_drift_factor,
                         const float *current_drift_factor, const float *terminal_velocity);
int odr_particles_count(odr_ctx *ctx, odr_particles *p, int64_t *n_active, int64_t *n_deactivated);
/* host copy of the live state (state_to_buffer input, basemodel/__init__.py:2384-2403); any pointer may be NULL */
int odr_particles_download(odr_ctx *ctx, odr_particles *p, double *lon, double *lat, double *z,
                           int32_t *id, int32_t *status, int32_t *moving);
int odr_particles_download_deactivated(odr_ctx *ctx, odr_particles *p, double *lon, double *lat,
                                       double *z, int32_t *id, int32_t *status);
/* overwrite properties of the active set from the host (model subclasses that update elements on the host) */
int odr_particles_upload(odr_ctx *ctx, odr_particles *p, const double *lon, const double *lat,
                         const double *z, const int32_t *moving, const float *wind_drift_factor,
                         const float *current_drift_factor, const float *terminal_velocity);
/* float32 element properties of the active set: "wind_drift_factor", "current_drift_factor", "terminal_velocity",
 * "age_seconds" (LagrangianArray variables, elements/elements.py:71-88) */
int odr_particles_download_f32(odr_ctx *ctx, odr_particles *p, const char *name, float *host);
/* raw device pointers (for torch.distributed / zero-copy consumers): name in
 * {"lon","lat","z","id","status","moving","env:<var_id>"} */
int odr_particles_device_ptr(odr_ctx *ctx, odr_particles *p, const char *name, void **dptr);

/* ------------------------------------------------------- field sources (readers)
 * A source is the device image of one Reader.  Priority lists per variable follow
 * Environment.priority_list (environment.py:339-374). */
/* reader_constant.Reader / environment:constant:<var> (reader_constant.py:60-82, environment.py:172-182) */
int odr_source_constant(odr_ctx *ctx, int nvars, const int32_t *var_ids, const double *values,
                        int32_t *source_id);
/* ContinuousReader analytic fields: reader_double_gyre.py:55-79 params {A, epsilon, omega, t0_epoch};
 * reader_oscillating.py:49-59 params {var_id, amplitude, period_seconds, t0_epoch} */
int odr_source_analytic(odr_ctx *ctx, int kind, const double *params, int nparams,
                        int32_t *source_id);
/* reader_global_landmask.Reader (readers/reader_global_landmask.py:201-255) as a device source: a lon/lat raster,
 * cells[iy * nx + ix] != 0 is land, cell (ix, iy) covers lon0 + [ix, ix+1) dlon x lat0 + [iy, iy+1) dlat; ocean outside.
 * Exact at the element position (ContinuousReader), longitudes modulated to [-180, 180).  The GSHHG data the
 * reference ships through roaring_landmask is not part of this repository: any raster can be handed over. */
int odr_source_landmask(odr_ctx *ctx, int32_t nx, int32_t ny, double lon0, double lat0, double dlon, double dlat,
                        const uint8_t *cells, int32_t *source_id);
/* StructuredReader on a regular grid in its own projection (basereader/structured.py).
 * domain = {xmin,xmax,ymin,ymax,zmin,zmax}; lon_mode 1: [-180,180), 2: [0,360) (variables.py:259-280);
 * z = block z levels (NULL / nz<=1 for surface fields). */
int odr_source_grid(odr_ctx *ctx, const odr_proj_desc *proj, const double *domain6,
                    int lon_mode, int mod360_x, int nz, const double *z, int32_t *source_id);
/* StructuredReader WITHOUT a projection (basereader/structured.py:44-113; reader_ROMS_native.py and every reader that
 * only has 2D lon/lat arrays): x/y are pixel indices, and lonlat2xy (structured.py:438-472) is scipy's
 * LinearNDInterpolator over the Delaunay triangulation of the nodes.  lon/lat: [ny, nx] float64 node coordinates;
 * domain = {0, nx-1, 0, ny-1, zmin, zmax}.  The same triangulation is built here from the structured mesh (cell
 * diagonals + edge flips, csrc/odr_mesh.h), the device walks it per particle; positions outside the
 * mesh outline are "not covered".  ODR_ERR_INVALID for folded / non-convex cells or non-finite nodes. */
int odr_source_grid_curvilinear(odr_ctx *ctx, const double *lon, const double *lat, int ny, int nx,
                                const double *domain6, int lon_mode, int nz, const double *z,
                                int32_t *source_id);
/* Variables.lonlat2xy of one source (variables.py:111-143, longitudes modulated as :259-280) for n host positions ->
 * reader coordinates x, y (NaN outside a curvilinear mesh); synchronous.  Host-side callers (seeding, tests); the
 * step kernels do the same transform in registers. */
int odr_source_lonlat2xy(odr_ctx *ctx, int32_t source_id, int64_t n, const double *lon, const double *lat,
                         double *x, double *y);
/* One time level = one ReaderBlock (interpolation/structured.py:15-94).  data[k] is a host
 * float32 array [var_nz[k], ny, nx] (var_nz 1 => 2D).  xy8 = {x0, xspan, y0, yspan, xmin,
 * xrange, ymin, yrange} with the spans formed in the dtype of the reader's x/y arrays
 * (interpolators.py:32-33,110-111).  The upload masks |v|>1e9, fills NaN towards the
 * seafloor and pre-dilates NaN cells 10x (interpolators.py:9-20,127-137). */
int odr_block_upload(odr_ctx *ctx, int32_t source_id, int32_t slot, double t_epoch, int nvars,
                     const int32_t *var_ids, const float *const *data, const int32_t *var_nz,
                     int ny, int nx, const double *xy8);
/* same, the float32 data already live in device memory (RCCL-broadcast blocks, odr_sgrid_zslice results); with
 * unified addressing each data[k] may individually be a host or a device pointer in either call */
int odr_block_upload_device(odr_ctx *ctx, int32_t source_id, int32_t slot, double t_epoch,
                            int nvars, const int32_t *var_ids, const void *const *dev_data,
                            const int32_t *var_nz, int ny, int nx, const double *xy8);
/* Asynchronous upload: odr_block_upload_async only ENQUEUES the copy and the preparation kernels on the context's
 * upload stream and returns; the simulation continues on the compute stream.  The staged block becomes the content
 * of its slot with odr_block_commit (the compute stream then waits for the upload's event; the block it replaces
 * is released once the compute stream has passed).  data[k] must stay valid until the commit and should be
 * page-locked (odr_host_register) or device memory, otherwise the copies are staged synchronously by the runtime.
 * odr_block_upload = upload_async + wait + commit. */
int odr_block_upload_async(odr_ctx *ctx, int32_t source_id, int32_t slot, double t_epoch, int nvars,
                           const int32_t *var_ids, const void *const *data, const int32_t *var_nz,
                           int ny, int nx, const double *xy8);
int odr_block_commit(odr_ctx *ctx, int32_t source_id, int32_t slot);
/* Optional: content ids of variables of the level just uploaded (the staged level of the slot if there is one, else the
 * resident one).  Two resident levels that carry the same non-zero id for a variable hold the same values for it -- the
 * reference re-reads sea_floor_depth / land_binary_mask with every ReaderBlock (structured.py:15-94) -- and the samplers then
 * gather that variable at one level only (the time interpolation keeps its arithmetic: same bits).  0 = unknown. */
int odr_block_set_content_ids(odr_ctx *ctx, int32_t source_id, int32_t slot, int nvars, const int32_t *var_ids,
                              const uint64_t *ids);
int odr_host_register(odr_ctx *ctx, void *ptr, uint64_t bytes);   /* hipHostRegister: reader arrays that are uploaded repeatedly */
int odr_host_unregister(odr_ctx *ctx, void *ptr);
int odr_block_drop(odr_ctx *ctx, int32_t source_id, int32_t slot);
/* Debugging / tests: the K plane of a resident level -- ocean_vertical_diffusivity a second time, as *krec = 4 * ((nz + 3) / 4)
 * floats per node (z innermost, node order iy * nx + ix, padding floats 0), written by the level's preparation next to the node
 * records when the block can serve the K-column mixing kernels (csrc/odr_field.hip.h DevBlock::kplane).  *krec = 0: the level
 * has none.  plane_out / records_out (both or neither; cap_floats >= ny * nx * *krec each): the plane, and the K part of the
 * node records in the plane's layout, which the plane equals bit for bit; synchronous. */
int odr_block_kplane_read(odr_ctx *ctx, int32_t source_id, int32_t slot, int32_t *krec, float *plane_out, float *records_out,
                          uint64_t cap_floats);
/* Debugging / tests: one variable of a resident level as the preparation left it -- convolved (odr_source_set_convolution), masked,
 * filled towards the sea floor and dilated -- gathered from the node records into a plain float32 [*nz][ny][nx] array.  *nz = 0: the
 * level does not hold the variable.  out may be NULL (only *nz is wanted); cap_floats >= *nz * ny * nx; synchronous. */
int odr_block_read(odr_ctx *ctx, int32_t source_id, int32_t slot, int32_t var_id, int32_t *nz, float *out, uint64_t cap_floats);
/* StructuredReader.set_convolution_kernel + __convolve_block__ (readers/basereader/structured.py:163-192, applied :278-306): every
 * level of the grid source uploaded AFTER this call -- odr_block_upload, _async, _device and odr_block_broadcast alike -- is
 * convolved on the upload stream before it is masked, filled and dilated, with the arithmetic of scipy.ndimage.convolve(array,
 * weights, mode='nearest'): one double accumulator per cell, the terms (double)value * weight added in C order of the flipped
 * kernel, weights with |w| <= DBL_EPSILON left out, the sum rounded once to float32 (csrc/odr_convolve.hip.h).  weights: [ky][kx]
 * doubles as the reference hands them to SciPy (an int N there means ones((N, N)) / N**2: the caller forms it), not normalised
 * here; 1 <= ky, kx <= 15.  A 2-D variable is convolved over (y, x); a 3-D one with weights[:, :, None], i.e. over (z, y) -- the
 * reference's behaviour.  Every variable of the level is convolved, land_binary_mask and sea_floor_depth_below_sea_level included.
 * vars3d[n3d]: the variables the reader hands out as 3-D arrays of ONE layer ([1][ny][nx]; var_nz says 1 for them as for a 2-D
 * array): the reference convolves such an array over (z, y) like any 3-D one, and so does the upload.  ky = kx = 0 (the other
 * arguments ignored) switches it off.  Levels already resident stay as they are.  ODR_ERR_INVALID for a larger kernel, and at the
 * upload of a level with ensemble members (odr_source_set_members). */
int odr_source_set_convolution(odr_ctx *ctx, int32_t source_id, int32_t ky, int32_t kx, const double *weights, int32_t n3d,
                               const int32_t *vars3d);
/* drift:truncate_ocean_model_below_m (models/basemodel/environment.py:554-566): every get_environment call samples the readers
 * at max(z, -truncate_depth) while the elements keep their depth.  odr_particles_truncate_z puts the clipped depths in place for
 * the sampling calls that follow (odr_env_sample, odr_advect / odr_env_coast_advect: the Runge-Kutta stage calls are
 * get_environment calls), odr_particles_restore_z brings the elements' own z back (before anything that changes z or the
 * element set). */
int odr_particles_truncate_z(odr_ctx *ctx, odr_particles *p, double truncate_depth);
int odr_particles_restore_z(odr_ctx *ctx, odr_particles *p);
/* A source that is no longer used (e.g. a gridded reader whose blocks are re-cut to another window and re-registered):
 * drops its resident blocks, removes it from every priority list (odr_env_bind) and frees its id for the next
 * odr_source_* call -- the context holds at most 16 sources at a time, not 16 per run. */
int odr_source_release(odr_ctx *ctx, int32_t source_id);
/* reader.start_time / end_time / always_valid (covers_time, variables.py:392-400): outside the
 * interval the reader is skipped and the next reader / the fallback applies */
int odr_source_time_coverage(odr_ctx *ctx, int32_t source_id, double t_start_epoch, double t_end_epoch,
                             int always_valid);
/* Ensemble data: the reader hands `var` out as a LIST of `members` arrays (readers/basereader/structured.py:125-147);
 * ReaderBlock.interpolate gives element number j of a call the member j % members
 * (readers/interpolation/structured.py:119-135).  Declare it before the blocks are uploaded; the block arrays of `var`
 * then hold the members one after the other along the layer axis ([members x nz][ny][nx], var_nz = members x nz).
 * Element number = rank, in ascending ID (the reference's array order for seed times that are monotonic in ID), among the
 * elements the reference HANDS to the block: the active ones the reader's domain covers at the positions of that call
 * (get_variables_interpolated, variables.py:747-765) -- formed per call by odr_env_sample and, for the stage calls of
 * odr_advect / odr_env_coast_advect, once at the elements' positions (a launch that holds all stages cannot renumber at
 * the stage positions: a host that needs that -- elements crossing the reader's edge -- samples the stages one by one, as
 * opendrift_amd's stage-split lane does).  With several ensemble readers, one behind another reader in its priority
 * list, or in a sharded run (odr_particles_set_rank_offset) every active element is numbered.  Sampled by the generic
 * kernels; ocean_vertical_diffusivity profiles cannot be ensemble data. */
int odr_source_set_members(odr_ctx *ctx, int32_t source_id, int32_t var, int32_t members);
/* Ensemble data hands element number j OF THE CALL member j % M (readers/interpolation/structured.py:119-135): j is the rank
 * of the element among the present ones in ascending ID.  A particle set that holds only a contiguous ID range of a larger
 * simulation (one rank of a sharded run) adds the number of present elements with smaller IDs held elsewhere; the host
 * knows it from the step's collective.  Default 0. */
int odr_particles_set_rank_offset(odr_ctx *ctx, odr_particles *p, int64_t offset);
/* priority list + fallback of one variable (environment.py:592-595,782-791); NaN = no fallback */
int odr_env_bind(odr_ctx *ctx, int32_t var_id, int nsources, const int32_t *source_ids,
                 float fallback);

/* ------------------------------------------------------------ hot-path stages */
/* Environment.get_environment (environment.py:499-923): sample var_ids at the particles'
 * (lon,lat,z) and time into the device environment (float32).  out_host[k] (optional)
 * receives a copy.  The sample positions are remembered for the vertical profiles used by
 * odr_vmix (environment_profiles are taken at these positions, oceandrift.py:431-447). */
int odr_env_sample(odr_ctx *ctx, odr_particles *p, int nvars, const int32_t *var_ids,
                   double t_epoch, float *const *out_host);
int odr_env_download(odr_ctx *ctx, odr_particles *p, int32_t var_id, float *out_host);
int odr_env_upload(odr_ctx *ctx, odr_particles *p, int32_t var_id, const float *host);
/* drift:current_uncertainty / wind_uncertainty (environment.py:869-879,887-891): env[x] += N(0,std), env[y] += N(0,std)
 * (ODR_NOISE_NORMAL); drift:current_uncertainty_uniform (:880-886): env[x] += U(-std,std), env[y] += U(-std,std)
 * (ODR_NOISE_UNIFORM).  ODR_RNG_HOST: host_nx / host_ny = the np.random draws (already scaled by std). */
enum { ODR_NOISE_NORMAL = 0, ODR_NOISE_UNIFORM = 1 };
int odr_env_add_noise(odr_ctx *ctx, odr_particles *p, int32_t var_x, int32_t var_y, double std, int distribution,
                      int rng_mode, const double *host_nx, const double *host_ny, uint64_t step);
/* The same uncertainties INSIDE advect_ocean_current: the reference adds them in every get_environment call whose
 * variables hold the current, i.e. also in the one (RK2) / three (RK4) stage calls (physics_methods.py:638-670 ->
 * environment.py:869-886).  Arms the NEXT odr_advect / odr_env_coast_advect on `p` (call it right before).
 * ODR_RNG_DEVICE: one Philox stream per (ID, step, call, distribution).  ODR_RNG_HOST: host_stage = the draws of the
 * stage calls in np.random order, [nstage][ncomp][n] with ncomp = 2 (normal x, y | uniform x, y) or 4 (normal x, y,
 * uniform x, y), n = active elements; host_main = [ncomp][n] draws of the main-loop sample for odr_env_coast_advect
 * with odr_step_extras.main_noise (NULL otherwise). */
int odr_advect_set_noise(odr_ctx *ctx, odr_particles *p, double std_normal, double std_uniform, int rng_mode,
                         const double *host_main, const double *host_stage, int nstage, uint64_t step);
/* Arithmetic of the Runge-Kutta STAGE evaluations inside odr_advect / odr_env_coast_advect (physics_methods.py:629-670: the
 * sub-stage position geod.fwd(lon, lat, azimuth, speed*dt*.5) and the get_environment call of the current there).
 *   ODR_STAGE_EXACT (default): every float32 rounding point of the reference inside a stage is reproduced (float32
 *     azimuth / distance, each (time, z) layer of the ReaderBlock rounded to float32): <= 1e-10 deg per step vs the oracle.
 *   ODR_STAGE_FAST: stage step taken directly along (u, v) dt/2, the stage value of a gridded reader as one float32
 *     weighted sum of its 16 corner values: <= 2e-9 deg per step vs the oracle (the stage value is a few float32 ulp off).
 * The main-loop sample (o.environment), the RK combination and the final update_positions are identical in both modes;
 * Euler is unaffected.  Applies to every particle set of the context from the next call on. */
enum { ODR_STAGE_EXACT = 0, ODR_STAGE_FAST = 1 };
int odr_ctx_set_stage_math(odr_ctx *ctx, int mode);
/* PhysicsMethods.advect_ocean_current (physics_methods.py:611-691) + update_positions
 * (basemodel/__init__.py:4631-4657), all sub-stages fused in one kernel. */
int odr_advect(odr_ctx *ctx, odr_particles *p, int scheme, double t_epoch, double dt, double factor);
/* One iteration of the run() loop up to and including the current advection
 * (basemodel/__init__.py:2136-2248): odr_env_sample(var_ids, t) -> odr_coastline(action, codes) ->
 * [odr_seafloor -> odr_increase_age, if `extras` asks for them] -> odr_store_previous (if store_previous) ->
 * odr_advect(scheme, t, dt, factor), fused into ONE kernel
 * when the group holding x/y_sea_water_velocity comes from one gridded reader (else the four calls are
 * made in that order).  Elements the coastline deactivates ('stranded', 'seeded_on_land') are
 * flagged and left where the coastline put them -- the reference removes them before update() --
 * so  fused call + odr_compact  is bit-identical to  sample, coastline, compact, store_previous,
 * advect. */
typedef struct {              /* optional bookkeeping of the same loop body, between the coastline and update_previous_state */
  int32_t seafloor_action;    /* 1: interact_with_seafloor 'lift_to_seafloor' (:748-783), else none */
  int32_t retired_code;       /* status of elements older than max_age_seconds */
  double age_dt;              /* increase_age_and_retire (:2342-2352): age_seconds += age_dt; 0: not part of this call */
  double max_age_seconds;     /* 0: no retirement */
  int32_t missing_code;       /* report_missing_variables (:2501-2515), first in the loop's order: elements with a NaN in
                               * any sampled variable (no reader covers them and there is no fallback) get this status;
                               * 0: not part of this call */
  int32_t main_noise;        /* 1: add the armed current uncertainty (odr_advect_set_noise) to the sampled current
                              * right after the sample, like get_environment does (environment.py:869-886) */
  /* OceanDrift.vertical_mixing (+ vertical_advection) of the same step as part of this call: what
   * odr_vmix_fuse_vertical_advection + odr_vmix(t_epoch, dt, vmix_dt_mix, vmix_at_surface, ODR_RNG_DEVICE, NULL,
   * vmix_step) would do after it (vertical mixing reads the environment of the step start and changes z only, so it
   * commutes with the horizontal movers).  The mixing runs as a second launch, right after the step's. */
  int32_t vmix;              /* 0: not part of this call */
  int32_t vmix_at_surface;   /* drift:vertical_mixing_at_surface */
  int32_t vmix_vadv;         /* vertical advection after the mixing: -1 none, 0 below the surface, 1 including it */
  int32_t pad;
  double vmix_dt_mix;        /* vertical_mixing:timestep */
  uint64_t vmix_step;        /* Philox offset (the model step number) */
} odr_step_extras;
int odr_env_coast_advect(odr_ctx *ctx, odr_particles *p, int nvars, const int32_t *var_ids, double t_epoch,
                         int coastline_action, int stranded_code, int seeded_on_land_code,
                         int store_previous, int scheme, double dt, double factor,
                         const odr_step_extras *extras /* NULL: none */, int64_t *n_on_land);
/* update_positions with caller-supplied velocities (models that compute them on the host) */
int odr_update_positions(odr_ctx *ctx, odr_particles *p, const double *x_vel, const double *y_vel,
                         int velocities_are_float32, double dt);

/* Per-element factors of the movers that follow, as OpenOil.advect_oil derives them from the float32
 * sea_ice_area_fraction A of the sampled environment (models/openoil/openoil.py:1182-1216): ICE_CURRENT = 1 - k_ice with
 * k_ice = clip((A - 0.3) / 0.5, 0, 1) for odr_advect and odr_advect_wind, ICE_STOKES = (0.7 - A) / 0.7 (0 above 0.7) for
 * odr_stokes_drift, ICE_DRIFT = k_ice for odr_advect_sea_ice.  With a kind other than SCALAR the scalar `factor`
 * argument of those calls is not used.  Stays in force until set again. */
enum { ODR_FACTOR_SCALAR = 0, ODR_FACTOR_ICE_CURRENT = 1, ODR_FACTOR_ICE_STOKES = 2, ODR_FACTOR_ICE_DRIFT = 3 };
int odr_set_element_factor(odr_ctx *ctx, odr_particles *p, int kind);
/* advect_with_sea_ice (models/physics_methods.py:693-710): update_positions(factor * sea_ice_x/y_velocity) with the
 * sampled ice velocity; without it the rule of thumb current + 1.5 % of the wind; nothing when neither is there. */
int odr_advect_sea_ice(odr_ctx *ctx, odr_particles *p, double dt, double factor);
/* advect_wind (physics_methods.py:712-791) */
int odr_advect_wind(odr_ctx *ctx, odr_particles *p, double dt, double wind_drift_depth,
                    int relative_wind, double factor);
/* stokes_drift (physics_methods.py:793-848); profile 0 monochromatic, 1 exponential, 2 Phillips, 3 windsea_swell
 * (stokes_drift_profile_windsea_swell :418-456: needs the six ODR_VAR_SWELL_* / ODR_VAR_WIND_WAVE_* variables sampled,
 * hs_mode / tp_mode not used); hs_mode/tp_mode 0 environment, 1 from wind, 2 scalar default, tp_mode 3 from wind and
 * read back as float32 */
int odr_stokes_drift(odr_ctx *ctx, odr_particles *p, double dt, int profile, int hs_mode,
                     int tp_mode, double factor);
/* model-specific float32 element properties (slots 0..8); for LeewayObj (models/leeway.py:50-131):
 * 0 downwind_slope 1 crosswind_slope 2 downwind_offset 3 crosswind_offset 4 downwind_eps
 * 5 crosswind_eps 6 jibe_probability 7 orientation 8 capsized.  set: elements [offset, offset+count) */
int odr_particles_set_property(odr_ctx *ctx, odr_particles *p, int slot, int64_t offset, int64_t count,
                               const float *host);
int odr_particles_get_property(odr_ctx *ctx, odr_particles *p, int slot, float *host);
/* copy of property `slot` as it is now, on the device, for the next odr_history_record (ODR_HIST_PROPERTIES_FROM_SNAPSHOT);
 * valid until the set is appended to, compacted or sorted; a record of more elements than the copy holds reads the live slot */
int odr_particles_snapshot_property(odr_ctx *ctx, odr_particles *p, int slot);
/* The Leeway loop body between two compactions in ONE launch: Environment.get_environment of `var_ids` at t_epoch
 * (environment.py:499-923; the list must hold x/y_wind and x/y_sea_water_velocity) + drift:current_uncertainty /
 * drift:wind_uncertainty (:869-891; device RNG, 0 = none) + interact_with_coastline (basemodel/__init__.py:670-746) +
 * update_previous_state + Leeway.update (models/leeway.py:430-494, capsizing not included).  Elements the coastline
 * deactivates are flagged and not moved: call + odr_compact is bit-identical to odr_env_sample, odr_env_add_noise x 2,
 * odr_coastline, odr_compact, odr_leeway.  Returns ODR_SPLIT_LANE (1, not an error) when wind, current and land mask do not
 * come from one gridded reader: sampling, noise, coastline and previous state are then done, the caller compacts and calls
 * odr_leeway itself.  n_on_land == NULL: the count is not read back (no host synchronisation). */
enum { ODR_SPLIT_LANE = 1 };
/* report_missing_variables (basemodel/__init__.py:2501-2515) inside the NEXT odr_env_coast_leeway, between the sampling and
 * the coastline as in the loop: an element with NaN in a sampled variable whose fallback is None gets status `code` and does
 * not move (0 = no such test, the default).  One-shot: taken and reset by that call, fused launch or split lane alike. */
int odr_leeway_set_missing_code(odr_ctx *ctx, int32_t code);
int odr_env_coast_leeway(odr_ctx *ctx, odr_particles *p, int nvars, const int32_t *var_ids, double t_epoch, int coast_action,
                         int stranded_code, int seeded_on_land_code, int store_previous, double dt, double capsize_fraction,
                         double std_current, double std_wind, uint64_t step, int64_t *n_on_land);
/* processes:capsizing (models/leeway.py:438-455): call before odr_leeway.  host_uniforms (ODR_RNG_HOST): one number
 * per element, used by those that can be capsized */
int odr_leeway_capsize(odr_ctx *ctx, odr_particles *p, double dt, double wind_threshold, double wind_threshold_sigma,
                       int rng_mode, const double *host_uniforms, uint64_t step);
/* Leeway.update (models/leeway.py:430-494, after the capsizing block): leeway from wind, current,
 * jibing; host_uniforms[i] = np.random.random draws in ODR_RNG_HOST mode */
int odr_leeway(odr_ctx *ctx, odr_particles *p, double dt, double capsize_leeway_fraction, int rng_mode,
               const double *host_uniforms, uint64_t step);
/* horizontal_diffusion (basemodel/__init__.py:1746-1772) */
int odr_hdiffusion(odr_ctx *ctx, odr_particles *p, double dt, int rng_mode,
                   const double *host_nx, const double *host_ny, uint64_t step);
/* advect_wind -> stokes_drift -> horizontal_diffusion (physics_methods.py:712-791, :793-848, basemodel/__init__.py:1746-1772)
 * in ONE launch behind one reduction: `which` = 1 wind | 2 Stokes drift | 4 horizontal diffusion, applied in that order (the
 * reference's); every mover keeps its own arguments, checks and global early-out (a mover that returns early does not call
 * update_positions).  Same results as odr_advect_wind, odr_stokes_drift, odr_hdiffusion called one after the other: a single
 * mover bit for bit; in a chain the later moves form their start-point coefficients from the previous move's (positions equal
 * to the last bit or two of float64, tests/test_gpu_movers.py). */
int odr_movers(odr_ctx *ctx, odr_particles *p, double dt, int which, double wind_drift_depth, int relative_wind,
               double wind_factor, int stokes_profile, int hs_mode, int tp_mode, double stokes_factor, int rng_mode,
               const double *host_nx, const double *host_ny, uint64_t step);
/* OceanDrift.vertical_mixing (oceandrift.py:397-571), environment diffusivity profiles sampled at
 * the positions of the last odr_env_sample; host_uniforms[i_sub*n + i] in ODR_RNG_HOST mode */
int odr_vmix(odr_ctx *ctx, odr_particles *p, double t_epoch, double dt, double dt_mix,
             int mix_at_surface, int rng_mode, const double *host_uniforms, uint64_t step);
/* OceanDrift.vertical_mixing with a wind-parameterised diffusivity profile (oceandrift.py:385-395,425-458;
 * verticaldiffusivity_Large1994 / _Sundby1983, physics_methods.py:203-250): K from each element's wind speed and
 * ocean_mixed_layer_thickness on 1 m levels down to max(MLD)+1.  This is also what the default 'environment' model
 * does when no reader provides ocean_vertical_diffusivity (oceandrift.py:431-447).  Needs x_wind, y_wind,
 * ocean_mixed_layer_thickness, sea_floor_depth_below_sea_level (sea_surface_height) in the environment. */
enum { ODR_DIFFUSIVITY_LARGE1994 = 1, ODR_DIFFUSIVITY_SUNDBY1983 = 2 };
/* drift:truncate_ocean_model_below_m together with reader diffusivity profiles (environment.py:554-566): the reference narrows the
 * depth range it asks the reader for, and a reader that hands out the levels asked for (reader_netCDF_CF_generic.py:414-423,
 * reader_ROMS_native.py:551-560: the span of the request, one level more on either side, plus `verticalbuffer`) returns a block
 * CUT there -- elements below mix on K and dK/dz (np.gradient's edge of the cut grid) of the last level held.  n: levels of that
 * block, taken by the NEXT odr_vmix on the profiles of the device block (which always holds every level); 0 = all. */
int odr_vmix_set_profile_levels(odr_ctx *ctx, int32_t n);
int odr_vmix_wind_profile(odr_ctx *ctx, odr_particles *p, int model, double background_diffusivity, double dt,
                          double dt_mix, int mix_at_surface, int rng_mode, const double *host_uniforms,
                          uint64_t step);
/* OpenOil (models/openoil/openoil.py): the oil physics INSIDE the vertical-mixing loop.  Element properties live in
 * the property slots of odr_particles_set_property: */
enum { ODR_OIL_DIAMETER = 0, ODR_OIL_DENSITY = 1, ODR_OIL_VISCOSITY = 2, ODR_OIL_FILM_THICKNESS = 3,
       ODR_OIL_DIAMETER_IF_ENTRAINED = 4 /* written by odr_oil_prepare_mixing */ };
enum { ODR_DROPLETS_JOHANSEN2015 = 1, ODR_DROPLETS_LI2017 = 2 };   /* wave_entrainment:droplet_size_distribution */
/* OpenOil.prepare_vertical_mixing (openoil.py:1017-1031): entrainment probability after Li et al. 2017
 * (physics_methods.py:115-137) and one droplet diameter per element drawn from the Johansen et al. 2015 / Li et al.
 * 2017 spectrum (:1072-1172: 1e6-point log-normal around the MEAN median diameter of all elements, np.random.choice).
 * It also arms the next odr_vmix / odr_vmix_wind_profile call on `p`: that call then runs the loop as OpenOil does --
 * update_terminal_velocity in every sub-step (:922-998; elements.terminal_velocity is overwritten), surface_stick
 * (:1056-1061), surface_wave_mixing (:1033-1054; entrained elements take their new diameter unless
 * keep_droplet_diameter).  hs_mode / tp_mode as in odr_stokes_drift, plus tp_mode 3 = period from the wind as stored
 * in the float32 environment (physics_methods.py:876-883).  temperature_to_kelvin: oil_weathering_noaa's in-place
 * conversion (:722-724) has happened.  sea_water_density: PhysicsMethods.sea_water_density() (T=10, S=35).
 * ODR_RNG_HOST: host_u_diameter[n] (the uniforms behind np.random.choice), host_u_entrain[i_sub*n + i] (np.random.uniform(0,1)),
 * host_u_intrusion[i_sub*n + i] (unit draws of np.random.uniform(0, mean(1.5 Hs)) placed at the element they belong to). */
int odr_oil_prepare_mixing(odr_ctx *ctx, odr_particles *p, double dt, double dt_mix, double interfacial_tension,
                           double sea_water_density, int droplet_distribution, int keep_droplet_diameter, int hs_mode,
                           int tp_mode, int temperature_to_kelvin, int rng_mode, const double *host_u_diameter,
                           const double *host_u_entrain, const double *host_u_intrusion, uint64_t step);
int odr_oil_mixing_stats(odr_ctx *ctx, double *mean_zb, double *dv50);
/* Sharded run (one process per GPU): OpenOil takes two means over ALL elements -- np.mean(dV_50) of the droplet spectrum
 * (openoil.py:1099-1101,1156-1158) and np.mean(1.5 Hs) (:1047).  odr_oil_local_sums returns this rank's sums (the
 * float32 1.5 Hs summed in float64), the caller adds sums and element counts over the ranks and installs the means;
 * the next odr_oil_prepare_mixing uses them instead of reducing over its own elements. */
int odr_oil_local_sums(odr_ctx *ctx, odr_particles *p, double interfacial_tension, double sea_water_density,
                       int droplet_distribution, int hs_mode, double *sum_dv50, double *sum_zb);
int odr_oil_set_mixing_stats(odr_ctx *ctx, double mean_zb, double dv50);
/* PelagicEggDrift.update_terminal_velocity (models/pelagicegg.py:100-179; Sundby 1983): elements.terminal_velocity of every
 * active element from the sampled float32 sea_water_temperature / sea_water_salinity and two float32 property slots (egg
 * diameter [m], salinity of neutral buoyancy) -- Stokes' law, Dallavalle's empirical form where Re > 0.5, in the reference's
 * float32 operation order (csrc/odr_egg.hip.h).  ODR_ERR_STATE when temperature or salinity have not been sampled or a slot has
 * not been set.  Enqueued on the context's stream; no host synchronisation. */
enum { ODR_EGG_DIAMETER = 0, ODR_EGG_NEUTRAL_BUOYANCY_SALINITY = 1, ODR_EGG_DENSITY = 2, ODR_EGG_HATCHED = 3 };
int odr_egg_terminal_velocity(odr_ctx *ctx, odr_particles *p, int diameter_slot, int salinity_slot);
/* drift:use_tabularised_stokes_drift (models/basemodel/environment.py:844-863): sea_surface_wave_stokes_drift_{x,y}_velocity
 * (ODR_PLAST_STOKES) and / or sea_surface_wave_significant_height (ODR_PLAST_HS) of every active element from the sampled float32
 * x_wind / y_wind, as wave_stokes_drift_parameterised and wave_significant_height_parameterised form them
 * (models/physics_methods.py:488-527, :530-568): float64 wind speed capped at 30, np.polyval as a float64 Horner chain, one
 * rounding into the float32 environment (csrc/odr_plast.hip.h).  stokes_coeff: the n_stokes (1 .. 7) coefficients of the drift
 * factor for the configured fetch, leading one first; hs_coeff: the two of the wave height.  They are np.polyfit's over the
 * reference's tables and come from the caller.  The slots are allocated where they were not sampled.  ODR_ERR_STATE when the wind
 * has not been sampled.  One launch on the context's stream; no host synchronisation. */
enum { ODR_PLAST_STOKES = 1, ODR_PLAST_HS = 2 };
int odr_stokes_from_wind(odr_ctx *ctx, odr_particles *p, const double *stokes_coeff, int n_stokes, const double *hs_coeff, int flags);
/* What environment.py:847-858 asks before it replaces anything: out3 = the plain maxima of Stokes x, Stokes y and the wave height
 * over the active elements (-inf: not sampled, or no active element).  Slots of the movers' reduction (odr_reduce_scalars), behind
 * the sixteen that call hands out; ODR_ERR_INVALID while a reduction combined over the ranks of a sharded run is installed. */
int odr_reduce_wave_maxima(odr_ctx *ctx, odr_particles *p, double *out3);
/* PlastDrift.update_particle_depth with vertical_mixing:mixingmodel = 'analytical' (models/plastdrift.py:94-107): z of every
 * active element is drawn anew, z = -(K / w) E with K the sampled float32 ocean_vertical_diffusivity, w the float32 terminal
 * velocity (one float32 division, widened) and E a standard exponential: draws[i] for element i of the set (ODR_RNG_HOST: what
 * np.random.standard_exponential(n) gave, in the order of the set) or the device generator's (ODR_RNG_DEVICE: -log1p(-u) of the
 * uniform in [0, 1) from the element's Philox block of `step`).  A scale NumPy refuses (sign bit set and not NaN: ValueError
 * 'scale < 0') on ANY active element: ODR_ERR_INVALID and no z of the call changed.  Elements that are not active are not
 * touched.  ODR_ERR_STATE when the diffusivity has not been sampled.  Two launches; the host waits for the flag of the first. */
int odr_plast_depth(odr_ctx *ctx, odr_particles *p, int rng_mode, const double *draws, uint64_t step);
/* LarvalFish (models/larvalfish.py; Kvile et al. 2018).  The element properties of LarvalFishElement (:31-52) in the property
 * slots of odr_particles_set_property, float32 all seven: `hatched` (uint8 in the reference) holds 0 (egg) or 1 (larva).  The
 * terminal velocity of the model (:105-183) is odr_egg_terminal_velocity with these slot numbers. */
enum { ODR_LARVA_DIAMETER = 0, ODR_LARVA_NEUTRAL_BUOYANCY_SALINITY = 1, ODR_LARVA_STAGE_FRACTION = 2, ODR_LARVA_HATCHED = 3,
       ODR_LARVA_LENGTH = 4, ODR_LARVA_WEIGHT = 5, ODR_LARVA_SURVIVAL = 6 };
/* LarvalFish.update_fish_larvae with fish_growth (models/larvalfish.py:200-231, :185-198) over the active set: an egg
 * (hatched == 0) adds days_in_timestep / exp(3.65 - 0.145 T) to stage_fraction and hatches when the float32 sum is >= 1; every
 * larva, one hatched in this call included, grows `weight` (Folkvord 2005) and gets `length` from the new weight.  T: the sampled
 * float32 sea_water_temperature [deg C].  Eggs keep weight and length untouched.  The reference's float32 operation order
 * (csrc/odr_larval.hip.h).  ODR_ERR_STATE when the temperature has not been sampled or a slot has not been set.  Enqueued on the
 * context's stream; no host synchronisation. */
int odr_larval_update(odr_ctx *ctx, odr_particles *p, int stage_fraction_slot, int hatched_slot, int weight_slot, int length_slot,
                      double dt_seconds);
/* LarvalFish.larvae_vertical_migration (models/larvalfish.py:233-253): z of a larva becomes min(0, z + direction *
 * fraction_swimming * swim_speed(length) * dt_seconds) (Peck et al. 2006; float32 displacement, float64 sum); eggs are untouched.
 * direction: -1 (down: the reference's `self.time.hour < 12`) or +1, decided by the caller once per step.  ODR_ERR_STATE when a
 * slot has not been set.  No host synchronisation. */
int odr_larval_migrate(odr_ctx *ctx, odr_particles *p, int hatched_slot, int length_slot, double fraction_swimming,
                       double dt_seconds, int direction);
/* OceanDrift.solar_elevation (models/physics_methods.py:977-979 with solar_elevation :1036-1043 and hour_angle :1026-1033): the
 * solar elevation [deg] of every active element, out_host[0 .. n), float64.  What depends on the time only is the caller's, as
 * float64 scalars: declination_rad = deg2rad(solar_declination(time)) (:997-1010), time_offset_minutes = equation_of_time(time)
 * (:1013-1023), day_minutes = hour * 60 + minute + second / 60.  The element part is float64 in the reference's operation order
 * (csrc/odr_solar.hip.h).  Waits for the context's stream. */
int odr_solar_elevation(odr_ctx *ctx, odr_particles *p, double declination_rad, double time_offset_minutes, double day_minutes,
                        double *out_host);
/* LarvalFishExtended (models/larvalfish_extended.py).  The element properties of LarvalFishExtendedElement (:28-41) in the property
 * slots of odr_particles_set_property, float32 both: `hatched` (uint8 in the reference) holds 0 (egg) or 1 (larva). */
enum { ODR_LARVALX_STAGE_FRACTION = 0, ODR_LARVALX_HATCHED = 1 };
enum { ODR_LARVALX_DEPTH = 1, ODR_LARVALX_DVM = 2 };     /* biology:vertical_behavior_mode ('none' launches nothing: no call) */
/* LarvalFishExtended.update_fish_larvae (models/larvalfish_extended.py:292-318) over the active set: an egg (hatched == 0) adds
 * float32(increment) to stage_fraction -- increment = (dt / 86400) / egg:hatch_time_days, formed by the caller in float64 -- and
 * hatches when the float32 sum is >= 1; larvae are untouched.  ODR_ERR_STATE when a slot has not been set.  Enqueued on the
 * context's stream; no host synchronisation. */
int odr_larvalx_hatch(odr_ctx *ctx, odr_particles *p, int stage_fraction_slot, int hatched_slot, double increment);
/* LarvalFishExtended._apply_vertical_behavior (models/larvalfish_extended.py:206-290, with _target_into_band :188-200) in ONE
 * launch: z of every moving element goes towards its depth band by at most w_active * dt_seconds, then min(z, 0) and
 * max(z, -sea_floor_depth) with the sampled float32 depth.  mode ODR_LARVALX_DEPTH: band 0 for every element; ODR_LARVALX_DVM:
 * band 1 (day) where the element's solar elevation is > 0, else band 0 (night); the three time scalars are those of
 * odr_solar_elevation (ignored for ODR_LARVALX_DEPTH).  A band is its centre and its half-width
 * clamp(dz_rel * |centre|, dz_min, dz_max) (_compute_band_half_width, :177-186), formed by the caller.  active_only_hatched != 0:
 * the larva case, only elements whose hatched slot is 1 move and the others keep their z bits; 0: the phytoplankton case, every
 * element moves and hatched_slot is not read.  z_is_float32 != 0: the reference still holds z in float32 (no vertical mixing has
 * run) and its float32 roundings are reproduced (csrc/odr_larvalx.hip.h).  w_active <= 0 or dt_seconds <= 0 launches nothing
 * (:246-247).  ODR_ERR_STATE when sea_floor_depth_below_sea_level has not been sampled or the slot has not been set.  No host
 * synchronisation. */
int odr_larvalx_behave(odr_ctx *ctx, odr_particles *p, int hatched_slot, int mode, int active_only_hatched, int z_is_float32,
                       double band0_centre, double band0_half_width, double band1_centre, double band1_half_width, double w_active,
                       double dt_seconds, double declination_rad, double time_offset_minutes, double day_minutes);
/* OpenBerg (models/openberg.py; Keghouche et al. 2010).  The element properties of IcebergObj (:45-100) that differ between
 * elements in the property slots of odr_particles_set_property, float32 all six; the six coefficients (weight_coef, the four drag
 * coefficients, wave_drag_coef) are scalars of a call. */
enum { ODR_BERG_SAIL = 0, ODR_BERG_DRAFT = 1, ODR_BERG_LENGTH = 2, ODR_BERG_WIDTH = 3, ODR_BERG_X_VELOCITY = 4, ODR_BERG_Y_VELOCITY = 5 };
/* OpenBerg.roll_over (models/openberg.py:587-614; Wagner et al. 2017) over the active set: length >= width, the berg rolls where
 * width / (sail + draft) < sqrt(6 a (1 - a)), a = 900 / 1027, and thickness is split again into draft = H a and sail = H - draft --
 * for EVERY element, as in the reference (csrc/odr_berg.hip.h).  ODR_ERR_STATE when a slot has not been set.  Enqueued on the
 * context's stream; no host synchronisation. */
int odr_berg_roll_over(odr_ctx *ctx, odr_particles *p, int sail_slot, int draft_slot, int length_slot, int width_slot);
/* OpenBerg.advect_iceberg with surface currents (models/openberg.py:427-552; the forces :104-218) over the active set.  From the
 * sampled float32 environment (current, wind; where sampled: Stokes drift, sea-floor depth, sea-surface height, wave height, sea-ice
 * fraction and velocity -- otherwise the reference's fallbacks 10000 m and 0) and the four dimensions: grounding and degrounding
 * of `moving`, V0 from the no-acceleration formula, then the momentum balance (ocean and wind drag, wave radiation, Coriolis, sea
 * ice) integrated over dt_seconds with SciPy's solve_ivp (RK45, rtol 1e-3, atol 1e-6, scipy/integrate/_ivp/rk.py) over the velocity
 * vector of ALL elements in float64: one error norm, summed in a fixed order, is read back per attempt.  Grounded elements get
 * velocity 0; positions move along the geodesic as in odr_update_positions; the velocities go to the two velocity slots (float32).
 * sea_surface_wave_from_direction [deg] and sea_ice_thickness [m] are scalars (they have no variable id); wave_rad, stokes_drift,
 * coriolis, grounding: the configuration flags of the same names.  lat_is_float32: the reference's elements.lat is still a float32
 * array (until the first update_positions of a run) and the Coriolis parameter a float32 value.  n_attempts / n_rejected (NULL: not reported): Dormand-Prince
 * attempts made and rejected.  velocity_f64 (NULL: not reported): 2 n doubles on the host, the float64 velocities of the n active
 * elements in device order (x of all, then y of all) as the positions were moved with them.  ODR_ERR_INVALID for a slot outside
 * 0..8 or a NaN scalar.  ODR_ERR_STATE for slot 8 on a set whose ensemble diffusivity parks its member there, and when current or wind (or, with stokes_drift, the Stokes drift) have not been sampled,
 * a dimension slot has not been set, or the solve fails (error norm not finite, step size below 10 ulp of t, more than 10000
 * attempts).  After a failed solve the call is partly applied: `moving` holds the grounding and degrounding of this call, the
 * positions and the two velocity slots are untouched.  Synchronises with the host once per attempt. */
int odr_berg_advect(odr_ctx *ctx, odr_particles *p, int sail_slot, int draft_slot, int length_slot, int width_slot, int x_velocity_slot,
                    int y_velocity_slot, double weight_coef, double water_form_drag_coef, double water_skin_drag_coef,
                    double wind_form_drag_coef, double wind_skin_drag_coef, double wave_drag_coef, double wave_from_direction,
                    double sea_ice_thickness, int wave_rad, int stokes_drift, int coriolis, int grounding, int lat_is_float32,
                    double dt_seconds, int32_t *n_attempts, int32_t *n_rejected, double *velocity_f64);
/* ShipDrift (models/shipdrift.py; Soergaard & Vada 1998).  The element properties of ShipObject (:32-77) in the property slots of
 * odr_particles_set_property, float32 all eight: length, height, draft, beam [m], wind_drag_coeff (Cf), water_drag_coeff (Cd),
 * orientation (uint8 there: 0 left, 1 right of the downwind direction, held as 0.f / 1.f) and the index of the element's class in
 * the class table (a small integer held exactly). */
enum { ODR_SHIP_LENGTH = 0, ODR_SHIP_HEIGHT = 1, ODR_SHIP_DRAFT = 2, ODR_SHIP_BEAM = 3, ODR_SHIP_WIND_DRAG = 4, ODR_SHIP_WATER_DRAG = 5,
       ODR_SHIP_ORIENTATION = 6, ODR_SHIP_CLASS = 7 };
/* The class tables of ShipDrift on the device, kept with their count.  A class is a unique pair of the clipped float32 ratios
 * (beam / length, draft / length) of :220-227; its table holds what the reference's two LinearNDInterpolator objects (:137-145)
 * return for it at the 49 spectrum points omega = 2.25 + i (12 - 2.25) / 99 < 7 (:262-277): table[n_classes][49][2] doubles, F
 * then D.  The caller evaluates the interpolators (the coefficient table wforce.dat is data of the reference).  ODR_ERR_INVALID
 * for a NaN.  odr_ship_table_destroy waits for the context's stream. */
typedef struct odr_ship_table odr_ship_table;
int odr_ship_table_create(odr_ctx *ctx, const double *table, int n_classes, odr_ship_table **out);
int odr_ship_table_classes(const odr_ship_table *table, int32_t *n_classes);
int odr_ship_table_destroy(odr_ctx *ctx, odr_ship_table *table);
/* ShipDrift.update (models/shipdrift.py:216-343) over the active set, ONE launch (csrc/odr_ship.hip.h): update_positions with the
 * sampled float32 current (:230); wind force, 0 where the wind is calm (:234-245); the 100-point wave spectrum from period and
 * height (:256-265) and the trapezoid integrals of force and damping over it, with the class table below omega = 7 and f = 0.5,
 * d = 2 omega above (:267-287); the factors for long (Tm > 8.55) and medium (5.7 <= Tm <= 8.55) periods (:290-296); form drag,
 * wave direction = wind direction (wave_dir_from_stokes 0) or Stokes drift direction (1) -+ 20 degrees by orientation
 * (:299-317) -- the reference decides between the two for the whole call (both Stokes components have a maximum of exactly 0),
 * the caller does; four damping iterations (:321-334); update_positions with the float64 drift velocity (:337-339); elements
 * whose sampled land_binary_mask is 1 get status stranded_code (where it was 0) and moving = 0 (:342).  hs_mode: 0 wave height as
 * sampled, 1 from the wind; tp_mode: 0 the wave period in the slot of ODR_VAR 13 as sampled, 3 from the wind as stored to the
 * float32 environment -- the conventions of odr_stokes_drift / odr_oil_prepare_mixing.  A period of exactly 0 on an element (a
 * reader that does not cover it) gives that element no waves (F_wave = beta2 = 0); the reference's replacement by the mean of
 * the other elements' periods (physics_methods.py:936-939) is not built.  table: odr_ship_table_create's; the caller guarantees
 * that every class index is below its class count (the kernel clamps, it does not report).  stranded_code: positive.
 * ODR_ERR_INVALID for a slot outside 0..8 or given twice, a NaN dt_seconds, no table, a stranded_code <= 0, other modes.  ODR_ERR_STATE when a slot has
 * not been set, for slot 8 on a set whose ensemble diffusivity parks its member there, and when current, wind or land mask -- or
 * what the modes and wave_dir_from_stokes name -- have not been sampled.  intermediates_f64 (NULL: not reported): 10 n doubles on
 * the host, for the n active elements in device order: F_wave and beta2 before the period factors, F_wave, beta2, the wave
 * direction, F_total, uw_tot, uw_dir and the two components of the drift velocity (all n of one, then the next).  Enqueued on the
 * context's stream; no host synchronisation unless intermediates_f64 is given. */
int odr_ship_drift(odr_ctx *ctx, odr_particles *p, int length_slot, int height_slot, int draft_slot, int beam_slot, int wind_drag_slot,
                   int water_drag_slot, int orientation_slot, int class_slot, const odr_ship_table *table, int hs_mode,
                   int tp_mode, int wave_dir_from_stokes, int stranded_code, double dt_seconds, double *intermediates_f64);
/* performance hint: apply vertical_advection (oceandrift.py:315-350) inside the next odr_vmix
 * kernel (OceanDrift.update() calls them back to back, oceandrift.py:201-208) */
int odr_vmix_fuse_vertical_advection(odr_ctx *ctx, int at_surface);
/* vertical_advection (oceandrift.py:315-350) / vertical_buoyancy (:352-368) */
int odr_vertical_advection(odr_ctx *ctx, odr_particles *p, double dt, int at_surface);
int odr_vertical_buoyancy(odr_ctx *ctx, odr_particles *p, double dt);
/* update_previous_state (basemodel/__init__.py:642-668): store lon/lat for the 'previous'
 * coastline / seafloor actions.  Newly appended elements start with previous = own position
 * (release_elements, :925-929). */
int odr_store_previous(odr_ctx *ctx, odr_particles *p);
/* interact_with_coastline (basemodel/__init__.py:670-746, approximation precision None) and
 * interact_with_seafloor 'lift_to_seafloor' (:748-783) on the current environment */
int odr_coastline(odr_ctx *ctx, odr_particles *p, int action, int stranded_code,
                  int seeded_on_land_code /* 'previous': deactivate age==0 elements on land, 0 = off */,
                  int64_t *n_on_land);
/* interact_with_coastline with general:coastline_approximation_precision (basemodel/__init__.py:694-746): elements on
 * land are moved to the coastline found by coastline_crossing (:81-134) between their previous (odr_store_previous)
 * and current position -- first sample on land ('stranding') or last sample in water ('previous') of the reference's
 * sampling pattern with step `precision_deg`, evaluated on the landmask raster `landmask_source`. */
int odr_coastline_crossing(odr_ctx *ctx, odr_particles *p, int action, int stranded_code, int seeded_on_land_code,
                           double precision_deg, int32_t landmask_source, int64_t *n_on_land);
/* report_missing_variables (basemodel/__init__.py:2501-2515) on the result of the last odr_env_sample: elements for
 * which any of var_ids is NaN in the environment (Environment.get_environment's `missing`, environment.py:903-908)
 * are deactivated with status_code ('missing_data') */
int odr_deactivate_missing(odr_ctx *ctx, odr_particles *p, int nvars, const int32_t *var_ids,
                           int32_t status_code, int64_t *n_missing);
/* increase_age_and_retire (basemodel/__init__.py:2342-2352); max_age_seconds <= 0: no retirement */
int odr_increase_age(odr_ctx *ctx, odr_particles *p, double dt, double max_age_seconds, int retired_code);
int odr_seafloor(odr_ctx *ctx, odr_particles *p, int64_t *n_below);   /* 'lift_to_seafloor' */
/* the other general:seafloor_action values (:768-783): DEACTIVATE flags the element with status_code ('seafloor') and
 * puts it on the sea floor, PREVIOUS moves it back to the lon/lat of odr_store_previous (z unchanged) */
enum { ODR_SEAFLOOR_LIFT = 1, ODR_SEAFLOOR_DEACTIVATE = 2, ODR_SEAFLOOR_PREVIOUS = 3,
       /* SedimentDrift.bottom_interaction (models/sedimentdrift.py:108-116), the hook the reference calls behind
        * interact_with_seafloor() inside update() (oceandrift.py:364-368, :556-561): the element is put on the sea floor
        * and SETTLES -- moving = 0, status unchanged, it stays active and no mover moves it until odr_resuspend.
        * Accepted by odr_set_seafloor_action only (the main-loop interact_with_seafloor() never settles). */
       ODR_SEAFLOOR_SETTLE = 4,
       /* RadionuclideDrift.bottom_interaction (models/radionuclides.py:912-942) behind the same hook: an element below the
        * sea floor is lifted onto it, and SETTLES (as above) only if its species -- the small integer held in a float32
        * property slot -- is in a set, given as a bit mask over the species numbers 0 .. 6; any other element is only lifted
        * and keeps mixing.  The status_code of odr_set_seafloor_action carries both: ODR_SEAFLOOR_SPECIES(slot, mask).  The
        * species number itself is changed by odr_radio_resuspend.  Accepted by odr_set_seafloor_action only; odr_vmix* and
        * odr_vertical_buoyancy return ODR_ERR_STATE when the slot has not been set on their particle set. */
       ODR_SEAFLOOR_SETTLE_SPECIES = 5 };
#define ODR_SEAFLOOR_SPECIES(slot, mask) ((int32_t)(((mask) & 127) | ((slot) << 16)))
int odr_seafloor_action(odr_ctx *ctx, odr_particles *p, int action, int32_t status_code, int64_t *n_below);
/* The reference calls interact_with_seafloor() again INSIDE update(): from vertical_buoyancy (oceandrift.py:362-368)
 * and from every sub-step of vertical_mixing (:555-559).  This sets what odr_vertical_buoyancy / odr_vmix* do with an
 * element below the sea floor there (default ODR_SEAFLOOR_LIFT; 0 = 'none'; ODR_SEAFLOOR_SETTLE). */
int odr_set_seafloor_action(odr_ctx *ctx, int action, int32_t status_code);
/* SedimentDrift.resuspension (models/sedimentdrift.py:118-126): every element of the active set with moving == 0 whose
 * current speed -- np.sqrt(u**2 + v**2) of the sampled float32 x_sea_water_velocity / y_sea_water_velocity
 * (current_speed(), physics_methods.py:889-891) -- exceeds `threshold` (the configuration value as float32) gets
 * moving = 1 and z + 0.01 (float64).  *n_resuspended: how many (NULL: not counted, no host synchronisation).
 * ODR_ERR_STATE when the two current components have not been sampled (csrc/odr_sediment.hip.h). */
int odr_resuspend(odr_ctx *ctx, odr_particles *p, float threshold, int64_t *n_resuspended);
/* RadionuclideDrift (models/radionuclides.py).  Element properties in the float32 property slots: diameter,
 * neutral_buoyancy_salinity, density, and `specie` (int32 there): a small integer held exactly. */
enum { ODR_RADIO_DIAMETER = 0, ODR_RADIO_NEUTRAL_BUOYANCY_SALINITY = 1, ODR_RADIO_DENSITY = 2, ODR_RADIO_SPECIE = 3 };
enum { ODR_RADIO_MAX_SPECIES = 7, ODR_RADIO_MAX_SALINITY_INTERVALS = 4 };
/* What init_species / init_transfer_rates (:233-278, :512-654) and the configuration give the device.  Species numbers are -1
 * where the setup has none: either lmm (the four 'LMM + ...' setups) or lmmcation, lmmanion and polymer ('LMM + Colloid + Rev')
 * are set.  rates[a][in][out] in 1/s, a = 0 for the LMM setups (nsalinity 1), the four salinity intervals (0,1], (1,10],
 * (10,20], (20,inf) of :597-644 for the other (nsalinity 4); only [nsalinity][nspecies][nspecies] is read.  lognormal: 0
 * radionuclide:particlesize_distribution 'normal', 1 'lognormal'.  The remaining members are the radionuclide:* configuration
 * values of the same names (diameter_uncertainty: particle_diameter_uncertainty). */
typedef struct {
  int32_t nspecies, nsalinity, lognormal;
  int32_t lmm, lmmcation, lmmanion, polymer, particle_rev, sediment_rev, particle_slow, sediment_slow, particle_irrev, sediment_irrev;
  double rates[4 * 7 * 7];
  double layer_thick, particle_diameter, dissolved_diameter, diameter_uncertainty, desorption_depth, desorption_depth_uncert,
      resuspension_depth, resuspension_depth_uncert, resuspension_critvel;
} odr_radio_setup;
/* The setup on the device, with the counters ntransformations[in][out] (:528), which the launches below add to.
 * ODR_ERR_INVALID for species numbers outside the table, a rate that is negative or not finite, a NaN.
 * odr_radio_counts: counts49[in * 7 + out] since creation or the last reset (reset != 0 clears them); waits for the context's
 * stream; ODR_ERR_STATE (after filling counts49) when a launch met an element whose species number is outside 0 .. nspecies - 1
 * -- such an element is left unchanged, nothing is read outside the table.  odr_radio_destroy waits for the context's stream. */
typedef struct odr_radio odr_radio;
int odr_radio_create(odr_ctx *ctx, const odr_radio_setup *setup, odr_radio **out);
int odr_radio_counts(odr_ctx *ctx, odr_radio *radio, int64_t *counts49, int reset);
int odr_radio_destroy(odr_ctx *ctx, odr_radio *radio);
/* update_transfer_rates + update_speciation (models/radionuclides.py:728-810) with update_radionuclide_diameter (:866-902, and
 * set_init_diameter :281-315), sorption_to_sediments (:814-830) and desorption_from_sediments (:834-860), over the active set in
 * ONE launch (csrc/odr_radio.hip.h).  The element's row of the rate table -- by species, for nsalinity 4 also by
 * np.searchsorted([0,1,10,20], S) - 1 of the sampled float32 salinity, S <= 0 taking the last table as the index -1 does there;
 * for an LMM element the rate to sediment is 0 further than layer_thick above the sea bed and the rate to particles is scaled by
 * conc3 / 1e-3, conc3 being the sampled float32 variable conc3_var (the variable has no id of its own: the caller names the slot
 * it rides); p = 1 - exp(-k dt) in float64; the element transforms when u1 < sum(p), to species
 * searchsorted(cumsum(p / sum(p)), u2), clamped to the last species with p > 0 where rounding pushes it past the table (the
 * reference stores the number nspecies there and fails on it a step later).  A new particle / dissolved element gets
 * particle_diameter / dissolved_diameter + noise (lognormal: * noise) rounded to float32, without the reference's clipping,
 * which assigns into a copy; a diameter of 0 gets none.  LMM(cation) -> sediment reversible: z = -depth, moving = 0; the reverse:
 * z = float32(-depth + desorption_depth) + N(0, desorption_depth_uncert), moving = 1, possibly below the sea floor as there.
 * z > 0 becomes 0 (the reference does that only in a step in which some element transforms).  Only elements that change are
 * written.  ODR_RNG_HOST: u1, u2 uniform in [0, 1), diameter_noise and depth_noise the values the reference ADDS (or multiplies
 * with), one per element of the active set in device order; ODR_RNG_DEVICE (the four pointers are not read): Philox streams keyed
 * by (ID, step).  ODR_ERR_STATE when a slot has not been set or depth, conc3 (LMM setups) or salinity (nsalinity 4) have not been
 * sampled.  No host synchronisation in ODR_RNG_DEVICE mode. */
int odr_radio_speciation(odr_ctx *ctx, odr_particles *p, odr_radio *radio, int specie_slot, int diameter_slot, int32_t conc3_var,
                         double dt_seconds, int rng_mode, const double *u1, const double *u2, const double *diameter_noise,
                         const double *depth_noise, uint64_t step);
/* update_terminal_velocity without profiles (models/radionuclides.py:665-721): Stokes' law W = (1/mu)(1/18) g d^2 (rho_w - rho)
 * from the sampled float32 temperature and salinity and the diameter and density slots, times moving, in the reference's
 * float32 operation order.  ODR_ERR_STATE when temperature or salinity have not been sampled or a slot has not been set. */
int odr_radio_terminal_velocity(odr_ctx *ctx, odr_particles *p, int diameter_slot, int density_slot);
/* bottom_interaction's change of species (models/radionuclides.py:912-942) for the elements ODR_SEAFLOOR_SETTLE_SPECIES has
 * settled -- moving == 0 with a particle species: the matching sediment species, counted -- and then resuspension (:946-997):
 * every element with z <= -depth and float32 sqrt(u^2 + v^2) >= resuspension_critvel, whatever its species, gets moving = 1 and
 * z = float32(-depth + resuspension_depth) + N(0, resuspension_depth_uncert); z > 0 becomes 0; the three sediment species become
 * the matching particle species, counted, with the diameter update of odr_radio_speciation.  ODR_RNG_HOST: the two noise arrays
 * as there.  ODR_ERR_STATE when the current or the depth have not been sampled or a slot has not been set. */
int odr_radio_resuspend(odr_ctx *ctx, odr_particles *p, odr_radio *radio, int specie_slot, int diameter_slot, int rng_mode,
                        const double *diameter_noise, const double *depth_noise, uint64_t step);
/* OpenOil's NOAA oil weathering (models/openoil/openoil.py:717-920, noaa_oil_weathering.py, csrc/odr_weather.hip.h) from an oil given as
 * a TABLE of pseudo-components.  The state lives in a side table the particle set owns, one record and one row of mass_components
 * per element, indexed by element ID like the reference's noaa_mass_balance (:682-693): compaction, the re-sort and the property
 * slots do not touch it.  The record is float64 like the reference's arrays at that point of the step. */
enum { ODR_OIL_MAXCOMP = 32 };
enum { ODR_WEATHER_PROPERTIES = 1,        /* the emulsion's density and viscosity and fraction_evaporated (:741-759) */
       ODR_WEATHER_EVAPORATION = 2,       /* evaporation_noaa (:822-853), elements with z == 0 */
       ODR_WEATHER_EMULSIFICATION = 4,    /* emulsification_noaa (:855-920), elements behind the bullwinkle test */
       ODR_WEATHER_DISPERSION = 8,        /* disperse_noaa (:792-815), every element */
       ODR_WEATHER_BIO_HALF_TIME = 16,    /* biodegradation_half_time (:568-586) */
       ODR_WEATHER_BIO_ADCROFT = 32 };    /* biodegradation_adcroft (:588-611) */
typedef struct odr_oil_table {
  int32_t ncomp;                /* 1 .. ODR_OIL_MAXCOMP */
  int32_t mwf_n;                /* entries of max_water_fraction (one entry of the reference's max_water_fraction.json): 0, 1 or 2 */
  /* per component, formed by the caller with the reference's NumPy expressions (adios/oil.py:155-166, noaa_oil_weathering.py:26):
   * [0] D_S * (bp - C_2i)**2 / (D_Zb * R_cal * bp), [1] C_2i, [2] 1 / (bp - C_2i), [3] molecular_weight / 1000 */
  double comp[4 * ODR_OIL_MAXCOMP];
  double density, density_ref_temp, density_k;         /* rho(T) = density - density_k (T - density_ref_temp) */
  double viscosity, viscosity_ref_temp, viscosity_B;   /* nu(T) = viscosity exp(B / T - B / viscosity_ref_temp) */
  double bulltime, bullwinkle, y_max;                  /* adios/oil.py:123-140 */
  double mwf_t[2], mwf_w[2];                           /* temperatures [deg C] and max water fractions */
  double sea_water_density;                            /* PhysicsMethods.sea_water_density() (T = 10, S = 35) */
} odr_oil_table;
/* prepare_run (:682-693): the table and a zeroed side table for n_total elements; replaces an earlier one of the particle set, which
 * frees it with odr_particles_destroy.  ODR_ERR_INVALID for more than ODR_OIL_MAXCOMP components, a NaN, other mwf_n. */
int odr_oil_weathering_setup(odr_ctx *ctx, odr_particles *p, const odr_oil_table *table, int64_t n_total);
/* seed_elements and prepare_run (:1726-1755, :686-691) for the rows [id0, id0 + n): records[n][14] in the order of
 * odr_oil_weathering_get's names (the 14th value is padding), rows[n][ncomp] = mass_fraction * mass_oil */
int odr_oil_weathering_seed(odr_ctx *ctx, odr_particles *p, int64_t id0, int64_t n, const double *records, const double *rows);
/* oil_weathering_noaa over the active set (:717-790), `flags` a sum of ODR_WEATHER_*: one reduction for the call-wide decisions --
 * no surface element or the youngest older than 24 h stops evaporation (:828-834), min(Y_max - sintef) > 0 over the elements that
 * start to emulsify lets max_water_fraction override Y_max (:888), wave height and period come from the samples when any is > 0,
 * else from the wind (physics_methods.py:893-943), a zero period takes the mean of the others (:936-939) -- whose results stay on
 * the device, then ONE launch: Kelvin conversion (:722-724, kept to the launch: the sampled temperature is not rewritten), property
 * update, evaporation, emulsification, dispersion, biodegradation.  Needs x_wind, y_wind and sea_water_temperature sampled and
 * the property slots ODR_OIL_DENSITY / ODR_OIL_VISCOSITY set: it stores the emulsion's values there rounded to float32, for the
 * mixing kernels.  Without ODR_WEATHER_PROPERTIES the launch works on the stored density, viscosity and fraction_evaporated (a
 * replay from the state in front of one process).  No host synchronisation.  ODR_ERR_STATE without a table or when an element's
 * ID has no row. */
int odr_oil_weather(odr_ctx *ctx, odr_particles *p, double dt_seconds, int flags);
/* one variable of the side table by element ID: out[n_total] for "mass_oil", "mass_evaporated", "mass_dispersed", "mass_biodegraded",
 * "fraction_evaporated", "water_fraction", "interfacial_area", "density", "viscosity", "bulltime", "biodegradation_half_time_droplet",
 * "biodegradation_half_time_slick", "oil_film_thickness"; out[n_total][ncomp] for "mass_components" (noaa_mass_balance, :689-691);
 * out[8] for "reduction": what the last odr_oil_weather decided on (surface elements, their least age, min(Y_max - sintef), the
 * maxima of wave height and period, the least period, sum and count of the periods > 0).  _set: all but "reduction". */
int odr_oil_weathering_get(odr_ctx *ctx, odr_particles *p, const char *name, double *out);
int odr_oil_weathering_set(odr_ctx *ctx, odr_particles *p, const char *name, const double *in);
/* get_oil_budget's sums at this moment (:1241-1306): out[8] = mass_surface, mass_submerged, mass_stranded, mass_evaporated,
 * mass_dispersed, mass_biodegraded, mass_total, elements counted.  Active elements and the deactivated store are counted, the
 * latter with the masses, depth and status they left with (the reference forward-fills its result).  One device reduction with a
 * fixed fold order: two runs agree bit for bit.  Waits for the stream. */
int odr_oil_budget(odr_ctx *ctx, odr_particles *p, int32_t stranded_code, double *out);
/* number of active-set elements currently flagged with status_code (not yet removed by odr_compact) */
int odr_particles_count_status(odr_ctx *ctx, odr_particles *p, int32_t status_code, int64_t *n);
/* status_categories grow in the order in which reasons FIRST OCCUR (deactivate_elements, :1778-1781): a caller hands
 * out a provisional code for a reason not seen yet, counts it, and renumbers it once the category index is known.
 * Renumbering one reason into another leaves the active set alone; from_code or to_code 0 deactivates / re-activates
 * elements (their `moving` flag is not touched) and counts as such: the cached reductions and the counts of
 * odr_scan_status are void afterwards */
int odr_particles_remap_status(odr_ctx *ctx, odr_particles *p, int32_t from_code, int32_t to_code);
/* deactivate elements flagged by the host (deactivate_elements, :1774-1795) */
int odr_deactivate(odr_ctx *ctx, odr_particles *p, const uint8_t *mask_host, int32_t status_code);
/* remove_deactivated_elements (:1797-1826) = LagrangianArray.move_elements (elements.py:197-228):
 * stable compaction of status==0 elements, the rest appended to the deactivated store */
/* deactivate_outside (basemodel/__init__.py:2354-2382): drift:deactivate_west_of/east_of/south_of/north_of;
 * a NaN bound is "not set" */
int odr_deactivate_outside(odr_ctx *ctx, odr_particles *p, double west, double east, double south, double north,
                           int32_t status_code);
int odr_compact(odr_ctx *ctx, odr_particles *p, int64_t *n_active);
/* odr_compact in two halves, for a loop that needs the deactivation state on the host once per step:
 * odr_scan_status counts the elements that stay and reports which PROVISIONAL status numbers are present (bit k of
 * *status_flags: some element carries status 100 + k -- a deactivation reason without a status category yet, which the
 * caller registers and renumbers with odr_particles_remap_status, basemodel/__init__.py:1778-1781) in ONE host read;
 * odr_compact_apply then removes the deactivated elements without another read.  No call that deactivates, adds or
 * re-orders elements may run in between (ODR_ERR_STATE otherwise). */
int odr_scan_status(odr_ctx *ctx, odr_particles *p, int64_t *n_kept, uint64_t *status_flags);
/* The same read in two halves, so that the loop's next launch need not wait for the host (round 5).  After
 * odr_env_coast_advect, odr_scan_status_begin enqueues the fold of the counts that launch left and returns at once (1 = that
 * launch left none -- another path ran --: call odr_scan_status instead); the device also keeps the verdict "every element
 * stays".  odr_ctx_guard_next_vmix(ctx, 1) makes the NEXT odr_vmix a launch that does nothing unless that verdict is "yes":
 * the mixing of the step (oceandrift.py:397-571) is enqueued BEFORE the host knows whether remove_deactivated_elements
 * (basemodel/__init__.py:2284) has anything to remove -- in the common step it has not, and the device goes from the step
 * launch into the mixing launch without waiting for the host; otherwise the host compacts and calls odr_vmix again, unguarded
 * (the guarded launch has not touched anything, and odr_scan_status_end re-arms the odr_vmix_fuse_vertical_advection setting it
 * took, for that call: the retry is expected -- a caller that skips it leaves the setting armed for its next odr_vmix).  A guarded odr_vmix that cannot honour the guard (host-drawn numbers, or
 * another kernel family than the reader-profile fast path: OpenOil's loop, profiles sampled in the float32 position class, a
 * level cut) launches nothing, leaves the one-shot settings of odr_vmix_fuse_vertical_advection, odr_vmix_set_profile_levels
 * and odr_oil_prepare_mixing armed for the unguarded call, and returns 1.  odr_vmix_wind_profile carries no guard: it drops an
 * armed one.  odr_scan_status_end waits for the fold only (not for the mixing launch behind it) and hands out what
 * odr_scan_status would have. */
int odr_scan_status_begin(odr_ctx *ctx, odr_particles *p);
int odr_scan_status_end(odr_ctx *ctx, odr_particles *p, int64_t *n_kept, uint64_t *status_flags);
int odr_ctx_guard_next_vmix(odr_ctx *ctx, int on);
int odr_compact_apply(odr_ctx *ctx, odr_particles *p, int64_t *n_active);
/* Device-side layout operation with no reference counterpart: re-order the particle arrays by
 * the grid cell of gridded source `source_id` so that the lanes of a wavefront gather
 * neighbouring grid nodes.  Particles keep their ID; results per ID are unchanged (the device
 * RNG is counter-based on ID).  Do not use together with ODR_RNG_HOST arrays, which are
 * indexed by position. */
int odr_sort_particles(odr_ctx *ctx, odr_particles *p, int32_t source_id);
/* keep_environment = 0: the sampled environment and the sample position are not carried along (the next odr_env_sample /
 * odr_env_coast_advect rewrites them for every element): a re-sort at the top of a step moves half the bytes */
int odr_sort_particles_ex(odr_ctx *ctx, odr_particles *p, int32_t source_id, int keep_environment);
/* The sort also leaves a table of workgroup ranges (each inside one 8x8-cell sort tile): while it is valid (no element
 * appended since), odr_env_coast_advect with a Runge-Kutta scheme on a lon/lat or polar-stereographic reader runs its
 * launch with the node records of each workgroup's rectangle staged in LDS (csrc/odr_tile.hip.h) -- same bits as the
 * launch that gathers from the blocks in HBM.  Diagnostics of that path since the set was created:
 * out4 = {launches that took the LDS-tile path, elements handed to the HBM path by those launches (footprint outside their
 *         workgroup's rectangle), workgroups whose rectangle was cut to the LDS capacity, ranges in the current table}.
 * Synchronises the context's stream. */
int odr_particles_tile_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out4);
/* The fused step launch of odr_env_coast_advect (csrc/odr_kernels.hip.h k_step_grid) since the set was created:
 * out2 = {launches other than those of the C3 group's two-level static layout (the run-time layout, and the on-level
 *         static layout counted by odr_particles_step_onlevel_stats), launches of the instantiation whose layout is the
 *         C3 group between two time levels as compile-time constants (under ODR_STAGE_FAST: csrc/odr_field.hip.h LayoutC3)}.
 * The environment variable ODR_NO_LAYOUT_SPEC=1 keeps every launch on the run-time layout. */
int odr_particles_step_layout_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out2);
/* The launches of the same kernel with the C3 group's static layout on a step whose time sits on a reader level
 * (csrc/odr_field.hip.h LayoutC3L1) since the set was created: out1 = {launches}.  They are part of out2[0] above. */
int odr_particles_step_onlevel_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out1);
/* The mixing launches of odr_vmix since the set was created:
 * out3 = {launches of the K-column kernel (csrc/odr_kernels.hip.h k_vmix_col) that read its configuration at run time, launches
 *         of its instantiation for C3's configuration as compile-time constants (VMixC3), launches of the other mixing kernels
 *         (the five-level window, the generic and OpenOil kernels)}.
 * The environment variable ODR_NO_VMIX_SPEC=1 keeps every column launch on the run-time configuration. */
int odr_particles_vmix_layout_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out3);
/* Where the K-column and five-level-window launches of odr_vmix gathered the diffusivity from since the set was created:
 * out2 = {launches that read the levels' K planes (every resident level of the K source has one, see odr_block_kplane_read),
 *         launches that read the node records}.
 * The environment variable ODR_NO_KPLANE=1 keeps every launch on the node records (the planes are still written). */
int odr_particles_vmix_kplane_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out2);
/* The launches of the K-column kernel for C3's static configuration on a 12-level column (counted in out3[1] of
 * odr_particles_vmix_layout_stats) since the set was created:
 * out3 = {launches that gathered two of the column's three K quads per particle (csrc/odr_kernels.hip.h VMixC3W), launches that
 *         gathered the whole column, elements the two-quad launches redid on the whole column because a sub-step left the
 *         resident levels (read from the device: waits for the stream)}.
 * The environment variable ODR_NO_VMIX_WINDOW=1 keeps every such launch on the whole column. */
int odr_particles_vmix_window_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out3);
/* The launches of the K-column kernel (k_vmix_col, every configuration) since the set was created.  A workgroup of that kernel
 * owns a tile of 4 x 256 consecutive elements, leaves out those the launch cannot change -- z == 0 on entry while the call does
 * not mix at the surface, does not advect the surface vertically and the sea floor is not above the surface: the launch stores
 * z = +0.0 for them whatever their column holds -- and mixes the rest densely packed:
 * out2 = {tiled launches, elements they skipped (read from the device: waits for the stream)}.
 * The environment variable ODR_NO_VMIX_SKIP=1 keeps the tiling and skips no element. */
int odr_particles_vmix_skip_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out2);
/* A static configuration of that kernel whose settings allow the skip compacts the whole launch instead of each tile: three small
 * kernels build one ascending list of the elements to mix on the device, and a one-element-per-thread launch (k_vmix_dense)
 * runs over it; its grid covers every element, the list's length is never read back.  Such a launch counts as a tiled launch
 * in odr_particles_vmix_skip_stats too, and its skipped elements count there.
 * out2 = {dense launches, elements they listed (read from the device: waits for the stream)}.
 * The environment variable ODR_NO_VMIX_DENSE=1 keeps the tiled launch. */
int odr_particles_vmix_dense_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out2);
/* Where the dense launches took their keep ballots from.  A static-layout step launch of odr_env_coast_advect that lifts to the
 * sea floor with the depth in its group forms them as it goes; odr_vmix uses them when nothing that changes z, the depth, the
 * ssh, the order or the count of the elements has run in between (odr_scan_status_begin / _end and odr_ctx_guard_next_vmix
 * leave them valid), and makes its own pass over the three arrays (k_vmix_keep) otherwise.  A list that holds every element is
 * not filled: the mixing launch takes the indices 0 .. n - 1 itself.
 * out3 = {dense launches on the step launch's ballots, dense launches on k_vmix_keep's, lists of every element (read from the
 * device: waits for the stream)}.
 * Results and the counters of odr_particles_vmix_skip_stats / _dense_stats are the same on either producer's ballots (a skipped
 * element that holds -0.0 included: the step launch marks its wave, and the list kernels store the +0.0 a mixing call that
 * walks a sub-step hands back).
 * The environment variable ODR_NO_STEP_KEEP=1 (read per odr_env_coast_advect call) leaves the ballots to k_vmix_keep. */
int odr_particles_vmix_keep_stats(odr_ctx *ctx, odr_particles *p, uint64_t *out3);
/* counts and min/max used for the per-step log line and early-outs (:2212-2233):
 * out16 = {n_active, lon_min, lon_max, lat_min, lat_max, z_min, z_max, D_max, stokes_sum_max,
 *          wind_speed_max, wdf_surface_max, n_surface, hs_max, tp_max, rel_wind_speed_max, mld_max}
 * over the elements with status 0 (deactivated, not yet compacted ones do not count); a maximum of nothing -- no such
 * element, the variable not sampled, no element at the surface -- is -inf, a minimum +inf; NaN values are ignored.  The
 * wind slots (9, 10, 11, 14) run over the elements with z >= -|wind_drift_depth|; relative_wind is 0 here, so slot 14
 * equals slot 9.  Always a pass over the arrays (never the cache); like odr_reduce_local it releases installed values
 * (odr_reduce_install), which it overwrites. */
int odr_reduce_scalars(odr_ctx *ctx, odr_particles *p, double wind_drift_depth, double *out16);
/* The global tests the movers open with -- no element at the surface, wind_drift_factor / (relative) wind speed / Stokes
 * drift / horizontal diffusivity identically zero (physics_methods.py:741-747,771-780,799-804, basemodel/__init__.py:1754)
 * -- formed by the launch of odr_env_coast_advect, which holds every value they read in registers, instead of by a pass of
 * its own over the arrays before the first mover (persistent setting; off by default).  The movers that follow
 * (odr_movers, odr_advect_wind with the same wind_drift_depth / relative_wind, odr_stokes_drift, odr_hdiffusion) take the
 * tests from there as long as nothing they depend on changed in between (a compaction does not; vertical mixing does:
 * the pass is then made as before).  Same results either way (tests/test_gpu_movers.py). */
int odr_ctx_set_step_reduce(odr_ctx *ctx, int on, double wind_drift_depth, int relative_wind);
/* The same reductions for a run sharded over several GPUs (one process per GPU): odr_reduce_local returns the RAW slots
 * of this particle set (0 and 11 are counts, every other slot a maximum; minima negated), the caller combines them over
 * the ranks (sum / max: an all-reduce of 16 doubles) and installs the result; until odr_reduce_unpin the movers
 * (odr_advect_wind, odr_stokes_drift, odr_hdiffusion, odr_vmix_wind_profile) use the installed values -- their global
 * early-outs and MLD.max() are then those of the reference's single process, independent of the number of ranks. */
int odr_reduce_local(odr_ctx *ctx, odr_particles *p, double wind_drift_depth, int relative_wind, double *out16);
int odr_reduce_install(odr_ctx *ctx, odr_particles *p, const double *in16);
int odr_reduce_unpin(odr_ctx *ctx);
/* What the last mover on this context read: the 16 RAW slots as they stand on the device (nothing is reduced), and what
 * the cache says about them -- *state bit 0: they describe `p` in its present state (a mover on `p` would reuse them),
 * bit 1: the lon / lat / z extremes (slots 1..6) are filled (the movers' own pass leaves them at -inf), bit 2: formed by
 * the launch of odr_env_coast_advect (odr_ctx_set_step_reduce): slots 7, 8, 10, 14 hold +1 / 0 / -inf for "some element
 * > 0" / "none > 0, some == 0" / "neither", slot 11 the count, the others nothing; bit 3: installed (odr_reduce_install).
 * For tests and diagnostics; waits for the stream. */
int odr_reduce_cached(odr_ctx *ctx, odr_particles *p, double *out16, int32_t *state);

/* Until the first update_positions of a run the reference's elements.lon / lat are float32 ARRAYS (elements/elements.py:71-88),
 * so modulate_longitude (readers/basereader/variables.py:259-280, called on the elements' longitudes :914) forms
 * np.mod(lon + 180, 360) - 180 in float32 in the FIRST get_environment: the readers are sampled at lon on the float32 grid of
 * lon + 180 (up to 8e-6 deg off).  f32 != 0: the main-loop samples that follow (odr_env_sample, odr_env_coast_advect,
 * odr_env_coast_leeway; not the Runge-Kutta stage calls, whose positions are float64 there) do the same; 0 ends it. */
int odr_ctx_set_position_class(odr_ctx *ctx, int f32);
/* The reader's x / y coordinate arrays are float32: in the float32 position class the index maps of a GEOGRAPHIC reader --
 * (x - xgrid[0]) / (xgrid[-1] - xgrid[0]) * (len - 1), interpolators.py:110-111, and the nearest-node map :32-37 -- are then
 * float32 arithmetic as well (x is the float32 longitude itself); projected readers get float64 x, y from pyproj. */
int odr_source_set_coordinate_dtype(odr_ctx *ctx, int32_t source_id, int x_is_float32, int y_is_float32);

/* ---------------------------------------------------------------- communication of a sharded run
 * One process per GPU; the reference has no multi-process mode (docs/source/performance.rst:22,36 suggests running several
 * simulations side by side), so there is no reference call to mirror: these are the three entry points SURVEY.md 8(b) lists
 * (odr_comm_init, odr_block_broadcast, odr_allreduce_scalars) plus the step's one collective.  They run over RCCL (librccl.so.1,
 * opened on first use; csrc/odr_comm.hip) -- no torch in the process.  ONE communicator pair per process: `step` for the small
 * collectives of the loop, `bulk` for reader levels (operations on one communicator execute in issue order; a 200 MB level
 * must not hold the step's 200-byte summary behind it).  Every rank makes the same calls in the same order. */
#define ODR_COMM_ID_BYTES 256
int odr_device_count(int32_t *n);
/* rank 0: the id of a new job (two ncclUniqueIds); the host hands it to the other ranks (opendrift_amd/distributed.py: a file) */
int odr_comm_unique_id(uint8_t *id /* [ODR_COMM_ID_BYTES] */);
/* ncclCommInitRank x 2 on the context's device; collective over all ranks */
int odr_comm_init(odr_ctx *ctx, const uint8_t *id, int32_t rank, int32_t nranks);
/* nranks = 0: no communicator.  id_hash: the same number on every rank of one job; collectives: calls made so far */
int odr_comm_info(int32_t *rank, int32_t *nranks, uint64_t *id_hash, int32_t *rccl_version, uint64_t *collectives);
int odr_comm_destroy(void);
/* in place, blocking; op 0 sum | 1 min | 2 max (counts of elements, extents; environment.py / basemodel bookkeeping over ALL elements) */
int odr_allreduce_scalars(odr_ctx *ctx, double *values, int32_t n, int32_t op);
/* THE collective of a sharded step, in two halves: every rank's row of n float64, gathered as [nranks][n].  _begin enqueues
 * (copy in, ncclAllGather, copy out into page-locked memory) on the communication stream and returns; _end waits.
 * from_scan != 0 (between odr_scan_status_begin and _end): row[0] = elements that stay and row[1..8] = status flags are
 * taken ON THE DEVICE from the fold of the step's status scan -- the collective starts when the device has the counts, not
 * when the host has read them; the mixing launch of the step runs meanwhile. */
int odr_comm_allgather_begin(odr_ctx *ctx, const double *row, int32_t n, int32_t from_scan);
int odr_comm_allgather_end(odr_ctx *ctx, double *rows /* [nranks][n] */);
/* host bytes (metadata of a reader level, pickled by the host mirror) from root to every rank; blocking; same nbytes everywhere */
int odr_comm_broadcast_bytes(odr_ctx *ctx, void *buf, int64_t nbytes, int32_t root);
int odr_comm_barrier(odr_ctx *ctx);
/* One reader time level (= one ReaderBlock, interpolation/structured.py:15-94) from the rank that runs the host Reader to
 * every rank: odr_block_upload_async with ONE ncclBroadcast of the level's staged float32 arrays in it (in place in the
 * upload pipeline's staging memory, on the upload stream, bulk communicator) -- `data` is read on `root` only (NULL
 * elsewhere), shapes and geometry are given by every rank.  Staged like an asynchronous upload: odr_block_commit makes it
 * current (a period later, when it is due). */
int odr_block_broadcast(odr_ctx *ctx, int32_t source_id, int32_t slot, double t_epoch, int nvars, const int32_t *var_ids,
                        const void *const *data, const int32_t *var_nz, int ny, int nx, const double *xy8, int32_t root);

/* kernel timing hook for bench.py: HIP events recorded on the context stream around the
 * launches issued between begin and end; returns milliseconds */
int odr_timer_begin(odr_ctx *ctx);
int odr_timer_end(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- output history
 * state_to_buffer (basemodel/__init__.py:2384-2499) and the float32 result buffer it fills
 * (:2084-2105): every exported variable is a float32 [trajectory, time] array initialised with NaN;
 * at an output time all elements present are written at (ID, time) -- float64 / int32 properties are
 * cast to float32 by the assignment -- and between output times only the deactivated elements are,
 * into the slot of the next output time (:2390-2397).  The buffer stays in HBM; a flush copies it to
 * pinned host memory on a second stream while the simulation continues.
 * Variable codes: an ODR_VAR_* id (environment variable) or one of ODR_HIST_*. */
enum {
  ODR_HIST_LON = 1000, ODR_HIST_LAT, ODR_HIST_Z, ODR_HIST_STATUS, ODR_HIST_MOVING, ODR_HIST_AGE_SECONDS,
  ODR_HIST_WIND_DRIFT_FACTOR, ODR_HIST_CURRENT_DRIFT_FACTOR, ODR_HIST_TERMINAL_VELOCITY,
  ODR_HIST_PROPERTY0 = 2000 /* + slot of odr_particles_set_property */
};
typedef struct odr_history odr_history;
int odr_history_create(odr_ctx *ctx, int64_t n_trajectories, int32_t n_times, int32_t nvars,
                       const int32_t *var_codes, odr_history **out);
/* trajectory row 0 of the buffer = element `id_base` (default 0): one rank of a particle-sharded run records its own
 * contiguous ID range */
int odr_history_set_id_base(odr_ctx *ctx, odr_history *h, int64_t id_base);
int odr_history_destroy(odr_ctx *ctx, odr_history *h);
/* position_from_previous (bit 0): lon / lat are taken from the state saved by update_previous_state (odr_store_previous,
 * odr_env_coast_advect) -- the position before this step's advection -- so that the record may follow the fused launch.
 * ODR_HIST_PROPERTIES_FROM_SNAPSHOT (bit 1): a property that odr_particles_snapshot_property has copied is read from
 * that copy (Leeway: crosswind_slope / orientation as they were before the jibes of odr_env_coast_leeway). */
enum { ODR_HIST_PROPERTIES_FROM_SNAPSHOT = 2 };
int odr_history_record(odr_ctx *ctx, odr_particles *p, odr_history *h, int32_t time_index, int only_deactivated,
                       int position_from_previous);
/* asynchronous: extract time slots [t0, t0+nt) of every variable into pinned host memory as
 * [trajectory][time] float32 (the reference's dims); _wait blocks; _host_ptr is valid until the next flush */
int odr_history_flush(odr_ctx *ctx, odr_history *h, int32_t t0, int32_t nt);
int odr_history_wait(odr_ctx *ctx, odr_history *h);
int odr_history_host_ptr(odr_ctx *ctx, odr_history *h, int32_t var_index, float **ptr, int32_t *nt);
int odr_history_reset(odr_ctx *ctx, odr_history *h);   /* new buffer: NaN (:2493-2499) */
int odr_history_minmax(odr_ctx *ctx, odr_history *h, int32_t var_index, double *minval, double *maxval); /* :2409-2414 */

/* ---------------------------------------------------------------- density maps
 * OpenDriftSimulation.get_density_array (models/basemodel/__init__.py:4091-4146) for GIVEN bin edges: per output time the three
 * np.histogram2d of the reference -- H: every entry unless z < 0; H_submerged: unless z >= 0 (a NaN z at a finite position counts
 * in both, z = -0.0 is surface); H_stranded: status == stranded_code (:4122-4128; < 0: no such category, H_stranded may be NULL and
 * is zero-filled if given).  The bin of a float32 lon / lat is np.histogram2d's on the edge arrays themselves:
 * searchsorted(edges, (double)v, side='right') - 1, a value equal to the last edge in the last bin, NaN and everything outside
 * dropped (csrc/odr_density.hip.h).  The edges are the caller's (:4095-4103 is NumPy arithmetic on the result arrays).
 * lon, lat, z, status, weight: [trajectory][time] float32, the layout of odr_history_flush, each in host OR device memory (device
 * arrays must be complete: no stream is waited for); weight NULL: counts, else each bin holds the float64 sum of its float32
 * weights (float64 atomic adds: the last bits depend on the order of arrival; counts are integer adds and exact).
 * lon_edges / lat_edges: host, strictly increasing, finite.  H, H_submerged, H_stranded: host, float64 [time][lon_bin][lat_bin].
 * Host inputs are uploaded in slabs of whole trajectories within a byte budget (256 MiB; the environment variable
 * ODR_DENSITY_SLAB_BYTES overrides it); the histograms stay on the device for all of them.  Synchronous.
 * ODR_ERR_INVALID: fewer than two edges, edges not finite or not strictly increasing, more than 2^28 bins per output time,
 * n_trajectories >= 2^32 (the counts are 32-bit), a NULL pointer other than weight and (stranded_code < 0) H_stranded -- checked
 * before anything is launched. */
int odr_density_map(odr_ctx *ctx, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, const float *z,
                    const float *status, const float *weight, int32_t stranded_code, int32_t n_lon_edges, const double *lon_edges,
                    int32_t n_lat_edges, const double *lat_edges, double *H, double *H_submerged, double *H_stranded);
/* device time [ms] of the kernel launches of this context's last odr_density_map, summed over its slabs (tools/bench_density.py) */
int odr_density_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- projected density and concentration maps
 * proj in all of these: the projection the map grid is regular in (NULL: longitude / latitude) -- ODR_PROJ_LATLONG, the two
 * ODR_PROJ_STERE_*, ODR_PROJ_STERE_OBLIQUE, ODR_PROJ_MERC, ODR_PROJ_LCC, ODR_PROJ_TMERC, ODR_PROJ_LAEA and ODR_PROJ_MOLL; ODR_PROJ_OB_TRAN,
 * ODR_PROJ_CURVILINEAR and unknown kinds are ODR_ERR_INVALID.  lon, lat, z, status, specie, weight: [trajectory][time] float32, each
 * in host OR device memory (device arrays must be complete: no stream is waited for); host arrays are uploaded in slabs of whole
 * trajectories within a byte budget (256 MiB; the environment variable ODR_CONC_SLAB_BYTES overrides it).  Every call is synchronous
 * and checks all of its arguments before anything is launched (csrc/odr_conc.hip.h).
 *
 * odr_density_map_proj: OpenDriftSimulation.get_density_array_proj (models/basemodel/__init__.py:4148-4245) for GIVEN edges in
 * projection units.  (x, y) = proj(lon, lat) in float64 from the float32 positions; the bin is np.histogram2d's on the edge arrays
 * themselves, as in odr_density_map.  The reference takes an entry out of a map by MOVING it to (outsidex, outsidey) = 1.5 *
 * (max(x_array), max(y_array)): out of H when z < 0, out of H_submerged when z >= 0, out of H_stranded when status != stranded_code
 * (a NaN z stays in both, a NaN status is moved).  outside_bin: the bin ix * (n_y_edges - 1) + iy of that point when it lies INSIDE
 * the grid (both maxima negative) -- moved entries are then counted there, whatever their own position -- or -1.  weight NULL:
 * counts (32-bit integer adds, exact), else float64 sums of the float32 weights (atomic adds: the last bits depend on the order of
 * arrival); a NaN weight of a moved entry makes outside_bin NaN, as in NumPy.  stranded_code < 0: no such category, H_stranded may
 * be NULL and is zero-filled if given.  H, H_submerged, H_stranded: host, float64 [time][x_bin][y_bin].
 * ODR_ERR_INVALID: fewer than two edges, edges not finite or not strictly increasing, more than 2^28 bins per output time, the
 * three maps larger than 8 GiB on the device (3 * n_times * bins * 4 bytes, 8 bytes with weights), outside_bin outside -1 .. bins - 1,
 * n_trajectories >= 2^32, a refused projection, a NULL pointer other than proj, weight and (stranded_code < 0) H_stranded. */
int odr_density_map_proj(odr_ctx *ctx, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, const float *z,
                         const float *status, const float *weight, int32_t stranded_code, const odr_proj_desc *proj, int32_t n_x_edges,
                         const double *x_edges, int32_t n_y_edges, const double *y_edges, int64_t outside_bin, double *H,
                         double *H_submerged, double *H_stranded);
/* odr_species_layer_map: RadionuclideDrift.get_radionuclide_density_array (models/radionuclides.py:1425-1492) for given edges and
 * layer bounds, counts only: an entry counts in H[time][sp][zi][x_bin][y_bin] iff specie == sp (sp in 0 .. n_species - 1),
 * z_array[zi] < z <= z_array[zi + 1] compared in float64, and its projected position has a bin; NaN z or specie: nowhere.  Nothing
 * is moved.  z_array[n_z]: host, strictly increasing, finite, at most 256 values.  H: host, float64 (32-bit integer adds on the
 * device, widened at the end).
 * ODR_ERR_INVALID: as above for edges and projection; z_array not increasing or not finite; more than 2^28 bins per output time,
 * species and layers included; the histogram larger than 8 GiB on the device (n_times * bins * 4 bytes); n_species < 1; a NULL
 * pointer other than proj. */
int odr_species_layer_map(odr_ctx *ctx, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat, const float *z,
                          const float *specie, const odr_proj_desc *proj, int32_t n_x_edges, const double *x_edges, int32_t n_y_edges,
                          const double *y_edges, int32_t n_z, const double *z_array, int32_t n_species, double *H);
/* device time [ms] of the kernel launches of this context's last odr_density_map_proj or odr_species_layer_map, summed over its
 * slabs (tools/bench_concentration.py) */
int odr_conc_last_kernel_ms(odr_ctx *ctx, float *ms);
/* odr_proj_extent: extent4 = (min x, max x, min y, max y) of (x, y) = proj(lon, lat) over the n positions whose projected
 * coordinates are both finite -- what x.min() ... y.max() of the reference give for a result without NaN (+inf, -inf, +inf, -inf when
 * no position is finite).  A reduction on the device: per-workgroup partial records, finished on the host; no float atomics. */
int odr_proj_extent(odr_ctx *ctx, const odr_proj_desc *proj, int64_t n, const float *lon, const float *lat, double *extent4);
/* odr_proj_grid_lonlat: lon, lat = proj(X, Y, inverse=True) of Y, X = np.meshgrid(ys, xs): host, float64 [nx][ny] degrees (NaN
 * outside a projection's range).  xs[nx], ys[ny]: host, finite. */
int odr_proj_grid_lonlat(odr_ctx *ctx, const odr_proj_desc *proj, int32_t nx, const double *xs, int32_t ny, const double *ys, double *lon,
                         double *lat);
/* odr_box_smooth: RadionuclideDrift.horizontal_smooth (models/radionuclides.py:1518-1551) of n_planes planes a[n0][n1], host
 * float64: every value is truncated to an integer, the plane padded with n zeros all round, the (2 n + 1)^2 window summed and the sum
 * divided by (2 n + 1)^2 in float64 -- integer sums, so the bits are the reference's.  n == 0 copies.  out may be a.
 * ODR_ERR_INVALID: a value that is not finite, integer parts of a plane that sum to 2^53 or more, more than 2^28 cells per plane,
 * n < 0 or n >= 2^26, a NULL pointer. */
int odr_box_smooth(odr_ctx *ctx, int64_t n_planes, int32_t n0, int32_t n1, int32_t n, const double *a, double *out);

/* ---------------------------------------------------------------- FTLE maps
 * physics_methods.ftle (models/physics_methods.py:458-484) of the displacements that OpenDriftSimulation.calculate_ftle
 * (models/basemodel/__init__.py:4844-4923) forms from the last positions of one run of a grid of elements (:4898-4902, :4911-4915).
 * proj: the projection the grid is regular in -- every kind odr_source_grid takes (ODR_PROJ_LATLONG by a descriptor of that kind),
 * not ODR_PROJ_CURVILINEAR.  xs[nx], ys[ny]: host, the caller's np.arange values (they are not equidistant to the last bit and
 * are never recomputed from a start and delta).  lon, lat: float32 [ny][nx], row j column i the last valid position of the element
 * seeded at (xs[i], ys[j]), each in host OR device memory (device arrays must be complete: no stream is waited for); a position
 * that is not finite gives a NaN displacement.
 * Displacement, float64: (x, y) = proj(lon, lat) on the device; dX = x - xs[i], dY = y - ys[j].  The reference differentiates this
 * displacement, not the flow map, with np.gradient at unit spacing (interior (f[k+1] - f[k-1]) / 2, ends f[1] - f[0] and
 * f[n-1] - f[n-2]) and divides by 2 * delta once more (:467-474); both are kept.  J float32 (each float64 quotient rounded once),
 * D = J^T J in float32 without fused multiply-adds, the largest eigenvalue of the symmetric 2 x 2 in closed form in float64 rounded
 * to float32, ftle = log(sqrt(lambda)) / |duration_seconds| in float64 rounded to float32 (csrc/odr_ftle.hip.h).  lambda == 0:
 * -inf.  A NaN anywhere in a cell's stencil: NaN (the reference's LAPACK call raises there).
 * ftle: host, float32 [ny][nx].  displacement: host, 2 * ny * nx float64, the x plane then the y plane, or NULL (not reported).
 * Two launches, no atomics: two calls give the same bits.  Synchronous.
 * ODR_ERR_INVALID: nx < 2 or ny < 2, nx * ny >= 2^31, xs / ys / delta not finite, delta <= 0, duration_seconds 0 or not finite, a
 * NULL pointer other than displacement, ODR_PROJ_CURVILINEAR or an unknown kind -- checked before anything is launched. */
int odr_ftle_map(odr_ctx *ctx, const odr_proj_desc *proj, int32_t nx, int32_t ny, const double *xs, const double *ys, double delta,
                 double duration_seconds, const float *lon, const float *lat, float *ftle, double *displacement);
/* device time [ms] of the two kernel launches of this context's last odr_ftle_map that launched (tools/bench_ftle.py) */
int odr_ftle_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- inverse geodesics, trajectory lengths
 * pyproj.Geod(ellps='WGS84').inv as OpenDriftSimulation.get_trajectory_lengths calls it (models/basemodel/__init__.py:4618-4620):
 * the shortest WGS84 geodesic between n pairs of points, Karney's inverse (J. Geodesy 87:43-55, 2013) at order 6
 * (csrc/odr_geodinv.hip.h).  lon1, lat1, lon2, lat2: host, float64 degrees.  azi1, azi2: the FORWARD azimuths at both ends in
 * degrees (pyproj's back azimuth is azi2 turned by 180), s12: metres; host, each may be NULL.  A NaN or infinite coordinate and
 * |lat| > 90 give NaN; coincident points give 0, 0, 0.  Synchronous.  ODR_ERR_INVALID: n < 0, a NULL input. */
int odr_geod_inverse(odr_ctx *ctx, int64_t n, const double *lon1, const double *lat1, const double *lon2, const double *lat2,
                     double *azi1, double *azi2, double *s12);
/* OpenDriftSimulation.get_trajectory_lengths (models/basemodel/__init__.py:4614-4628).  lon, lat: [trajectory][time] float32, the
 * layout of odr_history_flush, each in host OR device memory (device arrays must be complete: no stream is waited for).  Per
 * trajectory and output interval: the float32 positions widened to float64, the geodesic distance in float64, NaN (an end that is
 * NaN: before seeding, after deactivation) -> 0 (:4621), speed = distance / dt_seconds with the sign of dt (:4622), speed > 100 ->
 * distance and speed 0 (:4623-4625).  total_length[trajectory]: np.cumsum(distances, 0)[-1] (:4626), the float64 sum in time order.
 * distances, speeds: [time - 1][trajectory] float64 as in the reference, host; either may be NULL, and with both NULL nothing of
 * size n_trajectories * n_times leaves the device.  total_length: host.  Host inputs go up in slabs of whole trajectories, lon
 * and lat of a slab within 256 MiB (ODR_TRAJ_SLAB_BYTES overrides); device inputs are walked in the same slabs.  No atomics: two
 * calls give the same bits, and the host build of the header gives those bits too.  Synchronous.
 * ODR_ERR_INVALID: n_times < 2, dt_seconds 0 or not finite, n_trajectories < 0, a NULL lon / lat / total_length -- checked before
 * anything is launched. */
int odr_trajectory_lengths(odr_ctx *ctx, int64_t n_trajectories, int32_t n_times, const float *lon, const float *lat,
                           double dt_seconds, double *total_length, double *distances, double *speeds);
/* device time [ms] of the kernel launches of this context's last odr_trajectory_lengths, summed over its slabs
 * (tools/bench_trajectory_lengths.py) */
int odr_trajectory_lengths_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- seeding geometry
 * pyproj.Geod(ellps='WGS84').npts(lon1, lat1, lon2, lat2, npts) as seed_cone and seed_repeated_segment call it
 * (models/basemodel/__init__.py:1286-1291, :1432-1437): npts points on the WGS84 geodesic from point 1 to point 2 at
 * i * s12 / (npts + 1), i = 1 .. npts -- both ends excluded.  One inverse (csrc/odr_geodinv.hip.h) for s12 and the azimuth, then one
 * direct solve per lane (csrc/odr_geodesic.hip.h); longitudes come out in [-180, 180].  out_lon, out_lat: host, npts float64.
 * Synchronous.  ODR_ERR_INVALID: npts < 0, a NULL output, a coordinate that is not finite, |lat| > 90. */
int odr_geod_npts(odr_ctx *ctx, double lon1, double lat1, double lon2, double lat2, int64_t npts, double *out_lon, double *out_lat);
/* matplotlib.path.Path(ring).contains_points(points): the crossing rule of its point_in_path in float64 for n points (x, y) and a
 * ring of m vertices (vx, vy), the edge from the last vertex back to the first included; inside[i] = 1 or 0.  All arrays host.
 * The flags are matplotlib's bit for bit (csrc/odr_seed.hip.h).  Synchronous.
 * ODR_ERR_INVALID: a NULL pointer, n < 0, m < 3, a vertex that is not finite -- checked before anything is launched. */
int odr_points_in_polygon(odr_ctx *ctx, int64_t n, const double *x, const double *y, int32_t m, const double *vx, const double *vy,
                          uint8_t *inside);
/* OpenDriftSimulation.points_within_polygon (models/basemodel/__init__.py:1487-1558): `number` positions evenly placed within the
 * polygon of m vertices (lons, lats; host float64 degrees, closed here if the last vertex differs from the first).  A regular grid
 * of spacing sqrt(area / number) is laid over the ring in the spherical Albers projection the reference asks for (R = 6370997 m,
 * standard parallels at the extreme latitudes, the four parameters rounded to 6 decimals as its '%f' does), every grid point is
 * inverse-projected and tested against the ring in lon / lat, and the points inside are kept in grid order (row-major, x fastest).
 * Element k of out_lon / out_lat (host, `number` float64) is inside point k mod n_inside.  No grid point inside: the caller's
 * vertices lons[0 : number] take their place, repeated in the same way.  An empty grid (nx * ny == 0): every element is the mean
 * of the vertices.  n_inside: the inside points of the whole grid (before the cut at `number`); nx, ny: the grid.  The set-up is
 * O(m) work on the host; no atomics: two calls give the same bits, and the host build of the header gives those bits too.
 * Synchronous.  ODR_ERR_INVALID: a NULL pointer, m < 3, number < 1, a vertex that is not finite, a cone constant |n| < 1e-10
 * (parallels symmetric about the equator: PROJ refuses them), an area that is zero or not finite, nx * ny >= 2^31 -- checked
 * before anything is launched. */
int odr_polygon_points(odr_ctx *ctx, int32_t m, const double *lons, const double *lats, int64_t number, double *out_lon,
                       double *out_lat, int64_t *n_inside, int32_t *nx, int32_t *ny);
/* device time [ms] of the kernel launches of this context's last odr_polygon_points (tools/bench_seed.py); 0 when it launched none */
int odr_polygon_points_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- unstructured (triangular-mesh) readers
 * The reference's UnstructuredReader (readers/basereader/unstructured.py, readers/reader_netCDF_CF_unstructured.py): the value
 * at the nearest node (node variables) or nearest face centre (face variables), at the nearest sigma layer or level of that
 * column, at the nearest time level -- no interpolation anywhere (csrc/odr_umesh.hip.h).
 * odr_umesh_create: x, y [n_nodes] and xc, yc [n_faces] (n_faces may be 0) host float64 in the mesh's own coordinates (proj; NULL:
 * geographic).  One exact search index each is built on the host, once.  siglay [n_siglay][n_nodes], siglev [n_siglay + 1][n_nodes],
 * h [n_nodes], siglay_center / siglev_center / h_center the same over the faces: host float32, each may be NULL (n_siglay 0: all).
 * Coverage is the bounding box of the nodes.  ODR_ERR_INVALID: no node, a position that is not finite, sigma arrays without
 * their depth array or without n_siglay, ODR_PROJ_OB_TRAN / ODR_PROJ_CURVILINEAR.  odr_umesh_destroy waits for the context's stream. */
typedef struct odr_umesh odr_umesh;
int odr_umesh_create(odr_ctx *ctx, const odr_proj_desc *proj, int32_t n_nodes, const double *x, const double *y, int32_t n_faces,
                     const double *xc, const double *yc, int32_t n_siglay, const float *siglay, const float *siglev,
                     const float *siglay_center, const float *siglev_center, const float *h, const float *h_center, odr_umesh **out);
int odr_umesh_destroy(odr_ctx *ctx, odr_umesh *mesh);
/* Variable var_id (ODR_VAR_*) of the time level t_epoch becomes resident in `slot` (0 .. 2): data is host float32, [points] with
 * n_levels 0 or [n_levels][points], points = n_faces (on_faces != 0) or n_nodes.  n_levels == n_siglay: the variable sits on the
 * layers, n_siglay + 1: on the levels -- decided by the count, as the reference decides by the array's shape.  Synchronous.
 * ODR_ERR_INVALID: a slot outside 0 .. 2, another level count, a level count without the matching sigma and depth arrays of the
 * mesh, a face variable on a mesh without faces. */
int odr_umesh_set_level(odr_ctx *ctx, odr_umesh *mesh, int32_t slot, double t_epoch, int32_t var_id, int on_faces, int32_t n_levels,
                        const float *data);
/* For every element of the particle set, in ONE launch: lonlat2xy; the coverage test; the nearest node and / or face (one search
 * each, however many variables share it); per variable the sigma index argmin(|sigma * h - z|) (float32 product, float64
 * difference, first minimum) and the float32 value of the level in `slot`; x / y vector pairs (both components in var_ids)
 * rotated from the mesh's CRS to east / north unless it is geographic; then the merge into the element's environment slot: a
 * finite value is taken when first_flags[k] != 0 or the slot holds nothing finite.  Elements outside the box keep what they
 * have; a variable that was never sampled starts as NaN.  nvars: 1 .. 8.  Enqueued on the context's stream.
 * ODR_ERR_INVALID: a slot outside 0 .. 2, nvars outside 1 .. 8, a variable id given twice; ODR_ERR_STATE: the level in `slot`
 * does not hold one of the variables. */
int odr_umesh_sample(odr_ctx *ctx, odr_particles *p, odr_umesh *mesh, int32_t slot, int32_t nvars, const int32_t *var_ids,
                     const int32_t *first_flags);
/* The bare query (tests, tools/bench_umesh.py): idx_out[i] = index of the node (on_faces 0) or face centre nearest to (x[i], y[i]),
 * mesh coordinates, host float64; squared distances are dx * dx + dy * dy in float64 without contraction; exact.  -1 for a point
 * that is not finite.  A point far outside the box of the mesh is answered exactly too, but visits a large share of the tree
 * (every point is about as far away); odr_umesh_sample never searches for one.  Synchronous. */
int odr_umesh_nearest(odr_ctx *ctx, odr_umesh *mesh, int on_faces, int64_t n, const double *x, const double *y, int32_t *idx_out);
/* device time [ms] of the launches of this context's last odr_umesh_nearest, or of the launch of its last odr_umesh_sample if
 * that came later (waits for it) */
int odr_umesh_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- SCHISM-style mesh reader (three-node inverse-distance mean)
 * The reference's reader_schism_native (readers/reader_schism_native.py): a time level is a cloud of points -- the nodes for a 2-D
 * variable, node x vertical level at the level's own zcor for a 3-D one -- and a value is the inverse-distance mean over the
 * THREE nearest points of that cloud (ReaderBlockUnstruct.interpolate :982-1056), blended linearly between the two time levels
 * that bracket the time (:614-642).  The searches are exact and use one 2-D index for both kinds of cloud (csrc/odr_schism.hip.h,
 * DESIGN.md 8p).
 * odr_schism_create: x, y [n_nodes] host float64 in the mesh's own coordinates (proj; NULL: geographic); n_levels: vertical levels
 * of the 3-D variables (0: none); hull_x, hull_y [n_hull]: the vertices of the convex hull of the nodes in ring order -- coverage
 * is strict inclusion in that ring by odr_shape's predicate.  ODR_ERR_INVALID: fewer than 3 nodes or hull vertices, a position
 * that is not finite, more than 128 levels, ODR_PROJ_OB_TRAN / ODR_PROJ_CURVILINEAR.  odr_schism_destroy waits for the context's
 * stream. */
typedef struct odr_schism odr_schism;
int odr_schism_create(odr_ctx *ctx, const odr_proj_desc *proj, int32_t n_nodes, const double *x, const double *y, int32_t n_levels,
                      int32_t n_hull, const double *hull_x, const double *hull_y, odr_schism **out);
int odr_schism_destroy(odr_ctx *ctx, odr_schism *mesh);
/* The vertical coordinate of the time level in `slot` (0 .. 3): zcor [n_nodes][n_levels] host float32, negative down, NaN for the
 * levels below the sea bed of a node.  Synchronous.  ODR_ERR_INVALID: a slot outside 0 .. 3, a mesh without levels, fewer than
 * three finite entries. */
int odr_schism_set_zcor(odr_ctx *ctx, odr_schism *mesh, int32_t slot, double t_epoch, const float *zcor);
/* Variable var_id (ODR_VAR_*) of the time level in `slot`: host float32 [n_nodes] (n_levels 0) or [n_nodes][n_levels] (n_levels =
 * the mesh's).  Synchronous.  ODR_ERR_INVALID: a slot outside 0 .. 3, another level count. */
int odr_schism_set_level(odr_ctx *ctx, odr_schism *mesh, int32_t slot, double t_epoch, int32_t var_id, int32_t n_levels, const float *data);
/* For every element of the particle set, in ONE launch: lonlat2xy; the hull test; the three nearest nodes if a 2-D variable is
 * asked; the three nearest points of the cloud of each time level if a 3-D variable is asked; per variable
 * (fac * data).sum / fac.sum with fac = 1 / max(distance, 1e-10) in float64 at either level and before * (1 - w) + after * w;
 * x / y vector pairs rotated from the mesh's CRS to east / north unless it is geographic; the merge into the element's
 * environment slot as odr_umesh_sample does it.  slot_after < 0: the values of slot_before alone.  nvars: 1 .. 8.  Enqueued on
 * the context's stream.  ODR_ERR_INVALID: a slot outside 0 .. 3, w outside 0 .. 1, nvars outside 1 .. 8, a variable id given
 * twice; ODR_ERR_STATE: a level does not hold one of the variables, or a 3-D variable's level is without zcor. */
int odr_schism_sample(odr_ctx *ctx, odr_particles *p, odr_schism *mesh, int32_t slot_before, int32_t slot_after, double w, int32_t nvars,
                      const int32_t *var_ids, const int32_t *first_flags);
/* The bare query (tests, tools/bench_schism.py): the three nearest points of (x[i], y[i]) among the nodes (z NULL), or of
 * (x[i], y[i], z[i]) among node x level at the zcor of `slot`, ascending: idx_out [n][3] (the node; for a 3-D query the position in
 * the flattened [node][level] array with the NaN entries removed, as the reference numbers its cloud), dist_out [n][3] =
 * sqrt((dx dx + dy dy) + dz dz) in float64 without contraction; exact.  -1 / inf for a point that is not finite.  visits_out [n]
 * (may be NULL): tree nodes whose distance was formed.  Host arrays.  Synchronous. */
int odr_schism_nearest3(odr_ctx *ctx, odr_schism *mesh, int32_t slot, int64_t n, const double *x, const double *y, const double *z,
                        int64_t *idx_out, double *dist_out, int32_t *visits_out);
/* device time [ms] of the launches of this context's last odr_schism_nearest3, or of the launch of its last odr_schism_sample if
 * that came later (waits for it) */
int odr_schism_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- coastline polygons (shape reader)
 * The reference's reader_shape.Reader (readers/reader_shape.py): land_binary_mask = shapely.contains_xy(unary_union(polys), x, y),
 * here an exact crossing-number test behind a uniform grid whose cost per point is the local density of edges
 * (csrc/odr_shape.hip.h).
 * odr_shape_create (Reader.__init__, reader_shape.py:82-104): the edges of all rings of all polygons, host float64 in the
 * reader's own coordinates (proj; NULL: geographic), poly[k] in 0 .. n_poly - 1 the polygon edge k belongs to (exterior ring
 * and holes alike); closed rings, no edge of zero length.  nx, ny: the grid, 0 = automatic (about two cells per edge).  invert:
 * the mask is 1 - contains (:106-110).  The grid and its lists are built on the host, once; offsets are 64-bit.  Coverage is the
 * box of the vertices.  ODR_ERR_INVALID: no edge, a vertex that is not finite, an edge of zero length, a polygon id out of
 * range, more than 2^28 cells, ODR_PROJ_OB_TRAN / ODR_PROJ_CURVILINEAR.  odr_shape_destroy waits for the context's stream. */
typedef struct odr_shape odr_shape;
int odr_shape_create(odr_ctx *ctx, const odr_proj_desc *proj, int64_t n_edges, const double *x1, const double *y1, const double *x2,
                     const double *y2, const int32_t *poly, int32_t n_poly, int32_t nx, int32_t ny, int invert, odr_shape **out);
int odr_shape_destroy(odr_ctx *ctx, odr_shape *shape);
/* Reader.get_variables behind get_variables_interpolated (reader_shape.py:112-130; basereader/variables.py:860-914, covers_positions_xy
 * :229-257) for every element of the particle set, in ONE launch: lonlat2xy, the coverage box, the list walk of the element's
 * cell, invert, and the merge into the land_binary_mask slot: the value is taken when first != 0 or the slot holds nothing
 * finite.  Elements outside the box keep what they have; a slot that was never sampled starts as NaN.  Enqueued on the
 * context's stream. */
int odr_shape_sample(odr_ctx *ctx, odr_particles *p, odr_shape *shape, int first);
/* The bare query (Reader._on_land, reader_shape.py:106-110; tests, tools/bench_shape.py): out[i] = 1 / 0 at (x[i], y[i]) in the
 * reader's coordinates, NaN outside the box or where the point is not finite; host float64 in, host float32 out.  Synchronous. */
int odr_shape_contains(odr_ctx *ctx, odr_shape *shape, int64_t n, const double *x, const double *y, float *out);
/* stats[0 .. 7]: cells, list entries, longest list, mean list of the cells that have one, times the grid's origin was shifted to
 * keep its lines off the vertices, bytes of the index on the device, nx, ny */
int odr_shape_stats(odr_ctx *ctx, odr_shape *shape, double *stats);
/* device time [ms] of the launches of this context's last odr_shape_contains, or of the launch of its last odr_shape_sample if
 * that came later (waits for it) */
int odr_shape_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- reader operators (sums, numbers, Gaussian blends)
 * The reference's readers/operators/: `a + b` (ops.py:14-25 -> readerops.Combined), `n + r`, `n * r`, `r / n`, `r - n` (ops.py:30-50
 * -> numops.Combined) and r.combine_gaussian(measurements, std) (ops.py:52-96), evaluated per element and variable on the device
 * (csrc/odr_combine.hip.h).  The caller flattens the expression to postfix: */
enum { ODR_COMBINE_SOURCE = 0,      /* push the value of source `index` at the element (its own time interpolation and rotation) */
       ODR_COMBINE_UNIFORM = 1,     /* push uniform leaf `index`: one value per variable, resolved by the caller (a time series) */
       ODR_COMBINE_ADD = 2,         /* the two topmost values become their sum (readerops.py:107) */
       ODR_COMBINE_GAUSS_TERM = 3,  /* behind a blend's model operand, once per measurement: uniform leaf `index` measured at
                                     * longitude d[0], latitude d[1], with standard deviation d[2] [m] (readerops.py:110-123) */
       ODR_COMBINE_GAUSS_END = 4,   /* top = top (1 - sum f) + sum b f, f = exp(-(distance / std)^2 / 2) on WGS84 */
       ODR_COMBINE_NUM_ADD = 5,     /* top = d[0] + top   (numops.py:28-30) -- a number-op is the last operation of a program */
       ODR_COMBINE_NUM_MUL = 6,     /* top = d[0] * top   (numops.py:32-34) */
       ODR_COMBINE_NUM_DIV = 7 };   /* top = top / d[0]   (numops.py:40-42) */
typedef struct { int32_t kind, index; double d[3]; } odr_combine_op;
/* odr_combined_create (Combined.__init__, readerops.py:25-60; numops.py:20-27): 1 .. 32 operations, at most three values held at a
 * time -- (a + b) + (c + d) and every left-deep chain fit -- and 8 uniform leaves.  ODR_ERR_INVALID otherwise, and for a source id
 * that is not in use.  A value is float32 where the reference's array is: a 2-D block level of a reader that covers EVERY element
 * of the call (a reader that misses one hands out a masked float64 array, variables.py:840-858); float32 + float32 is a float32
 * sum, number o float32 a float64 operation (the reference's operands are masked arrays).  The operands' vector pairs are NOT rotated: readerops.py:84-101 does not pass
 * rotate_to_proj on. */
typedef struct odr_combined odr_combined;
int odr_combined_create(odr_ctx *ctx, int32_t n_ops, const odr_combine_op *ops, odr_combined **out);
int odr_combined_destroy(odr_ctx *ctx, odr_combined *combined);
/* Combined.get_variables_interpolated (readerops.py:78-133; numops.py:52-71) behind get_environment's reader loop
 * (environment.py:597-762, the float32 cast of :695) for every element of the particle set at time t_epoch: the reader front
 * door once per leaf (its projection and coverage, which also settle the leaf's dtype class; the positions go through the particle
 * set's scratch memory), then ONE sampling launch for var_ids (1 .. 8, none twice).  The result is missing where an operand is; a
 * finite value is taken where first[k] != 0 or where the slot of variable k holds nothing finite; a slot that was never sampled
 * starts as NaN.  uniform_values: [nvars][n_uniform].  ODR_ERR_STATE when a gridded leaf's resident levels do not serve t_epoch;
 * ODR_ERR_INVALID for a leaf with ensemble members.  Enqueued on the context's stream. */
int odr_combined_sample(odr_ctx *ctx, odr_particles *p, odr_combined *combined, int32_t nvars, const int32_t *var_ids, const uint8_t *first,
                        double t_epoch, int32_t n_uniform, const double *uniform_values);
/* device time [ms] of the two launches of this context's last odr_combined_sample (waits for them) */
int odr_combined_last_kernel_ms(odr_ctx *ctx, float *ms);

/* ---------------------------------------------------------------- ROMS sigma grid
 * The sigma -> z regridding reader_ROMS_native.get_variables applies to every 4-D variable of a block
 * (reader_ROMS_native.py:512-538,617-684) with roppy (readers/roppy/depth.py): sdepth (:31-113, rho points,
 * Vtransform 1 | 2, S = NULL: -1 + (k + 0.5)/N), z_rho -= zeta, positive z_rho -> NaN; multi_zslice (:213-284),
 * values > 1e9 -> NaN.  float64 arithmetic in NumPy's operation order.  H, zeta: [ny][nx] host arrays. */
typedef struct odr_sgrid odr_sgrid;
int odr_sgrid_create(odr_ctx *ctx, int32_t ny, int32_t nx, int32_t N, const double *H, const double *zeta_or_null,
                     double Hc, const double *Cs_r, const double *S_or_null, int32_t Vtransform, odr_sgrid **out);
int odr_sgrid_destroy(odr_ctx *ctx, odr_sgrid *g);
int odr_sgrid_download_zrho(odr_ctx *ctx, odr_sgrid *g, double *out /* [N][ny][nx] */);
/* field [N][ny][nx] float32 (is_f64 = 0) or float64, host or device memory -> *out_dev32: device float32
 * [kmax][ny][nx] in result slot out_slot (0..7; valid until the next call with the same slot -- one slot per
 * variable of a block, then pass the pointers to odr_block_upload_device); out_host64 (optional): the float64 result */
int odr_sgrid_zslice(odr_ctx *ctx, odr_sgrid *g, const void *field, int is_f64, int on_device, int32_t kmax,
                     const double *Z, int32_t out_slot, void **out_dev32, double *out_host64);

#ifdef __cplusplus
}
#endif
#endif /* ODRIFT_H */
