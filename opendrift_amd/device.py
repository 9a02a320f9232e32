"""Thin NumPy-facing wrapper over the C ABI (include/odrift.h).

`Context` is the device image of OpenDrift's Environment (readers + priority lists);
`Particles` is the device image of a LagrangianArray.  All arithmetic happens in
libodrift_hip.so; this file only marshals arrays.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import VARIABLES, check

_dp, _fp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)

# the 16 slots of the movers' global reduction (Particles.reduce_scalars, Particles.reduction_dict), in the library's order
REDUCTION_KEYS = ('n_active', 'lon_min', 'lon_max', 'lat_min', 'lat_max', 'z_min', 'z_max', 'D_max',
                  'stokes_sum_max', 'wind_speed_max', 'wdf_surface_max', 'n_surface', 'hs_max', 'tp_max', 'rel_wind_speed_max',
                  'mld_max')


def _vid(v, aliases=None):
    """Device id of a variable name (ids pass through).  aliases: Context.slot_aliases."""
    if isinstance(v, (int, np.integer)):
        return v
    if v in VARIABLES:
        return VARIABLES[v]
    if aliases and v in aliases:
        return aliases[v]
    raise KeyError(v)


def _d(a, n=None):
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)) if n is not None
                             else np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(_dp)


def _f(a, n=None):
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32), (n,)) if n is not None
                             else np.asarray(a, dtype=np.float32))
    return a, a.ctypes.data_as(_fp)


def _i(a, n=None):
    if a is None:
        return None, None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32), (n,)) if n is not None
                             else np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(_ip)


def proj_desc(proj, map_grid=False):
    """dict(kind='latlong'|'stere_equit_sphere'|'stere_polar'|'merc'|'lcc'|'tmerc'|'laea'|'stere_oblique'|'ob_tran', a, rf|es, lat0,
    lon0, lat_ts, k0, x0, y0, lat1, lat2) -- projection.parse_proj4's output (ob_tran: lat1 = o_lat_p, lat2 = o_lon_p).
    map_grid: the projection of a map grid (Context.density_map_proj ...), which may be 'moll' as well; no reader can."""
    if proj is None or proj.get('kind', 'latlong') == 'latlong':
        return None
    if proj['kind'] == 'moll' and not map_grid:
        raise NotImplementedError('+proj=moll serves map grids only (get_density_array_proj, get_radionuclide_density_array)')
    kind = {'stere_equit_sphere': _abi.PROJ_STERE_EQUIT_SPHERE, 'stere_polar': _abi.PROJ_STERE_POLAR,
            'merc': _abi.PROJ_MERC, 'lcc': _abi.PROJ_LCC, 'tmerc': _abi.PROJ_TMERC, 'laea': _abi.PROJ_LAEA,
            'stere_oblique': _abi.PROJ_STERE_OBLIQUE, 'ob_tran': _abi.PROJ_OB_TRAN, 'moll': _abi.PROJ_MOLL}[proj['kind']]
    if 'es' in proj:
        es = proj['es']
    else:
        rf = proj.get('rf', 0.0)
        f = 0.0 if not rf else 1.0 / rf
        es = f * (2 - f)
    return _abi.ProjDesc(kind, proj.get('a', 6378137.0), es, proj.get('lat0', 0.0), proj.get('lon0', 0.0),
                         proj.get('lat_ts', 90.0), proj.get('k0', 1.0), proj.get('x0', 0.0), proj.get('y0', 0.0),
                         proj.get('lat1', 0.0), proj.get('lat2', proj.get('lat1', 0.0)))


def _grid_proj(proj):
    """The descriptor argument of the map-grid entry points: projection.parse_proj4's dict, an _abi.ProjDesc, or None (latlong)."""
    if not isinstance(proj, _abi.ProjDesc):
        proj = proj_desc(proj, map_grid=True)
    return proj, (None if proj is None else C.byref(proj))


class ContentIds:
    """Content ids of the 2-D variables of successive time levels of one reader (odr_block_set_content_ids) BY COMPARISON: a
    variable whose array equals, bit for bit, the one last seen for it keeps its id -- the reader re-reads the sea floor
    depth and the land mask with every block (structured.py:15-94), and the samplers then gather such a variable at one of
    the two bracketing levels.  Compared against a private copy (the caller may reuse its buffers); costs a pass over the
    array per level, so the reader bindings prefer a reader's own declaration (`static_variables`).  3-D variables,
    ensemble lists and device pointers get id 0 (unknown)."""
    _counter = 0

    def __init__(self):
        self.last = {}

    def assign(self, names, arrays):
        out = {}
        for k in names:
            a = arrays.get(k) if hasattr(arrays, 'get') else None
            if not isinstance(a, np.ndarray) or a.ndim != 2:
                out[k] = 0
                continue
            prev = self.last.get(k)
            a = np.ascontiguousarray(a, dtype=np.float32)
            if prev is None or prev[1].shape != a.shape or not np.array_equal(prev[1].view(np.uint32), a.view(np.uint32)):
                ContentIds._counter += 1
                prev = self.last[k] = (ContentIds._counter, np.array(a, copy=True))
            out[k] = prev[0]
        return out


def sea_water_density_default():
    """PhysicsMethods.sea_water_density() with its default arguments T=10., S=35. (physics_methods.py:574-608): the
    UNESCO 1983 one-atmosphere equation of state, a float64 constant of the oil formulae."""
    T, S = 10., 35.
    R1 = ((((6.536332E-09 * T - 1.120083E-06) * T + 1.001685E-04) * T - 9.095290E-03) * T + 6.793952E-02) * T - 28.263737
    R2 = (((5.3875E-09 * T - 8.2467E-07) * T + 7.6438E-05) * T - 4.0899E-03) * T + 8.24493E-01
    R3 = (-1.6546E-06 * T + 1.0227E-04) * T - 5.72466E-03
    SIG = R1 + (4.8314E-04 * S + R3 * np.sqrt(S) + R2) * S
    return float(SIG + 28.106331 + 1000.)


class Context:
    def __init__(self, device=0, seed=0):
        self.lib = _abi.load()
        self.h = C.c_void_p()
        check(self.lib.odr_ctx_create(device, seed, C.byref(self.h)))
        self.device = device
        self._grids = {}
        # A variable without a device id of its own that rides the slot of another one ON THIS CONTEXT: {name: id}.  Empty unless
        # a model opts in (ShipDrift: the Tm02 wave period in the peak period's slot); every other model's
        # context keeps failing on such a name with a KeyError that names it.
        self.slot_aliases = {}
        self.stage_math = 'exact'
        if os.environ.get('ODR_STAGE_MATH'):     # what-if runs of whole test / bench sessions: 'exact' | 'fast'
            self.set_stage_math(os.environ['ODR_STAGE_MATH'])

    def _vid(self, v):
        return _vid(v, self.slot_aliases)

    def _block_ids(self, names):
        """The ids of the variables of one block; two names that resolve to the same id (an alias and the variable whose slot
        it rides) in one block raise: the later one would silently replace the earlier."""
        ids = [self._vid(k) for k in names]
        if len(set(ids)) != len(ids):
            twice = [k for k, i in zip(names, ids) if ids.count(i) > 1]
            raise ValueError('variables %s of one block resolve to the same device id' % twice)
        return ids

    def close(self):
        if self.h:
            self.lib.odr_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.odr_sync(self.h))

    def _last_kernel_ms(self, symbol):
        """Device time [ms] of the launches of one unit's last call on this context (the odr_*_last_kernel_ms entry points)."""
        ms = C.c_float()
        check(getattr(self.lib, symbol)(self.h, C.byref(ms)))
        return ms.value

    def set_stream(self, stream_ptr):
        check(self.lib.odr_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- sources ----
    def add_constant(self, values):
        ids, pi = _i([self._vid(k) for k in values])
        vals, pv = _d([float(v) for v in values.values()])
        sid = C.c_int32()
        check(self.lib.odr_source_constant(self.h, len(ids), pi, pv, C.byref(sid)))
        return sid.value

    def add_landmask(self, lon0, lat0, dlon, dlat, cells):
        """Landmask raster source (reader_global_landmask.Reader on the device): cells[iy, ix] != 0 is land."""
        cells = np.ascontiguousarray(np.asarray(cells) != 0, dtype=np.uint8)
        ny, nx = cells.shape
        sid = C.c_int32()
        check(self.lib.odr_source_landmask(self.h, nx, ny, float(lon0), float(lat0), float(dlon), float(dlat),
                                           cells.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(sid)))
        return sid.value

    def add_double_gyre(self, A=0.25, epsilon=0.1, omega=0.628, t0=0.0):
        prm, pp = _d([A, epsilon, omega, t0])
        sid = C.c_int32()
        check(self.lib.odr_source_analytic(self.h, _abi.ANALYTIC_DOUBLE_GYRE, pp, 4, C.byref(sid)))
        return sid.value

    def add_oscillating(self, variable, amplitude, period_s, t0):
        prm, pp = _d([self._vid(variable), amplitude, period_s, t0])
        sid = C.c_int32()
        check(self.lib.odr_source_analytic(self.h, _abi.ANALYTIC_OSCILLATING, pp, 4, C.byref(sid)))
        return sid.value

    def add_grid(self, x, y, z=None, proj=None, lon_mode=1, mod360_x=0, domain=None):
        """x, y: the reader's coordinate arrays in the dtype it hands out (float32 for file readers)."""
        x, y = np.asarray(x), np.asarray(y)
        if domain is None:
            domain = (float(x.min()), float(x.max()), float(y.min()), float(y.max()), -np.inf, np.inf)
        dom, pd = _d(domain)
        nz = 0 if z is None else int(np.size(z))
        zz, pz = _d(np.atleast_1d(z)) if nz > 1 else (None, None)
        desc = proj_desc(proj)
        sid = C.c_int32()
        check(self.lib.odr_source_grid(self.h, C.byref(desc) if desc is not None else None, pd, lon_mode,
                                       mod360_x, nz, pz, C.byref(sid)))
        # index maps with the spans formed in the coordinate dtype (interpolators.py:32-33,110-111)
        xy8 = np.array([float(x[0]), float(x[-1] - x[0]), float(y[0]), float(y[-1] - y[0]),
                        float(x.min()), float(x.max() - x.min()), float(y.min()), float(y.max() - y.min())])
        self._grids[sid.value] = dict(xy8=xy8, ny=len(y), nx=len(x), nz=max(nz, 1))
        # float32 coordinate arrays: the index maps of a geographic reader are float32 arithmetic in the first get_environment of
        # a run (odr_ctx_set_position_class; interpolators.py:110-111 with elements.py:71-88)
        check(self.lib.odr_source_set_coordinate_dtype(self.h, sid.value, int(x.dtype == np.float32), int(y.dtype == np.float32)))
        return sid.value

    def add_grid_curvilinear(self, lon2d, lat2d, z=None, lon_mode=None, domain=None):
        """Reader without a projection (basereader/structured.py:44-113): 2D lon/lat node arrays, x/y = pixel indices."""
        lon2d = np.ascontiguousarray(lon2d, dtype=np.float64)
        lat2d = np.ascontiguousarray(lat2d, dtype=np.float64)
        assert lon2d.ndim == 2 and lon2d.shape == lat2d.shape
        ny, nx = lon2d.shape
        if lon_mode is None:   # modulate_longitude, variables.py:259-280: from the corner longitudes
            lon_mode = 1 if min(lon2d[0, 0], lon2d[0, -1], lon2d[-1, 0], lon2d[-1, -1]) < 0 else 2
        if domain is None:
            domain = (0.0, nx - 1.0, 0.0, ny - 1.0, -np.inf, np.inf)
        dom, pd = _d(domain)
        nz = 0 if z is None else int(np.size(z))
        zz, pz = _d(np.atleast_1d(z)) if nz > 1 else (None, None)
        sid = C.c_int32()
        check(self.lib.odr_source_grid_curvilinear(self.h, lon2d.ctypes.data_as(_dp), lat2d.ctypes.data_as(_dp), ny, nx,
                                                   pd, int(lon_mode), nz, pz, C.byref(sid)))
        # x = arange(nx), y = arange(ny): the index maps of interpolators.py:32-33,110-111
        xy8 = np.array([0.0, nx - 1.0, 0.0, ny - 1.0, 0.0, nx - 1.0, 0.0, ny - 1.0])
        self._grids[sid.value] = dict(xy8=xy8, ny=ny, nx=nx, nz=max(nz, 1))
        return sid.value

    def lonlat2xy(self, sid, lon, lat):
        """Variables.lonlat2xy of one source for host positions (variables.py:111-143)."""
        lon, pl = _d(np.atleast_1d(lon))
        lat, pa = _d(np.atleast_1d(lat))
        x, y = np.empty(len(lon)), np.empty(len(lon))
        check(self.lib.odr_source_lonlat2xy(self.h, sid, len(lon), pl, pa, x.ctypes.data_as(_dp), y.ctypes.data_as(_dp)))
        return x, y

    def _ensemble_arrays(self, sid, arrays):
        """A variable given as a LIST of member arrays (ensemble data, basereader/structured.py:125-147): declared on the
        source (odr_source_set_members) and stacked along the layer axis, [members x nz, ny, nx]."""
        out = {}
        for k, v in arrays.items():
            if isinstance(v, (list, tuple)):
                m = np.stack([np.ma.filled(a, np.nan) if isinstance(a, np.ma.MaskedArray) else np.asarray(a) for a in v]).astype(np.float32)
                known = self._grids[sid].setdefault('members', {})
                if known.get(k) != len(v):
                    check(self.lib.odr_source_set_members(self.h, sid, self._vid(k), len(v)))
                    known[k] = len(v)
                v = np.ascontiguousarray(m.reshape((-1,) + m.shape[-2:]))
            out[k] = v
        return out

    def declare_members(self, sid, variable, members):
        """The variable of this source arrives as `members` ensemble members stacked along the layer axis (what
        _ensemble_arrays does for a list of member arrays; a sharded run receives the stack itself)."""
        known = self._grids[sid].setdefault('members', {})
        if known.get(variable) != members:
            check(self.lib.odr_source_set_members(self.h, sid, self._vid(variable), int(members)))
            known[variable] = members

    def _content_ids(self, sid, slot, given):
        """odr_block_set_content_ids: {variable: id} for the level just uploaded (0 / missing: unknown).  The ids come from
        whoever knows the data -- a reader that declares `static_variables`, or ContentIds.assign where a comparison by
        value is affordable; nothing is compared here (a 1 M-node comparison per variable and level on the host costs more
        than the gathers it saves)."""
        given = {k: v for k, v in (given or {}).items() if v}
        if given:
            (va, pv), ia = _i([self._vid(k) for k in given]), np.asarray(list(given.values()), dtype=np.uint64)
            check(self.lib.odr_block_set_content_ids(self.h, sid, slot, len(given), pv, ia.ctypes.data_as(C.POINTER(C.c_uint64))))

    def upload_block(self, sid, slot, t_epoch, arrays, content_ids=None):
        """arrays: {variable: float32 [ny,nx] or [nz,ny,nx], or a list of such arrays (ensemble members)} -- one
        ReaderBlock / time level."""
        g = self._grids[sid]
        arrays = self._ensemble_arrays(sid, arrays)
        names = list(arrays)
        ids, pi = _i(self._block_ids(names))
        keep = [np.ascontiguousarray(np.ma.filled(arrays[k], np.nan) if isinstance(arrays[k], np.ma.MaskedArray)
                                     else arrays[k], dtype=np.float32) for k in names]
        for a in keep:
            assert a.shape[-2:] == (g['ny'], g['nx']), 'block shape %s does not match grid' % (a.shape,)
        nzs, pn = _i([a.shape[0] if a.ndim == 3 else 1 for a in keep])
        ptrs = (_fp * len(keep))(*[a.ctypes.data_as(_fp) for a in keep])
        xy8, px = _d(g['xy8'])
        check(self.lib.odr_block_upload(self.h, sid, slot, float(t_epoch), len(keep), pi, ptrs, pn, g['ny'],
                                        g['nx'], px))
        self._content_ids(sid, slot, content_ids)

    def upload_block_device(self, sid, slot, t_epoch, dev_ptrs, var_nz, content_ids=None):
        """dev_ptrs: {variable: device pointer (int) of a float32 array already in HBM, or a host NumPy array};
        var_nz: levels per variable (needed for the device pointers); content_ids: {variable: id} assigned by
        ContentIds.assign where the host arrays were (the rank that read the level)."""
        g = self._grids[sid]
        dev_ptrs = self._ensemble_arrays(sid, dev_ptrs)
        names = list(dev_ptrs)
        ids, pi = _i(self._block_ids(names))
        keep = {k: np.ascontiguousarray(np.ma.filled(v, np.nan) if isinstance(v, np.ma.MaskedArray) else v, dtype=np.float32)
                for k, v in dev_ptrs.items() if not isinstance(v, (int, np.integer))}
        nzs, pn = _i([(keep[k].shape[0] if keep[k].ndim == 3 else 1) if k in keep else var_nz[k] for k in names])
        ptrs = (C.c_void_p * len(names))(*[C.c_void_p(keep[k].ctypes.data if k in keep else int(dev_ptrs[k])) for k in names])
        xy8, px = _d(g['xy8'])
        check(self.lib.odr_block_upload_device(self.h, sid, slot, float(t_epoch), len(names), pi, ptrs, pn,
                                               g['ny'], g['nx'], px))
        self._content_ids(sid, slot, content_ids)

    def upload_block_async(self, sid, slot, t_epoch, arrays, var_nz=None, content_ids=None):
        """Enqueue the upload of one time level on the upload stream and return (the simulation continues); the
        block becomes visible with commit_block().  arrays: {variable: float32 host array (pin it with pin() for a true
        DMA transfer) or device pointer (int)}.  The arrays are kept referenced until the commit."""
        g = self._grids[sid]
        arrays = self._ensemble_arrays(sid, arrays)
        names = list(arrays)
        ids, pi = _i(self._block_ids(names))
        keep = {k: np.ascontiguousarray(np.ma.filled(v, np.nan) if isinstance(v, np.ma.MaskedArray) else v, dtype=np.float32)
                for k, v in arrays.items() if not isinstance(v, (int, np.integer))}
        nzs, pn = _i([(keep[k].shape[0] if keep[k].ndim == 3 else 1) if k in keep else var_nz[k] for k in names])
        ptrs = (C.c_void_p * len(names))(*[C.c_void_p(keep[k].ctypes.data if k in keep else int(arrays[k])) for k in names])
        xy8, px = _d(g['xy8'])
        check(self.lib.odr_block_upload_async(self.h, sid, slot, float(t_epoch), len(names), pi, ptrs, pn, g['ny'], g['nx'], px))
        self._content_ids(sid, slot, content_ids)      # (on the staged level: it becomes the slot's with the commit)
        self._staged_refs = getattr(self, '_staged_refs', {})
        self._staged_refs[(sid, slot)] = keep

    def block_broadcast(self, sid, slot, t_epoch, arrays, shapes, root=0, content_ids=None):
        """One reader time level from rank `root` to every rank over RCCL (odr_block_broadcast): staged on the upload stream
        like upload_block_async -- commit_block() makes it current.  arrays: {variable: float32 host array} on `root`, None
        elsewhere; shapes: {variable: shape} on every rank (the order of its keys is the order of the level's variables)."""
        g = self._grids[sid]
        names = list(shapes)
        ids, pi = _i(self._block_ids(names))
        nzs, pn = _i([(int(shapes[k][0]) if len(shapes[k]) == 3 else 1) for k in names])
        xy8, px = _d(g['xy8'])
        keep, ptrs = None, None
        if arrays is not None:
            keep = {k: np.ascontiguousarray(np.ma.filled(arrays[k], np.nan) if isinstance(arrays[k], np.ma.MaskedArray) else arrays[k],
                                            dtype=np.float32) for k in names}
            for k in names:
                if tuple(keep[k].shape) != tuple(shapes[k]):
                    raise ValueError('block_broadcast: %s has shape %s, announced %s' % (k, keep[k].shape, tuple(shapes[k])))
            ptrs = (C.c_void_p * len(names))(*[C.c_void_p(keep[k].ctypes.data) for k in names])
        check(self.lib.odr_block_broadcast(self.h, sid, slot, float(t_epoch), len(names), pi, ptrs, pn, g['ny'], g['nx'], px, int(root)))
        self._content_ids(sid, slot, content_ids)
        self._staged_refs = getattr(self, '_staged_refs', {})
        self._staged_refs[(sid, slot)] = keep

    def commit_block(self, sid, slot):
        check(self.lib.odr_block_commit(self.h, sid, slot))
        getattr(self, '_staged_refs', {}).pop((sid, slot), None)

    def pin(self, array):
        """Page-lock a host array (hipHostRegister) so that uploads from it are asynchronous DMA transfers."""
        a = np.asarray(array)
        assert a.flags['C_CONTIGUOUS']
        check(self.lib.odr_host_register(self.h, C.c_void_p(a.ctypes.data), a.nbytes))
        self._pinned = getattr(self, '_pinned', [])
        self._pinned.append(a)
        return a

    def unpin(self, array):
        check(self.lib.odr_host_unregister(self.h, C.c_void_p(np.asarray(array).ctypes.data)))

    def set_position_class(self, float32):
        """True: the main-loop samples that follow see the reference's float32 element arrays of the first get_environment of a run
        (odr_ctx_set_position_class: modulate_longitude in float32); False ends it."""
        check(self.lib.odr_ctx_set_position_class(self.h, 1 if float32 else 0))

    def set_stage_math(self, mode):
        """'exact' | 'fast': arithmetic of the Runge-Kutta stage evaluations (odr_ctx_set_stage_math, include/odrift.h)"""
        check(self.lib.odr_ctx_set_stage_math(self.h, _abi.STAGE_MATH[mode]))
        self.stage_math = mode

    def set_step_reduce(self, on=True, wind_drift_depth=0.1, relative_wind=False):
        """The movers' global early-out tests formed by the env_coast_advect launch instead of by a pass of their own
        (odr_ctx_set_step_reduce)."""
        check(self.lib.odr_ctx_set_step_reduce(self.h, int(bool(on)), float(wind_drift_depth), int(bool(relative_wind))))

    def set_seafloor_action(self, action, status_code=0):
        """general:seafloor_action for the sea floor checks inside update() (vertical_buoyancy, vertical_mixing)."""
        a = _abi.SEAFLOOR[action]      # ('settle': SedimentDrift.bottom_interaction, sedimentdrift.py:108-116)
        check(self.lib.odr_set_seafloor_action(self.h, a, int(status_code)))

    def set_seafloor_settle_species(self, slot, species):
        """The sea-floor action 'settle_species' (RadionuclideDrift.bottom_interaction, radionuclides.py:912-942): an element below
        the sea floor is lifted onto it and settles only if the species number in property slot `slot` is one of `species`."""
        mask = 0
        for k in species:
            if not 0 <= int(k) < _abi.RADIO_MAX_SPECIES:
                raise ValueError('species number %s outside 0 .. %d' % (k, _abi.RADIO_MAX_SPECIES - 1))
            mask |= 1 << int(k)
        check(self.lib.odr_set_seafloor_action(self.h, _abi.SEAFLOOR['settle_species'], mask | (int(slot) << 16)))

    def set_time_coverage(self, sid, t_start, t_end, always_valid=False):
        check(self.lib.odr_source_time_coverage(self.h, sid, float(t_start), float(t_end), int(always_valid)))

    def drop_block(self, sid, slot):
        check(self.lib.odr_block_drop(self.h, sid, slot))

    def kplane_read(self, sid, slot):
        """Debugging / tests (odr_block_kplane_read): (K plane of a resident level, K part of its node records in the same
        layout) as float32 [ny, nx, krec] arrays, or None when the level has no K plane."""
        g = self._grids[sid]
        krec = C.c_int32(0)
        check(self.lib.odr_block_kplane_read(self.h, sid, slot, C.byref(krec), None, None, 0))
        if krec.value == 0:
            return None
        plane = np.empty((g['ny'], g['nx'], krec.value), dtype=np.float32)
        recs = np.empty_like(plane)
        check(self.lib.odr_block_kplane_read(self.h, sid, slot, C.byref(krec), plane.ctypes.data_as(_fp), recs.ctypes.data_as(_fp),
                                             plane.size))
        return plane, recs

    def read_block(self, sid, slot, variable):
        """Debugging / tests (odr_block_read): one variable of a resident level as the preparation left it, float32 [ny, nx] or
        [nz, ny, nx]; None when the level does not hold it."""
        g = self._grids[sid]
        nz = C.c_int32(0)
        check(self.lib.odr_block_read(self.h, sid, slot, self._vid(variable), C.byref(nz), None, 0))
        if nz.value == 0:
            return None
        out = np.empty((nz.value, g['ny'], g['nx']), dtype=np.float32)
        check(self.lib.odr_block_read(self.h, sid, slot, self._vid(variable), C.byref(nz), out.ctypes.data_as(_fp), out.size))
        return out[0] if nz.value == 1 else out

    def set_convolution(self, sid, kernel, three_d=()):
        """StructuredReader.set_convolution_kernel for the levels of a grid source uploaded from now on (odr_source_set_convolution).
        kernel: the 2-D array of weights the reference hands to scipy.ndimage.convolve, or None to switch it off; three_d: the
        variables that arrive as 3-D arrays of one layer, [1, ny, nx] (convolved over z and y like every 3-D array)."""
        if kernel is None:
            check(self.lib.odr_source_set_convolution(self.h, sid, 0, 0, None, 0, None))
            return
        w = np.ascontiguousarray(kernel, dtype=np.float64)
        if w.ndim != 2 or w.size == 0:
            raise ValueError('a convolution kernel is a 2-D array of weights, got shape %s' % (w.shape,))
        if max(w.shape) > _abi.CONVOLVE_MAX_EDGE:
            raise ValueError('convolution kernel of %d x %d weights: at most %d x %d fit' % (w.shape + (_abi.CONVOLVE_MAX_EDGE,) * 2))
        ids, pi = _i([self._vid(v) for v in three_d]) if len(three_d) else (None, None)
        check(self.lib.odr_source_set_convolution(self.h, sid, w.shape[0], w.shape[1], w.ctypes.data_as(_dp), len(three_d), pi))

    def release_source(self, sid):
        """The source is no longer used: its blocks are dropped, its id is free for the next add_* (odr_source_release)."""
        check(self.lib.odr_source_release(self.h, int(sid)))
        self._grids.pop(sid, None)

    def bind(self, variable, source_ids, fallback=np.nan):
        ids, pi = _i(list(source_ids)) if len(source_ids) else (None, None)
        check(self.lib.odr_env_bind(self.h, self._vid(variable), len(source_ids), pi,
                                    np.nan if fallback is None else float(fallback)))

    def history(self, n_trajectories, n_times, variables, id_base=0):
        return History(self, n_trajectories, n_times, variables, id_base=id_base)

    def density_map(self, lon, lat, z, status, lon_edges, lat_edges, weight=None, stranded_code=-1, shape=None):
        """The three histograms per output time of get_density_array for given bin edges (odr_density_map): (H, H_submerged,
        H_stranded), float64 [time, lon_bin, lat_bin].  lon, lat, z, status, weight: [trajectory, time] float32 arrays, or device
        addresses (int) with `shape` = (n_trajectories, n_times).  stranded_code < 0: no such category, H_stranded stays zero."""
        arrays = [lon, lat, z, status] + ([weight] if weight is not None else [])
        keep, ptrs = [], []
        for a in arrays:
            if isinstance(a, (int, np.integer)):
                if shape is None:
                    raise ValueError('device addresses need shape=(n_trajectories, n_times)')
                ptrs.append(C.c_void_p(int(a)))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or (shape is not None and a.shape != tuple(shape)):
                raise ValueError('density_map: an input of shape %s, not [trajectory, time] %s' % (a.shape, shape or ''))
            shape = a.shape
            keep.append(a)
            ptrs.append(C.c_void_p(a.ctypes.data))
        if weight is None:
            ptrs.append(None)
        ntraj, nt = int(shape[0]), int(shape[1])
        le, pe = _d(np.asarray(lon_edges, dtype=np.float64).ravel())
        la, pa = _d(np.asarray(lat_edges, dtype=np.float64).ravel())
        dims = (nt, max(len(le) - 1, 0), max(len(la) - 1, 0))
        out = [np.zeros(dims) for _ in range(3)]
        check(self.lib.odr_density_map(self.h, ntraj, nt, *ptrs, int(stranded_code), len(le), pe, len(la), pa,
                                       *(o.ctypes.data_as(_dp) for o in out)))
        return tuple(out)

    def density_last_kernel_ms(self):
        return self._last_kernel_ms('odr_density_last_kernel_ms')

    @staticmethod
    def _traj_time_arrays(what, arrays, shape):
        """[trajectory, time] float32 arrays or device addresses (int) -> (arrays kept alive, pointers, shape)"""
        keep, ptrs = [], []
        for a in arrays:
            if isinstance(a, (int, np.integer)):
                if shape is None:
                    raise ValueError('device addresses need shape=(n_trajectories, n_times)')
                ptrs.append(C.c_void_p(int(a)))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or (shape is not None and a.shape != tuple(shape)):
                raise ValueError('%s: an input of shape %s, not [trajectory, time] %s' % (what, a.shape, shape or ''))
            shape = a.shape
            keep.append(a)
            ptrs.append(C.c_void_p(a.ctypes.data))
        return keep, ptrs, (int(shape[0]), int(shape[1]))

    def density_map_proj(self, proj, lon, lat, z, status, x_edges, y_edges, weight=None, stranded_code=-1, outside_bin=-1, shape=None):
        """The three histograms per output time of get_density_array_proj for given edges in the units of `proj`
        (odr_density_map_proj): (H, H_submerged, H_stranded), float64 [time, x_bin, y_bin].  proj: projection.parse_proj4's dict
        (None: latlong) or an _abi.ProjDesc.  outside_bin: ix * (len(y_edges) - 1) + iy of the point the reference moves removed
        entries to when that lies inside the grid, else -1.  Arrays as in density_map."""
        keep, ptrs, (ntraj, nt) = self._traj_time_arrays('density_map_proj', [lon, lat, z, status] + ([weight] if weight is not None else []), shape)
        if weight is None:
            ptrs.append(None)
        desc, pd = _grid_proj(proj)
        xe, px = _d(np.asarray(x_edges, dtype=np.float64).ravel())
        ye, py = _d(np.asarray(y_edges, dtype=np.float64).ravel())
        out = [np.zeros((nt, max(len(xe) - 1, 0), max(len(ye) - 1, 0))) for _ in range(3)]
        check(self.lib.odr_density_map_proj(self.h, ntraj, nt, *ptrs, int(stranded_code), pd, len(xe), px, len(ye), py, int(outside_bin),
                                            *(o.ctypes.data_as(_dp) for o in out)))
        return tuple(out)

    def species_layer_map(self, proj, lon, lat, z, specie, x_edges, y_edges, z_array, n_species, shape=None):
        """get_radionuclide_density_array's counts for given edges and layer bounds (odr_species_layer_map): float64
        [time, species, layer, x_bin, y_bin].  Arrays as in density_map."""
        keep, ptrs, (ntraj, nt) = self._traj_time_arrays('species_layer_map', [lon, lat, z, specie], shape)
        desc, pd = _grid_proj(proj)
        xe, px = _d(np.asarray(x_edges, dtype=np.float64).ravel())
        ye, py = _d(np.asarray(y_edges, dtype=np.float64).ravel())
        zb, pz = _d(np.asarray(z_array, dtype=np.float64).ravel())
        out = np.zeros((nt, max(int(n_species), 0), max(len(zb) - 1, 0), max(len(xe) - 1, 0), max(len(ye) - 1, 0)))
        check(self.lib.odr_species_layer_map(self.h, ntraj, nt, *ptrs, pd, len(xe), px, len(ye), py, len(zb), pz, int(n_species),
                                             out.ctypes.data_as(_dp)))
        return out

    def conc_last_kernel_ms(self):
        return self._last_kernel_ms('odr_conc_last_kernel_ms')

    def proj_extent(self, proj, lon, lat, n=None):
        """(min x, max x, min y, max y) of proj(lon, lat) over the positions whose projected coordinates are finite
        (odr_proj_extent).  lon, lat: float32 arrays of any shape, or device addresses (int) with n entries."""
        ptrs, keep = [], []
        for a in (lon, lat):
            if isinstance(a, (int, np.integer)):
                if n is None:
                    raise ValueError('device addresses need n')
                ptrs.append(C.c_void_p(int(a)))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if n is not None and a.size != n:
                raise ValueError('proj_extent: %d and %d positions' % (n, a.size))
            n = a.size
            keep.append(a)
            ptrs.append(C.c_void_p(a.ctypes.data))
        desc, pd = _grid_proj(proj)
        out = np.empty(4)
        check(self.lib.odr_proj_extent(self.h, pd, int(n), *ptrs, out.ctypes.data_as(_dp)))
        return tuple(float(v) for v in out)

    def proj_grid_lonlat(self, proj, xs, ys):
        """proj(X, Y, inverse=True) of Y, X = np.meshgrid(ys, xs) (odr_proj_grid_lonlat): lon, lat float64 [len(xs), len(ys)]."""
        xs, px = _d(np.asarray(xs, dtype=np.float64).ravel())
        ys, py = _d(np.asarray(ys, dtype=np.float64).ravel())
        desc, pd = _grid_proj(proj)
        lon, lat = np.empty((len(xs), len(ys))), np.empty((len(xs), len(ys)))
        check(self.lib.odr_proj_grid_lonlat(self.h, pd, len(xs), px, len(ys), py, lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp)))
        return lon, lat

    def box_smooth(self, a, n):
        """horizontal_smooth of the last two dimensions of `a` (odr_box_smooth): float64, the shape of `a`."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim < 2:
            raise ValueError('box_smooth: %d-dimensional input' % a.ndim)
        out = np.empty_like(a)
        planes = int(np.prod(a.shape[:-2], dtype=np.int64))
        check(self.lib.odr_box_smooth(self.h, planes, a.shape[-2], a.shape[-1], int(n), a.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def ftle_map(self, proj, xs, ys, delta, duration_seconds, lon, lat, displacement=False):
        """physics_methods.ftle of the displacements of a grid of elements (odr_ftle_map): float32 [ny, nx], and with
        displacement=True also the float64 [2, ny, nx] planes (x, y) the device differentiated.  proj: projection.parse_proj4's
        dict (None: latlong) or an _abi.ProjDesc; xs, ys: the grid's np.arange axes; lon, lat: float32 [ny, nx] (or ny * nx) last
        positions, row j column i the element seeded at (xs[i], ys[j]), or device addresses (int)."""
        xs, px = _d(np.asarray(xs, dtype=np.float64).ravel())
        ys, py = _d(np.asarray(ys, dtype=np.float64).ravel())
        nx, ny = len(xs), len(ys)
        if nx * ny >= 2 ** 31:
            raise ValueError('ftle_map: %d x %d cells, 2^31 or more' % (ny, nx))
        if not isinstance(proj, _abi.ProjDesc):
            proj = proj_desc(proj) or _abi.ProjDesc(_abi.PROJ_LATLONG, 6378137.0, 0.0, 0.0, 0.0, 90.0, 1.0, 0.0, 0.0, 0.0, 0.0)
        keep, ptrs = [], []
        for a in (lon, lat):
            if isinstance(a, (int, np.integer)):
                ptrs.append(C.c_void_p(int(a)))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.size != nx * ny:
                raise ValueError('ftle_map: %d positions for %d x %d cells' % (a.size, ny, nx))
            keep.append(a)
            ptrs.append(C.c_void_p(a.ctypes.data))
        out = np.empty((ny, nx), np.float32)
        disp = np.empty((2, ny, nx)) if displacement else None
        check(self.lib.odr_ftle_map(self.h, C.byref(proj), nx, ny, px, py, float(delta), float(duration_seconds), *ptrs,
                                    out.ctypes.data_as(_fp), None if disp is None else disp.ctypes.data_as(_dp)))
        return (out, disp) if displacement else out

    def ftle_last_kernel_ms(self):
        return self._last_kernel_ms('odr_ftle_last_kernel_ms')

    def geod_inv(self, lon1, lat1, lon2, lat2):
        """pyproj.Geod(ellps='WGS84').inv on the device (odr_geod_inverse): (az12, az21, dist) as float64 arrays of the broadcast
        shape -- the forward azimuth at point 1, the BACK azimuth at point 2 (pyproj's convention: the forward azimuth there turned
        by 180 degrees) and the distance in metres."""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in
                np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (lon1, lat1, lon2, lat2)))]
        shape = arrs[0].shape
        out = [np.empty(shape) for _ in range(3)]
        check(self.lib.odr_geod_inverse(self.h, arrs[0].size, *(a.ctypes.data_as(_dp) for a in arrs),
                                        *(o.ctypes.data_as(_dp) for o in out)))
        az12, azi2, dist = out
        az21 = np.where(azi2 > 0, azi2 - 180.0, azi2 + 180.0)
        return az12, az21, dist

    def trajectory_lengths(self, lon, lat, dt, segments=True, shape=None):
        """get_trajectory_lengths (odr_trajectory_lengths): (total_length [trajectory], distances, speeds [time - 1, trajectory]),
        float64; segments=False: total_length alone, and nothing per output interval leaves the device.  lon, lat: [trajectory,
        time] float32 arrays, or device addresses (int) with `shape` = (n_trajectories, n_times); dt: seconds between two output
        times, with its sign."""
        keep, ptrs = [], []
        for a in (lon, lat):
            if isinstance(a, (int, np.integer)):
                if shape is None:
                    raise ValueError('device addresses need shape=(n_trajectories, n_times)')
                ptrs.append(C.c_void_p(int(a)))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or (shape is not None and a.shape != tuple(shape)):
                raise ValueError('trajectory_lengths: an input of shape %s, not [trajectory, time] %s' % (a.shape, shape or ''))
            shape = a.shape
            keep.append(a)
            ptrs.append(C.c_void_p(a.ctypes.data))
        ntraj, nt = int(shape[0]), int(shape[1])
        total = np.zeros(ntraj)
        dims = (max(nt - 1, 0), ntraj)
        dist, speed = (np.zeros(dims), np.zeros(dims)) if segments else (None, None)
        check(self.lib.odr_trajectory_lengths(self.h, ntraj, nt, *ptrs, float(dt), total.ctypes.data_as(_dp),
                                              *(None if o is None else o.ctypes.data_as(_dp) for o in (dist, speed))))
        return (total, dist, speed) if segments else total

    def trajectory_lengths_last_kernel_ms(self):
        return self._last_kernel_ms('odr_trajectory_lengths_last_kernel_ms')

    def geod_npts(self, lon1, lat1, lon2, lat2, npts):
        """pyproj.Geod(ellps='WGS84').npts on the device (odr_geod_npts): (lon, lat) float64 arrays of the npts points at
        i * s12 / (npts + 1), i = 1 .. npts, on the geodesic from point 1 to point 2 -- both ends excluded."""
        npts = int(npts)
        lon, lat = np.empty(max(npts, 0)), np.empty(max(npts, 0))
        check(self.lib.odr_geod_npts(self.h, float(lon1), float(lat1), float(lon2), float(lat2), npts, lon.ctypes.data_as(_dp),
                                     lat.ctypes.data_as(_dp)))
        return lon, lat

    def points_in_polygon(self, x, y, vx, vy):
        """matplotlib.path.Path(np.c_[vx, vy]).contains_points(np.c_[x, y]) on the device (odr_points_in_polygon): a bool array."""
        x, y = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y))
        vx, vy = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (vx, vy))
        if len(x) != len(y) or len(vx) != len(vy):
            raise ValueError('points_in_polygon: %d x and %d y, %d vx and %d vy' % (len(x), len(y), len(vx), len(vy)))
        inside = np.zeros(len(x), np.uint8)
        check(self.lib.odr_points_in_polygon(self.h, len(x), x.ctypes.data_as(_dp), y.ctypes.data_as(_dp), len(vx),
                                             vx.ctypes.data_as(_dp), vy.ctypes.data_as(_dp), inside.ctypes.data_as(C.POINTER(C.c_uint8))))
        return inside.astype(bool)

    def points_within_polygon(self, lons, lats, number, info=False):
        """OpenDriftSimulation.points_within_polygon on the device (odr_polygon_points): (lonpoints, latpoints), `number` float64
        each; info=True adds dict(n_inside, nx, ny): the grid and how many of its points lie inside."""
        lons, lats = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (lons, lats))
        if len(lons) != len(lats):
            raise ValueError('lon and lat arrays must have same length.')
        number = int(number)
        lon, lat = np.empty(max(number, 0)), np.empty(max(number, 0))
        n_inside, nx, ny = C.c_int64(), C.c_int32(), C.c_int32()
        check(self.lib.odr_polygon_points(self.h, len(lons), lons.ctypes.data_as(_dp), lats.ctypes.data_as(_dp), number,
                                          lon.ctypes.data_as(_dp), lat.ctypes.data_as(_dp), C.byref(n_inside), C.byref(nx), C.byref(ny)))
        return (lon, lat, dict(n_inside=n_inside.value, nx=nx.value, ny=ny.value)) if info else (lon, lat)

    def polygon_points_last_kernel_ms(self):
        return self._last_kernel_ms('odr_polygon_points_last_kernel_ms')

    def umesh(self, x, y, xc=None, yc=None, proj=None, **sigma):
        """The device image of a triangular mesh (odr_umesh_create): UMesh."""
        return UMesh(self, x, y, xc, yc, proj=proj, **sigma)

    def umesh_last_kernel_ms(self):
        return self._last_kernel_ms('odr_umesh_last_kernel_ms')

    def schism(self, x, y, hull_x, hull_y, n_levels=0, proj=None):
        """The device image of a SCHISM-style mesh (odr_schism_create): SchismMesh."""
        return SchismMesh(self, x, y, hull_x, hull_y, n_levels=n_levels, proj=proj)

    def schism_last_kernel_ms(self):
        return self._last_kernel_ms('odr_schism_last_kernel_ms')

    def shape(self, x1, y1, x2, y2, poly, n_polygons, proj=None, invert=False, nx=0, ny=0):
        """The device image of coastline polygons (odr_shape_create): Shape."""
        return Shape(self, x1, y1, x2, y2, poly, n_polygons, proj=proj, invert=invert, nx=nx, ny=ny)

    def shape_last_kernel_ms(self):
        return self._last_kernel_ms('odr_shape_last_kernel_ms')

    def combined(self, ops):
        """The device program of a reader expression (odr_combined_create): Combined.  ops: (kind, index, (d0, d1, d2)) in postfix."""
        return Combined(self, ops)

    def combined_last_kernel_ms(self):
        return self._last_kernel_ms('odr_combined_last_kernel_ms')

    def particles(self, capacity):
        return Particles(self, capacity)

    def timer_begin(self):
        check(self.lib.odr_timer_begin(self.h))

    def timer_end(self):
        ms = C.c_float()
        check(self.lib.odr_timer_end(self.h, C.byref(ms)))
        return ms.value


class Particles:
    def __init__(self, ctx, capacity):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        check(self.lib.odr_particles_create(ctx.h, int(capacity), C.byref(self.h)))

    def close(self):
        if self.h and self.ctx.h:
            self.lib.odr_particles_destroy(self.ctx.h, self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.count()[0]

    def count(self):
        a, d = C.c_int64(), C.c_int64()
        check(self.lib.odr_particles_count(self.ctx.h, self.h, C.byref(a), C.byref(d)))
        return a.value, d.value

    def append(self, lon, lat, z=None, id=None, moving=None, wind_drift_factor=None,
               current_drift_factor=None, terminal_velocity=None):
        lon = np.atleast_1d(np.asarray(lon, dtype=np.float64))
        n = lon.size
        a = [_d(lon, n), _d(lat, n), _d(z, n), _i(id, n), _i(moving, n), _f(wind_drift_factor, n),
             _f(current_drift_factor, n), _f(terminal_velocity, n)]
        if id is None:                       # the device numbers them (active + deactivated so far) + 0 .. n-1
            act, dead = self.count()
            ids = act + dead + np.arange(n, dtype=np.int64)
        else:
            ids = np.atleast_1d(np.asarray(id, dtype=np.int64))
        check(self.lib.odr_particles_append(self.ctx.h, self.h, n, *[p for _, p in a]))
        # release sequence of every ID: the reference keeps its arrays in release order (move_elements appends the
        # scheduled elements as they are released, elements.py:197-228), which differs from ID order when the seed times
        # are not monotonic in ID; host-drawn random numbers (rng='numpy') arrive in that order (_host_order)
        seq = getattr(self, '_release_seq', None)
        top = int(ids.max()) + 1 if n else 0
        if seq is None or seq.size < top:
            new = np.full(max(top, 2 * (seq.size if seq is not None else 0), 1024), -1, np.int64)
            if seq is not None:
                new[:seq.size] = seq
            seq = self._release_seq = new
        k0 = getattr(self, '_release_count', 0)
        seq[ids] = k0 + np.arange(n)
        self._release_count = k0 + n

    def upload(self, lon=None, lat=None, z=None, moving=None, wind_drift_factor=None,
               current_drift_factor=None, terminal_velocity=None):
        n = len(self)
        a = [_d(lon, n), _d(lat, n), _d(z, n), _i(moving, n), _f(wind_drift_factor, n),
             _f(current_drift_factor, n), _f(terminal_velocity, n)]
        check(self.lib.odr_particles_upload(self.ctx.h, self.h, *[p for _, p in a]))

    def download(self):
        n = len(self)
        out = dict(lon=np.empty(n), lat=np.empty(n), z=np.empty(n), ID=np.empty(n, np.int32),
                   status=np.empty(n, np.int32), moving=np.empty(n, np.int32))
        check(self.lib.odr_particles_download(
            self.ctx.h, self.h, out['lon'].ctypes.data_as(_dp), out['lat'].ctypes.data_as(_dp),
            out['z'].ctypes.data_as(_dp), out['ID'].ctypes.data_as(_ip), out['status'].ctypes.data_as(_ip),
            out['moving'].ctypes.data_as(_ip)))
        return out

    def download_f32(self, name):
        """wind_drift_factor / current_drift_factor / terminal_velocity / age_seconds of the active elements"""
        out = np.empty(len(self), np.float32)
        check(self.lib.odr_particles_download_f32(self.ctx.h, self.h, name.encode(), out.ctypes.data_as(_fp)))
        return out

    def download_deactivated(self):
        n = self.count()[1]
        out = dict(lon=np.empty(n), lat=np.empty(n), z=np.empty(n), ID=np.empty(n, np.int32),
                   status=np.empty(n, np.int32))
        check(self.lib.odr_particles_download_deactivated(
            self.ctx.h, self.h, out['lon'].ctypes.data_as(_dp), out['lat'].ctypes.data_as(_dp),
            out['z'].ctypes.data_as(_dp), out['ID'].ctypes.data_as(_ip), out['status'].ctypes.data_as(_ip)))
        return out

    def device_ptr(self, name):
        p = C.c_void_p()
        check(self.lib.odr_particles_device_ptr(self.ctx.h, self.h, name.encode(), C.byref(p)))
        return p.value

    # ---- hot-path stages ----
    def env_sample(self, variables, t_epoch, download=False):
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        if download:
            n = len(self)
            outs = [np.empty(n, np.float32) for _ in variables]
            ptrs = (_fp * len(outs))(*[o.ctypes.data_as(_fp) for o in outs])
            check(self.lib.odr_env_sample(self.ctx.h, self.h, len(ids), pi, float(t_epoch), ptrs))
            return dict(zip(variables, outs))
        check(self.lib.odr_env_sample(self.ctx.h, self.h, len(ids), pi, float(t_epoch), None))

    def env_download(self, variable):
        out = np.empty(len(self), np.float32)
        check(self.lib.odr_env_download(self.ctx.h, self.h, self.ctx._vid(variable), out.ctypes.data_as(_fp)))
        return out

    def env_upload(self, variable, values):
        a, p = _f(values, len(self))
        check(self.lib.odr_env_upload(self.ctx.h, self.h, self.ctx._vid(variable), p))

    def umesh_sample(self, mesh, slot, variables, first):
        """The variables of the mesh's resident level `slot` at every element, merged into the environment slots in one launch
        (odr_umesh_sample): a finite value is taken where first[k] or where the slot holds nothing finite."""
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        if len(first) != len(ids):
            raise ValueError('%d variables and %d first flags' % (len(ids), len(first)))
        fl, pf = _i([int(bool(f)) for f in first])
        check(self.lib.odr_umesh_sample(self.ctx.h, self.h, mesh.ptr, int(slot), len(ids), pi, pf))

    def schism_sample(self, mesh, slot_before, slot_after, w, variables, first):
        """The inverse-distance mean over the three nearest points of the mesh's resident levels at every element, blended as
        before * (1 - w) + after * w (slot_after None: the level `slot_before` alone), merged into the environment slots in one
        launch (odr_schism_sample): a finite value is taken where first[k] or where the slot holds nothing finite."""
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        if len(first) != len(ids):
            raise ValueError('%d variables and %d first flags' % (len(ids), len(first)))
        fl, pf = _i([int(bool(f)) for f in first])
        check(self.lib.odr_schism_sample(self.ctx.h, self.h, mesh.ptr, int(slot_before), -1 if slot_after is None else int(slot_after),
                                         float(w), len(ids), pi, pf))

    def shape_sample(self, shape, first):
        """land_binary_mask of the polygons at every element, merged into the environment slot in one launch (odr_shape_sample):
        the value is taken where `first` or where the slot holds nothing finite; elements outside the box keep what they have."""
        check(self.lib.odr_shape_sample(self.ctx.h, self.h, shape.ptr, int(bool(first))))

    def combined_sample(self, combined, variables, first, t_epoch, uniform=None):
        """The expression's values at every element at time t_epoch, merged into the environment slots in one launch
        (odr_combined_sample): a finite value is taken where first[k] or where the slot holds nothing finite.  uniform:
        [variable][uniform leaf] values of the program's uniform leaves."""
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        if len(first) != len(ids):
            raise ValueError('%d variables and %d first flags' % (len(ids), len(first)))
        fl = np.ascontiguousarray([bool(f) for f in first], dtype=np.uint8)
        uni = np.zeros((len(ids), 0)) if uniform is None else np.ascontiguousarray(uniform, dtype=np.float64)
        if uni.ndim != 2 or uni.shape[0] != len(ids):
            raise ValueError('uniform values of shape %s for %d variables' % (uni.shape, len(ids)))
        check(self.lib.odr_combined_sample(self.ctx.h, self.h, combined.ptr, len(ids), pi, fl.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           float(t_epoch), uni.shape[1], uni.ctypes.data_as(_dp) if uni.size else None))

    def env_add_noise(self, var_x, var_y, std, step=0, normals=None, uniform=False):
        """drift:current_uncertainty / wind_uncertainty (normal) or drift:current_uncertainty_uniform (uniform=True) on
        the last sample (environment.py:869-891).  normals: the caller's np.random draws (x, y), already scaled."""
        n = len(self)
        dist = _abi.NOISE_UNIFORM if uniform else _abi.NOISE_NORMAL
        if normals is not None:
            (ax, px), (ay, py) = _d(self._host_order(normals[0]), n), _d(self._host_order(normals[1]), n)
            check(self.lib.odr_env_add_noise(self.ctx.h, self.h, self.ctx._vid(var_x), self.ctx._vid(var_y), float(std), dist,
                                             _abi.RNG_HOST, px, py, step))
        else:
            check(self.lib.odr_env_add_noise(self.ctx.h, self.h, self.ctx._vid(var_x), self.ctx._vid(var_y), float(std), dist,
                                             _abi.RNG_DEVICE, None, None, step))

    def set_advect_noise(self, std_normal=0.0, std_uniform=0.0, step=0, stage_draws=None, main_draws=None):
        """drift:current_uncertainty(_uniform) inside the next advect() / env_coast_advect() (odr_advect_set_noise): the
        reference adds them in the Runge-Kutta stage get_environment calls too (physics_methods.py:638-670).
        stage_draws [nstage][ncomp][n] / main_draws [ncomp][n]: np.random draws in the reference's order (parity mode);
        None: Philox on the device."""
        if stage_draws is None and main_draws is None:
            check(self.lib.odr_advect_set_noise(self.ctx.h, self.h, float(std_normal), float(std_uniform), _abi.RNG_DEVICE,
                                                None, None, 0, step))
            return
        ps = pm = None
        nstage = 0
        if stage_draws is not None:
            sd, ps = _d(np.ascontiguousarray(self._host_order(np.asarray(stage_draws, dtype=np.float64))))
            nstage = sd.shape[0]
        if main_draws is not None:
            md, pm = _d(np.ascontiguousarray(self._host_order(np.asarray(main_draws, dtype=np.float64))))
        check(self.lib.odr_advect_set_noise(self.ctx.h, self.h, float(std_normal), float(std_uniform), _abi.RNG_HOST,
                                            pm, ps, nstage, step))

    def advect(self, scheme, t_epoch, dt, factor=1.0):
        s = scheme if isinstance(scheme, int) else _abi.SCHEME.get(scheme, -1)
        if s < 0:
            raise ValueError('Drift scheme not recognised: ' + str(scheme))
        check(self.lib.odr_advect(self.ctx.h, self.h, s, float(t_epoch), float(dt), float(factor)))

    def env_coast_advect(self, variables, t_epoch, scheme, dt, coastline='none', stranded_code=1,
                         seeded_on_land_code=0, store_previous=True, factor=1.0, count=True, seafloor=False,
                         age_dt=0.0, max_age_seconds=0.0, retired_code=0, missing_code=0, main_noise=False, vmix=None):
        """env_sample -> coastline -> store_previous -> advect in one launch (odr_env_coast_advect).
        count=False skips reading back the number of elements on land (no host synchronisation).  seafloor=True and
        age_dt != 0 add interact_with_seafloor ('lift_to_seafloor') and increase_age_and_retire, in the loop's order."""
        s = scheme if isinstance(scheme, int) else _abi.SCHEME.get(scheme, -1)
        if s < 0:
            raise ValueError('Drift scheme not recognised: ' + str(scheme))
        a = coastline if isinstance(coastline, int) else _abi.COAST[coastline]
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        n = C.c_int64()
        ex = None
        if seafloor or age_dt or missing_code or main_noise or vmix:
            # vmix = dict(dt_mix=, step=, mix_at_surface=False, vertical_advection=None | False (below the surface) | True):
            # OceanDrift.vertical_mixing (+ vertical_advection) of the same step inside the call (device RNG)
            m = vmix or {}
            va = m.get('vertical_advection')
            ex = C.byref(_abi.StepExtras(1 if seafloor else 0, int(retired_code), float(age_dt), float(max_age_seconds),
                                         int(missing_code), 1 if main_noise else 0, 1 if vmix else 0,
                                         int(bool(m.get('mix_at_surface', False))), -1 if va is None else int(bool(va)), 0,
                                         float(m.get('dt_mix', 0.0)), int(m.get('step', 0))))
        check(self.lib.odr_env_coast_advect(self.ctx.h, self.h, len(ids), pi, float(t_epoch), a, stranded_code,
                                            seeded_on_land_code, int(bool(store_previous)), s, float(dt),
                                            float(factor), ex, C.byref(n) if count else None))
        return n.value if count else None

    def set_rank_offset(self, offset):
        """Present elements with smaller IDs held by other particle sets (the lower ranks of a sharded run): added to the
        rank among the present elements that selects the ensemble member (odr_particles_set_rank_offset)."""
        check(self.lib.odr_particles_set_rank_offset(self.ctx.h, self.h, int(offset)))

    def update_positions(self, x_vel, y_vel, dt):
        n = len(self)
        is32 = int(np.asarray(x_vel).dtype == np.float32)
        (a, pa), (b, pb) = _d(x_vel, n), _d(y_vel, n)
        check(self.lib.odr_update_positions(self.ctx.h, self.h, pa, pb, is32, float(dt)))

    def advect_wind(self, dt, wind_drift_depth=0.1, relative_wind=False, factor=1.0):
        check(self.lib.odr_advect_wind(self.ctx.h, self.h, float(dt), float(wind_drift_depth),
                                       int(relative_wind), float(factor)))

    ELEMENT_FACTORS = {None: 0, 'scalar': 0, 'ice_current': 1, 'ice_stokes': 2, 'ice_drift': 3}

    def set_element_factor(self, kind):
        """Per-element factors of the following movers from the sampled sea_ice_area_fraction (OpenOil.advect_oil,
        openoil.py:1179-1216): 'ice_current' (advect, advect_wind), 'ice_stokes' (stokes_drift), 'ice_drift'
        (advect_sea_ice); None: the scalar `factor` arguments again."""
        check(self.lib.odr_set_element_factor(self.ctx.h, self.h, self.ELEMENT_FACTORS[kind]))

    def advect_sea_ice(self, dt, factor=1.0):
        check(self.lib.odr_advect_sea_ice(self.ctx.h, self.h, float(dt), float(factor)))

    def stokes_drift(self, dt, profile=2, hs_mode=0, tp_mode=0, factor=1.0):
        check(self.lib.odr_stokes_drift(self.ctx.h, self.h, float(dt), profile, hs_mode, tp_mode, float(factor)))

    def set_property(self, slot, values, offset=0):
        a, pa = _f(np.atleast_1d(values))
        check(self.lib.odr_particles_set_property(self.ctx.h, self.h, slot, int(offset), a.size, pa))

    def get_property(self, slot):
        out = np.empty(len(self), np.float32)
        check(self.lib.odr_particles_get_property(self.ctx.h, self.h, slot, out.ctypes.data_as(_fp)))
        return out

    def ids(self):
        n = len(self)
        out = np.empty(n, np.int32)
        check(self.lib.odr_particles_download(self.ctx.h, self.h, None, None, None, out.ctypes.data_as(_ip), None, None))
        return out

    def _ref_key(self, ids):
        """Sort key that puts elements in the reference's array order: the release sequence (ID where unknown)."""
        seq = getattr(self, '_release_seq', None)
        if seq is not None and ids.size and ids.max() < seq.size and (seq[ids] >= 0).all():
            return seq[ids]
        return ids

    def _host_order(self, arr):
        """Host-drawn random numbers (RNG_HOST parity mode) arrive in the reference's element order,
        i.e. release order of the active elements (= ascending ID unless the seed times are not monotonic in ID); in-place compaction and spatial sorting permute the
        device arrays, so the numbers are gathered into device order first."""
        n = len(self)
        a = np.asarray(arr)[..., :n]
        if not getattr(self, '_permuted', False):
            return a
        key = self._ref_key(self.ids())
        rank = np.empty(n, np.int64)
        rank[np.argsort(key, kind='stable')] = np.arange(n)
        return np.ascontiguousarray(a[..., rank])

    def leeway_capsize(self, dt, wind_threshold=30.0, wind_threshold_sigma=5.0, step=0, uniforms=None):
        """processes:capsizing (leeway.py:438-455).  uniforms (RNG_HOST parity mode) = np.random.rand(len(can_be_capsized))
        in the reference's order (ascending ID of the elements that can be capsized)."""
        if uniforms is not None:
            n = len(self)
            cap = self.get_property(8)
            can = np.nonzero(cap == (0.0 if dt >= 0 else 1.0))[0]
            order = can[np.argsort(self._ref_key(self.ids()[can]), kind='stable')]      # reference order of those elements
            full = np.zeros(n)
            full[order] = np.asarray(uniforms, dtype=np.float64)[:len(order)]
            a, pa = _d(full, n)
            check(self.lib.odr_leeway_capsize(self.ctx.h, self.h, float(dt), float(wind_threshold),
                                              float(wind_threshold_sigma), _abi.RNG_HOST, pa, step))
        else:
            check(self.lib.odr_leeway_capsize(self.ctx.h, self.h, float(dt), float(wind_threshold),
                                              float(wind_threshold_sigma), _abi.RNG_DEVICE, None, step))

    def leeway(self, dt, capsize_fraction=0.4, step=0, uniforms=None):
        if uniforms is not None:
            u, pu = _d(self._host_order(uniforms), len(self))
            check(self.lib.odr_leeway(self.ctx.h, self.h, float(dt), float(capsize_fraction), _abi.RNG_HOST, pu, step))
        else:
            check(self.lib.odr_leeway(self.ctx.h, self.h, float(dt), float(capsize_fraction), _abi.RNG_DEVICE, None, step))

    def env_coast_leeway(self, variables, t_epoch, dt, capsize_fraction=0.4, coastline='stranding', stranded_code=1,
                         seeded_on_land_code=0, store_previous=False, current_uncertainty=0.0, wind_uncertainty=0.0, step=0,
                         split='finish', missing_code=0, count=True):
        """The Leeway loop body between two compactions in one launch (odr_env_coast_leeway): sample, uncertainties (device
        RNG), coastline, previous state, Leeway.update.  When wind / current / landmask do not come from one gridded reader the
        library has sampled, perturbed and applied the coastline only: compaction and Leeway.update follow here, so that
        env_coast_leeway() + compact() is the same sequence either way.  Returns the number of elements on land.
        split='return': in that case nothing more is done here and (elements on land, True) comes back -- the caller compacts
        (after whatever it does between coastline and update) and calls leeway() itself; (elements on land, False) otherwise."""
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        nhit = C.c_int64()
        if missing_code:     # report_missing_variables inside the call (status of an element without data)
            check(self.lib.odr_leeway_set_missing_code(self.ctx.h, int(missing_code)))
        rc = self.lib.odr_env_coast_leeway(self.ctx.h, self.h, len(variables), pi, float(t_epoch), _abi.COAST[coastline],
                                           int(stranded_code), int(seeded_on_land_code), int(bool(store_previous)), float(dt),
                                           float(capsize_fraction), float(current_uncertainty), float(wind_uncertainty), int(step),
                                           C.byref(nhit) if count else None)      # count=False: no host synchronisation
        if rc == 1:          # ODR_SPLIT_LANE
            if split == 'return':
                return nhit.value, True
            self.compact()
            self.leeway(dt, capsize_fraction, step=step)
        else:
            check(rc)
        return (nhit.value, False) if split == 'return' else nhit.value

    def hdiffusion(self, dt, step=0, normals=None):
        n = len(self)
        if normals is not None:
            (ax, px), (ay, py) = _d(self._host_order(normals[0]), n), _d(self._host_order(normals[1]), n)
            check(self.lib.odr_hdiffusion(self.ctx.h, self.h, float(dt), _abi.RNG_HOST, px, py, step))
        else:
            check(self.lib.odr_hdiffusion(self.ctx.h, self.h, float(dt), _abi.RNG_DEVICE, None, None, step))

    def movers(self, dt, wind=None, stokes=None, hdiffusion=None):
        """advect_wind -> stokes_drift -> horizontal_diffusion in one launch (odr_movers).  Each argument is None (mover not
        applied) or the keyword arguments of the method of that name: wind=dict(wind_drift_depth=0.1, relative_wind=False,
        factor=1.0), stokes=dict(profile=2, hs_mode=0, tp_mode=0, factor=1.0), hdiffusion=dict(step=0, normals=None)."""
        which = (1 if wind is not None else 0) | (2 if stokes is not None else 0) | (4 if hdiffusion is not None else 0)
        w, s, h = wind or {}, stokes or {}, hdiffusion or {}
        px = py = None
        mode = _abi.RNG_DEVICE
        if h.get('normals') is not None:
            n = len(self)
            (ax, px), (ay, py) = _d(self._host_order(h['normals'][0]), n), _d(self._host_order(h['normals'][1]), n)
            mode = _abi.RNG_HOST
        check(self.lib.odr_movers(self.ctx.h, self.h, float(dt), which, float(w.get('wind_drift_depth', 0.1)),
                                  int(bool(w.get('relative_wind', False))), float(w.get('factor', 1.0)),
                                  int(s.get('profile', 2)), int(s.get('hs_mode', 0)), int(s.get('tp_mode', 0)),
                                  float(s.get('factor', 1.0)), mode, px, py, int(h.get('step', 0))))

    def snapshot_property(self, slot):
        """Device copy of one property as it is now, read by the next History.record(position_from_previous=3)."""
        check(self.lib.odr_particles_snapshot_property(self.ctx.h, self.h, int(slot)))

    def vmix(self, t_epoch, dt, dt_mix, mix_at_surface=False, step=0, uniforms=None, fuse_vertical_advection=None, guarded=False,
             profile_levels=0):
        """guarded=True (between scan_status_begin and scan_status_end): the launch does nothing unless the fold finds that every
        element stays (odr_ctx_guard_next_vmix); returns False when the library could not launch it that way (nothing happened)."""
        if fuse_vertical_advection is not None:   # True: include surface elements, False: z<0 only
            check(self.lib.odr_vmix_fuse_vertical_advection(self.ctx.h, int(bool(fuse_vertical_advection))))
        if profile_levels:     # the K columns end there (a reader that cut its block at the depth asked of it, odr_vmix_set_profile_levels)
            check(self.lib.odr_vmix_set_profile_levels(self.ctx.h, int(profile_levels)))
        if guarded:
            assert uniforms is None
            check(self.lib.odr_ctx_guard_next_vmix(self.ctx.h, 1))
            rc = self.lib.odr_vmix(self.ctx.h, self.h, float(t_epoch), float(dt), float(dt_mix), int(mix_at_surface), _abi.RNG_DEVICE, None, step)
            if rc < 0:
                check(rc)
            return rc == 0
        if uniforms is not None:
            u, pu = _d(np.ascontiguousarray(self._host_order(uniforms)))
            check(self.lib.odr_vmix(self.ctx.h, self.h, float(t_epoch), float(dt), float(dt_mix),
                                    int(mix_at_surface), _abi.RNG_HOST, pu, step))
        else:
            check(self.lib.odr_vmix(self.ctx.h, self.h, float(t_epoch), float(dt), float(dt_mix),
                                    int(mix_at_surface), _abi.RNG_DEVICE, None, step))

    def vmix_analytic(self, model, background_diffusivity, dt, dt_mix, mix_at_surface=False, step=0, uniforms=None,
                      fuse_vertical_advection=None):
        """vertical_mixing with 'windspeed_Large1994' / 'windspeed_Sundby1983' profiles (oceandrift.py:385-395,448-458)."""
        if model not in _abi.DIFFUSIVITY:
            raise ValueError('Unknown diffusivity model: ' + str(model))      # oceandrift.py:395
        if fuse_vertical_advection is not None:
            check(self.lib.odr_vmix_fuse_vertical_advection(self.ctx.h, int(bool(fuse_vertical_advection))))
        pu, mode = None, _abi.RNG_DEVICE
        if uniforms is not None:
            u, pu = _d(np.ascontiguousarray(self._host_order(uniforms)))
            mode = _abi.RNG_HOST
        check(self.lib.odr_vmix_wind_profile(self.ctx.h, self.h, _abi.DIFFUSIVITY[model], float(background_diffusivity),
                                             float(dt), float(dt_mix), int(mix_at_surface), mode, pu, step))

    def oil_prepare_mixing(self, dt, dt_mix, interfacial_tension, distribution, sea_water_density, keep_droplet_diameter=False,
                           hs_mode=1, tp_mode=3, temperature_to_kelvin=True, step=0, uniforms=None):
        """OpenOil.prepare_vertical_mixing on the device (openoil.py:1017-1031); the next vmix / vmix_analytic call runs
        OpenOil's version of the mixing loop.  uniforms (np.random parity): dict(diameter [n], entrain [nt, n],
        intrusion [nt, n])."""
        if distribution not in _abi.DROPLETS:
            raise ValueError('no wave entrainment droplet size distribution specified')      # openoil.py:1070
        pd = pe = pi = None
        mode = _abi.RNG_DEVICE
        if uniforms is not None:
            d, pd = _d(np.ascontiguousarray(self._host_order(uniforms['diameter'])))
            e, pe = _d(np.ascontiguousarray(self._host_order(uniforms['entrain'])))
            i, pi = _d(np.ascontiguousarray(self._host_order(uniforms['intrusion'])))
            mode = _abi.RNG_HOST
        check(self.lib.odr_oil_prepare_mixing(self.ctx.h, self.h, float(dt), float(dt_mix), float(interfacial_tension),
                                              float(sea_water_density), _abi.DROPLETS[distribution],
                                              int(bool(keep_droplet_diameter)), int(hs_mode), int(tp_mode),
                                              int(bool(temperature_to_kelvin)), mode, pd, pe, pi, step))

    def oil_global_stats(self, allreduce_sum, interfacial_tension, distribution, sea_water_density, hs_mode=1):
        """Sharded run: np.mean(dV_50) and np.mean(1.5 Hs) over the elements of ALL ranks, installed for the next
        oil_prepare_mixing (odr_oil_local_sums / odr_oil_set_mixing_stats)."""
        a, b = C.c_double(), C.c_double()
        check(self.lib.odr_oil_local_sums(self.ctx.h, self.h, float(interfacial_tension), float(sea_water_density),
                                          _abi.DROPLETS[distribution], int(hs_mode), C.byref(a), C.byref(b)))
        g = allreduce_sum([a.value, b.value, float(len(self))])
        if g[2] > 0:
            check(self.lib.odr_oil_set_mixing_stats(self.ctx.h, g[1] / g[2], g[0] / g[2]))

    def oil_mixing_stats(self):
        a, b = C.c_double(), C.c_double()
        check(self.lib.odr_oil_mixing_stats(self.ctx.h, C.byref(a), C.byref(b)))
        return dict(mean_zb=a.value, dV_50=b.value)

    def vmix_oil(self, model, background_diffusivity, dt, dt_mix, interfacial_tension, distribution, sea_water_density=None,
                 t_epoch=0.0, uniforms=None, step=0, mix_at_surface=False, profile_levels=0, **kw):
        """prepare_vertical_mixing + vertical_mixing as OpenOil.update runs them (openoil.py:1228-1231).  model: a wind
        parameterisation of the diffusivity or 'environment' (profiles from a reader)."""
        if sea_water_density is None:
            sea_water_density = sea_water_density_default()
        self.oil_prepare_mixing(dt, dt_mix, interfacial_tension, distribution, sea_water_density, step=step,
                                uniforms=uniforms, **kw)
        mix = None if uniforms is None else uniforms['mix']
        if model in ('environment', 'constant'):
            self.vmix(t_epoch, dt, dt_mix, mix_at_surface=mix_at_surface, step=step, uniforms=mix,
                      profile_levels=profile_levels if model == 'environment' else 0)
        else:
            self.vmix_analytic(model, background_diffusivity, dt, dt_mix, mix_at_surface=mix_at_surface, step=step, uniforms=mix)

    def egg_terminal_velocity(self, diameter_slot=0, salinity_slot=1):
        """PelagicEggDrift.update_terminal_velocity (pelagicegg.py:100-179): terminal_velocity of every element from the sampled
        sea_water_temperature / sea_water_salinity and the two property slots (egg diameter, salinity of neutral buoyancy)."""
        check(self.lib.odr_egg_terminal_velocity(self.ctx.h, self.h, int(diameter_slot), int(salinity_slot)))

    def stokes_from_wind(self, stokes_coeff=None, hs_coeff=None):
        """drift:use_tabularised_stokes_drift (environment.py:844-863): the Stokes drift (stokes_coeff given: the 1 .. 7
        coefficients of the drift factor, leading one first) and / or the significant wave height (hs_coeff given: its two) of
        every active element from the sampled wind, in ONE launch (odr_stokes_from_wind)."""
        flags = (_abi.PLAST_STOKES if stokes_coeff is not None else 0) | (_abi.PLAST_HS if hs_coeff is not None else 0)
        if not flags:
            raise ValueError('neither the coefficients of the drift factor nor those of the wave height were given')
        (sa, ps), (ha, ph) = _d(stokes_coeff), _d(hs_coeff)
        if ha is not None and ha.shape != (2,):
            raise ValueError('the wave height has two coefficients, not %s' % (ha.shape,))
        if sa is not None and (sa.ndim != 1 or not 1 <= len(sa) <= 7):
            raise ValueError('the drift factor has 1 .. 7 coefficients, not %s' % (sa.shape,))
        check(self.lib.odr_stokes_from_wind(self.ctx.h, self.h, ps, 0 if sa is None else len(sa), ph, flags))

    def wave_maxima(self):
        """(max Stokes x, max Stokes y, max wave height) over the active elements: the plain maxima environment.py:847-858 asks
        about (-inf: not sampled / no active element), from the movers' reduction (odr_reduce_wave_maxima)."""
        out = np.empty(3)
        check(self.lib.odr_reduce_wave_maxima(self.ctx.h, self.h, out.ctypes.data_as(_dp)))
        return tuple(float(v) for v in out)

    def plast_depth(self, step=0, draws=None):
        """PlastDrift.update_particle_depth, 'analytical' (plastdrift.py:102-107): z = -(K / terminal_velocity) E for every active
        element.  draws: np.random.standard_exponential(n) in the reference's element order (parity mode); None: the device
        generator.  ValueError -- and no z changed -- when K / terminal_velocity is negative for some element, as NumPy raises."""
        if draws is not None:
            a, pa = _d(self._host_order(draws), len(self))
            check(self.lib.odr_plast_depth(self.ctx.h, self.h, _abi.RNG_HOST, pa, step))
        else:
            check(self.lib.odr_plast_depth(self.ctx.h, self.h, _abi.RNG_DEVICE, None, step))

    def larval_update(self, dt, stage_fraction_slot=2, hatched_slot=3, weight_slot=5, length_slot=4):
        """LarvalFish.update_fish_larvae (larvalfish.py:200-231, with fish_growth :185-198) over the active set: eggs add to
        stage_fraction and hatch at >= 1, larvae grow in weight and get their length from it.  `hatched` is uint8 in the
        reference; here it is a float32 property slot holding 0 (egg) or 1 (larva), like PelagicEggDrift's."""
        check(self.lib.odr_larval_update(self.ctx.h, self.h, int(stage_fraction_slot), int(hatched_slot), int(weight_slot),
                                         int(length_slot), float(dt)))

    def larval_migrate(self, dt, fraction_swimming, direction, hatched_slot=3, length_slot=4):
        """LarvalFish.larvae_vertical_migration (larvalfish.py:233-253): every larva (hatched slot == 1) swims for
        `fraction_swimming` of the time step, down (direction -1) or up (+1), not above z = 0."""
        check(self.lib.odr_larval_migrate(self.ctx.h, self.h, int(hatched_slot), int(length_slot), float(fraction_swimming),
                                          float(dt), int(direction)))

    def solar_elevation(self, declination_rad, time_offset_minutes, day_minutes):
        """OceanDrift.solar_elevation (physics_methods.py:977-979, :1036-1043): the solar elevation [deg] of the active elements,
        float64.  The three scalars depend on the time only (oceandrift.solar_time_scalars)."""
        out = np.zeros(len(self), np.float64)
        check(self.lib.odr_solar_elevation(self.ctx.h, self.h, float(declination_rad), float(time_offset_minutes), float(day_minutes),
                                           out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def larvalx_hatch(self, increment, stage_fraction_slot=0, hatched_slot=1):
        """LarvalFishExtended.update_fish_larvae (larvalfish_extended.py:292-318) over the active set: eggs add float32(increment)
        = (dt / 86400) / hatch_time_days to stage_fraction and hatch at >= 1.  `hatched` is uint8 in the reference; here it is a
        float32 property slot holding 0 (egg) or 1 (larva), like LarvalFish's."""
        check(self.lib.odr_larvalx_hatch(self.ctx.h, self.h, int(stage_fraction_slot), int(hatched_slot), float(increment)))

    def larvalx_behave(self, mode, dt, w_active, band0, band1=(0.0, 0.0), solar=(0.0, 0.0, 0.0), active_only_hatched=True,
                       z_is_float32=False, hatched_slot=1):
        """LarvalFishExtended._apply_vertical_behavior (larvalfish_extended.py:206-290) in one launch.  mode 'depth': every moving
        element goes towards band0; 'dvm': towards band1 (day) where its solar elevation is > 0, else band0 (night).  A band is
        (centre, half-width); solar: the three scalars of solar_elevation.  active_only_hatched: only larvae (hatched slot == 1)
        move, else every element.  z_is_float32: the reference's roundings while it holds z in float32 (no mixing has run)."""
        check(self.lib.odr_larvalx_behave(self.ctx.h, self.h, int(hatched_slot), _abi.LARVALX_MODES[mode], int(bool(active_only_hatched)),
                                          int(bool(z_is_float32)), float(band0[0]), float(band0[1]), float(band1[0]), float(band1[1]),
                                          float(w_active), float(dt), float(solar[0]), float(solar[1]), float(solar[2])))

    def berg_roll_over(self, sail_slot=0, draft_slot=1, length_slot=2, width_slot=3):
        """OpenBerg.roll_over (openberg.py:587-614) over the active set: length >= width, bergs that fail the stability criterion of
        Wagner et al. roll, and every berg's thickness is split again into draft and sail."""
        check(self.lib.odr_berg_roll_over(self.ctx.h, self.h, int(sail_slot), int(draft_slot), int(length_slot), int(width_slot)))

    def berg_advect(self, dt, weight_coef=1.0, water_form_drag_coef=0.25, water_skin_drag_coef=0.0055, wind_form_drag_coef=0.8,
                    wind_skin_drag_coef=0.0022, wave_drag_coef=0.3, wave_from_direction=0.0, sea_ice_thickness=0.0, wave_rad=True,
                    stokes_drift=False, coriolis=True, grounding=True, lat_is_float32=False, sail_slot=0, draft_slot=1, length_slot=2, width_slot=3,
                    x_velocity_slot=4, y_velocity_slot=5, velocity_f64=False):
        """OpenBerg.advect_iceberg with surface currents (openberg.py:427-552): grounding, the momentum balance of every berg
        integrated over `dt` with SciPy's RK45 over the whole active set, positions and the two velocity slots.  Returns
        (attempts, rejected attempts) of the solve; with velocity_f64 also the float64 velocities (x, y) of the active elements in
        device order, as the positions were moved with them."""
        na, nr = C.c_int32(), C.c_int32()
        vel = np.empty((2, len(self)), np.float64) if velocity_f64 else None
        # IcebergObj declares the coefficients float32: the reference's float64 arrays hold float32 values (0.8 is 0.800000011920929)
        (weight_coef, water_form_drag_coef, water_skin_drag_coef, wind_form_drag_coef, wind_skin_drag_coef, wave_drag_coef) = (
            float(np.float32(v)) for v in (weight_coef, water_form_drag_coef, water_skin_drag_coef, wind_form_drag_coef, wind_skin_drag_coef,
                                           wave_drag_coef))
        check(self.lib.odr_berg_advect(self.ctx.h, self.h, int(sail_slot), int(draft_slot), int(length_slot), int(width_slot),
                                       int(x_velocity_slot), int(y_velocity_slot), float(weight_coef), float(water_form_drag_coef),
                                       float(water_skin_drag_coef), float(wind_form_drag_coef), float(wind_skin_drag_coef),
                                       float(wave_drag_coef), float(wave_from_direction), float(sea_ice_thickness), int(bool(wave_rad)),
                                       int(bool(stokes_drift)), int(bool(coriolis)), int(bool(grounding)), int(bool(lat_is_float32)), float(dt), C.byref(na),
                                       C.byref(nr), vel.ctypes.data_as(C.c_void_p) if velocity_f64 else None))
        if velocity_f64:
            return na.value, nr.value, vel[0], vel[1]
        return na.value, nr.value

    SHIP_INTERMEDIATES = ('F_wave_b', 'beta2_b', 'F_wave', 'beta2', 'wave_dir', 'F_total', 'uw_tot', 'uw_dir', 'velocity_u', 'velocity_v')

    def ship_table(self, table):
        """The class tables of ShipDrift on the device (odr_ship_table_create): table[n_classes][49][2] float64, F and D of the
        reference's interpolators at the 49 spectrum points below omega = 7.  Returns a ShipTable (free it with close())."""
        return ShipTable(self.ctx, table)

    def ship_drift(self, dt, table, hs_mode=1, tp_mode=3, wave_dir_from_stokes=False, stranded_code=1, length_slot=0, height_slot=1,
                   draft_slot=2, beam_slot=3, wind_drag_slot=4, water_drag_slot=5, orientation_slot=6, class_slot=7, check_classes=True,
                   intermediates=False):
        """ShipDrift.update (shipdrift.py:216-343) over the active set in one launch: the move with the current, wind force, wave
        force and damping from the spectrum and the class tables, the four damping iterations, the move with the drift velocity,
        stranding.  table: a ShipTable.  check_classes: every element's class index is read back and checked against the table
        (one download); a caller that built the indices with the table passes False.  intermediates: returns the float64
        intermediates of the active elements in device order, {name: array} (the host waits for the launch)."""
        if check_classes and len(self):
            k = self.get_property(class_slot)
            if not (np.all(k == np.floor(k)) and k.min() >= 0 and k.max() < table.n_classes):
                raise ValueError('ship_drift: class indices %s..%s, the table has %d classes' % (k.min(), k.max(), table.n_classes))
        rep = np.empty((len(self.SHIP_INTERMEDIATES), len(self)), np.float64) if intermediates else None
        check(self.lib.odr_ship_drift(self.ctx.h, self.h, int(length_slot), int(height_slot), int(draft_slot), int(beam_slot),
                                      int(wind_drag_slot), int(water_drag_slot), int(orientation_slot), int(class_slot), table.ptr,
                                      int(hs_mode), int(tp_mode), int(bool(wave_dir_from_stokes)), int(stranded_code),
                                      float(dt), rep.ctypes.data_as(C.c_void_p) if intermediates else None))
        if intermediates:
            return dict(zip(self.SHIP_INTERMEDIATES, rep))

    def resuspend(self, threshold, count=True):
        """SedimentDrift.resuspension (sedimentdrift.py:118-126): settled elements (moving == 0) whose sampled current speed
        exceeds `threshold` (compared as float32, like NumPy 2) move again, 1 cm up.  Returns how many (count=False: None,
        and the host does not wait)."""
        n = C.c_int64()
        check(self.lib.odr_resuspend(self.ctx.h, self.h, C.c_float(np.float32(threshold)), C.byref(n) if count else None))
        return n.value if count else None

    def radio_setup(self, **setup):
        """The species setup of RadionuclideDrift on the device with its transformation counters (odr_radio_create): the members
        of odr_radio_setup by name (include/odrift.h), `rates` as [nsalinity][nspecies][nspecies] or [nspecies][nspecies].
        Returns a RadioSetup (counts() reads the counters, close() frees it)."""
        return RadioSetup(self.ctx, **setup)

    @staticmethod
    def _draws(arrays, n):
        out = []
        for a in arrays:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (n,):
                raise ValueError('host draws of shape %s for %d elements' % (a.shape, n))
            out.append(a)
        return out

    def radio_speciation(self, setup, dt, conc3='conc3', specie_slot=3, diameter_slot=0, step=0, u1=None, u2=None, diameter_noise=None,
                         depth_noise=None):
        """RadionuclideDrift.update_transfer_rates + update_speciation (radionuclides.py:728-860, :866-902) over the active set:
        every element may change its species; a new particle or dissolved element gets a new diameter, sorption puts it on the
        sea bed (moving 0), desorption takes it off.  conc3: the variable whose slot carries conc3 (Context.slot_aliases).  With
        u1 (one uniform per element) the numbers are the caller's -- u2, diameter_noise, depth_noise too, one per element --
        else Philox streams keyed by (ID, step)."""
        host = u1 is not None
        d = self._draws((u1, u2, diameter_noise, depth_noise), len(self)) if host else [None] * 4
        check(self.lib.odr_radio_speciation(self.ctx.h, self.h, setup.ptr, int(specie_slot), int(diameter_slot), self.ctx._vid(conc3),
                                            float(dt), _abi.RNG_HOST if host else _abi.RNG_DEVICE,
                                            *[a.ctypes.data_as(_dp) if host else None for a in d], int(step)))

    def radio_terminal_velocity(self, diameter_slot=0, density_slot=2):
        """RadionuclideDrift.update_terminal_velocity without profiles (radionuclides.py:665-721): Stokes' law from the sampled
        temperature and salinity and the element's diameter and density, times moving."""
        check(self.lib.odr_radio_terminal_velocity(self.ctx.h, self.h, int(diameter_slot), int(density_slot)))

    def radio_resuspend(self, setup, specie_slot=3, diameter_slot=0, step=0, diameter_noise=None, depth_noise=None):
        """The change of species of RadionuclideDrift.bottom_interaction for the elements the sea-floor action 'settle_species' has
        settled, then resuspension (radionuclides.py:912-942, :946-997).  With diameter_noise / depth_noise (one per element) the
        numbers are the caller's, else Philox streams keyed by (ID, step)."""
        host = depth_noise is not None
        d = self._draws((diameter_noise, depth_noise), len(self)) if host else [None] * 2
        check(self.lib.odr_radio_resuspend(self.ctx.h, self.h, setup.ptr, int(specie_slot), int(diameter_slot),
                                           _abi.RNG_HOST if host else _abi.RNG_DEVICE, *[a.ctypes.data_as(_dp) if host else None for a in d],
                                           int(step)))

    def weathering_setup(self, oil, n_total, sea_water_density=None):
        """OpenOil.prepare_run for the NOAA weathering (openoil.py:682-693): the oil as a table (weathering_table's dict) and a zeroed
        side table for n_total elements, indexed by element ID (odr_oil_weathering_setup)."""
        t = weathering_table(oil, sea_water_density_default() if sea_water_density is None else sea_water_density)
        check(self.lib.odr_oil_weathering_setup(self.ctx.h, self.h, C.byref(t), int(n_total)))
        self._weather_ncomp, self._weather_n_total = int(t.ncomp), int(n_total)

    def weathering_seed(self, id0, mass_oil, mass_fraction, density, viscosity, oil_film_thickness=0.001, bulltime=0.0,
                        biodegradation_half_time_droplet=1.0, biodegradation_half_time_slick=3.0):
        """The rows [id0, id0 + len(mass_oil)) as seed_elements and prepare_run leave them (openoil.py:1726-1755, :686-691):
        mass_components = mass_fraction * mass_oil, the other masses, water_fraction and interfacial_area 0."""
        mass_oil = np.atleast_1d(np.asarray(mass_oil, np.float64))
        n = mass_oil.size
        rec = np.zeros((n, _abi.WEATHER_RECORD_N))
        for name, v in (('mass_oil', mass_oil), ('density', density), ('viscosity', viscosity), ('oil_film_thickness', oil_film_thickness),
                        ('bulltime', bulltime), ('biodegradation_half_time_droplet', biodegradation_half_time_droplet),
                        ('biodegradation_half_time_slick', biodegradation_half_time_slick)):
            rec[:, _abi.WEATHER_RECORD.index(name)] = v
        rows = np.ascontiguousarray(np.asarray(mass_fraction, np.float64) * (mass_oil.reshape((n, -1))))      # (:689-691)
        if rows.shape != (n, self._weather_ncomp):
            raise ValueError('mass_fraction of %d components for a table of %d' % (rows.shape[1], self._weather_ncomp))
        check(self.lib.odr_oil_weathering_seed(self.ctx.h, self.h, int(id0), n, rec.ctypes.data_as(_dp), rows.ctypes.data_as(_dp)))

    def oil_weather(self, dt, processes=('properties', 'evaporation', 'emulsification', 'dispersion')):
        """OpenOil.oil_weathering_noaa over the active set (openoil.py:717-790; odr_oil_weather): processes by name, 'half_time' /
        'Adcroft' for biodegradation.  Density and viscosity of the emulsion go to the oil's property slots as float32."""
        flags = 0
        for k in processes:
            flags |= _abi.WEATHER[k]
        check(self.lib.odr_oil_weather(self.ctx.h, self.h, float(dt), flags))

    def weathering_get(self, name):
        """One variable of the weathering table BY ELEMENT ID (odr_oil_weathering_get): [n_total], 'mass_components' [n_total, ncomp],
        'reduction' {name: value} of the last oil_weather call."""
        n = 8 if name == 'reduction' else self._weather_n_total * (self._weather_ncomp if name == 'mass_components' else 1)
        out = np.empty(n)
        check(self.lib.odr_oil_weathering_get(self.ctx.h, self.h, name.encode(), out.ctypes.data_as(_dp)))
        if name == 'reduction':
            return dict(zip(_abi.WEATHER_REDUCTION, out))
        return out.reshape(self._weather_n_total, -1) if name == 'mass_components' else out

    def weathering_set(self, name, values):
        a = np.ascontiguousarray(values, dtype=np.float64)
        if a.size != self._weather_n_total * (self._weather_ncomp if name == 'mass_components' else 1):
            raise ValueError('%s: %d values for a table of %d elements' % (name, a.size, self._weather_n_total))
        check(self.lib.odr_oil_weathering_set(self.ctx.h, self.h, name.encode(), a.ctypes.data_as(_dp)))

    def oil_budget(self, stranded_code):
        """get_oil_budget's sums now (openoil.py:1241-1306; odr_oil_budget): {mass_surface, ..., mass_total}, active and deactivated
        elements counted, and 'n', how many."""
        out = np.empty(8)
        check(self.lib.odr_oil_budget(self.ctx.h, self.h, int(stranded_code), out.ctypes.data_as(_dp)))
        b = dict(zip(_abi.OIL_BUDGET, out[:7]))
        b['n'] = int(out[7])
        return b

    def vertical_advection(self, dt, at_surface=False):
        check(self.lib.odr_vertical_advection(self.ctx.h, self.h, float(dt), int(at_surface)))

    def vertical_buoyancy(self, dt):
        check(self.lib.odr_vertical_buoyancy(self.ctx.h, self.h, float(dt)))

    def store_previous(self):
        check(self.lib.odr_store_previous(self.ctx.h, self.h))

    def coastline(self, action, stranded_code=1, seeded_on_land_code=0):
        a = action if isinstance(action, int) else _abi.COAST[action]
        n = C.c_int64()
        check(self.lib.odr_coastline(self.ctx.h, self.h, a, stranded_code, seeded_on_land_code, C.byref(n)))
        return n.value

    def coastline_crossing(self, action, precision, landmask_source, stranded_code=1, seeded_on_land_code=0):
        """interact_with_coastline with general:coastline_approximation_precision (basemodel/__init__.py:694-746)."""
        a = action if isinstance(action, int) else _abi.COAST[action]
        n = C.c_int64()
        check(self.lib.odr_coastline_crossing(self.ctx.h, self.h, a, stranded_code, seeded_on_land_code, float(precision),
                                              int(landmask_source), C.byref(n)))
        return n.value

    def increase_age(self, dt, max_age_seconds=0.0, retired_code=0):
        check(self.lib.odr_increase_age(self.ctx.h, self.h, float(dt), float(max_age_seconds), retired_code))

    def deactivate_missing(self, variables, status_code):
        """report_missing_variables (basemodel/__init__.py:2501-2515) on the last environment sample."""
        ids, pi = _i([self.ctx._vid(v) for v in variables])
        n = C.c_int64()
        check(self.lib.odr_deactivate_missing(self.ctx.h, self.h, len(ids), pi, int(status_code), C.byref(n)))
        return n.value

    def count_status(self, status_code):
        n = C.c_int64()
        check(self.lib.odr_particles_count_status(self.ctx.h, self.h, int(status_code), C.byref(n)))
        return n.value

    def remap_status(self, from_code, to_code):
        check(self.lib.odr_particles_remap_status(self.ctx.h, self.h, int(from_code), int(to_code)))

    def seafloor(self, action='lift_to_seafloor', status_code=0):
        """interact_with_seafloor (basemodel/__init__.py:748-783): 'lift_to_seafloor' | 'deactivate' | 'previous'."""
        n = C.c_int64()
        a = {'lift_to_seafloor': 1, 'deactivate': 2, 'previous': 3}[action]
        check(self.lib.odr_seafloor_action(self.ctx.h, self.h, a, int(status_code), C.byref(n)))
        return n.value

    def deactivate(self, mask, status_code):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        check(self.lib.odr_deactivate(self.ctx.h, self.h, m.ctypes.data_as(C.POINTER(C.c_uint8)), status_code))

    def deactivate_outside(self, west, east, south, north, status_code):
        f = lambda v: np.nan if v is None else float(v)
        check(self.lib.odr_deactivate_outside(self.ctx.h, self.h, f(west), f(east), f(south), f(north), int(status_code)))

    def compact(self):
        """Remove the deactivated elements (remove_deactivated_elements).  In place: the survivors are
        permuted (holes filled from the tail); elements are identified by their ID."""
        n0 = len(self)
        n = C.c_int64()
        check(self.lib.odr_compact(self.ctx.h, self.h, C.byref(n)))
        if n.value != n0:
            self._permuted = True
        return n.value

    def scan_status(self):
        """(elements that stay, provisional status numbers present as a bit mask: bit k <-> status 100 + k) in one host
        read (odr_scan_status); follow with compact_apply()."""
        n, f = C.c_int64(), C.c_uint64()
        check(self.lib.odr_scan_status(self.ctx.h, self.h, C.byref(n), C.byref(f)))
        return n.value, f.value

    def scan_status_begin(self):
        """First half of scan_status (odr_scan_status_begin): the fold of the counts the step launch left is enqueued; False
        when that launch left none (then call scan_status())."""
        rc = self.lib.odr_scan_status_begin(self.ctx.h, self.h)
        if rc < 0:
            check(rc)
        return rc == 0

    def scan_status_end(self):
        """Second half: waits for the fold only (not for a guarded mixing launch enqueued behind it)."""
        n, f = C.c_int64(), C.c_uint64()
        check(self.lib.odr_scan_status_end(self.ctx.h, self.h, C.byref(n), C.byref(f)))
        return n.value, f.value

    def compact_apply(self):
        n0 = len(self)
        n = C.c_int64()
        check(self.lib.odr_compact_apply(self.ctx.h, self.h, C.byref(n)))
        if n.value != n0:
            self._permuted = True
        return n.value

    def sort_by_cell(self, source_id, keep_environment=True):
        """Re-order the SoA by grid cell of a gridded source (layout only; IDs are preserved).  keep_environment=False:
        the sampled environment is not carried along (a re-sort right before the next sample)."""
        check(self.lib.odr_sort_particles_ex(self.ctx.h, self.h, int(source_id), int(bool(keep_environment))))
        self._permuted = True

    def truncate_z(self, depth):
        """The sampling calls that follow see max(z, -depth) (drift:truncate_ocean_model_below_m); restore_z() ends it."""
        check(self.lib.odr_particles_truncate_z(self.ctx.h, self.h, float(depth)))

    def restore_z(self):
        check(self.lib.odr_particles_restore_z(self.ctx.h, self.h))

    def _counters(self, symbol, keys):
        """One uint64 per key from a diagnostics entry point (ctx, particles, uint64 *out)."""
        out = (C.c_uint64 * len(keys))()
        check(getattr(self.lib, symbol)(self.ctx.h, self.h, out))
        return dict(zip(keys, map(int, out)))

    def tile_stats(self):
        """Diagnostics of the LDS-tile step (odr_particles_tile_stats): launches on that path, elements they handed to the
        HBM path, rectangles cut to the LDS capacity, workgroup ranges of the current table."""
        return self._counters('odr_particles_tile_stats', ('launches', 'handed_over', 'rectangles_cut', 'ranges'))

    def step_layout_stats(self):
        """Launches of the fused step kernel (odr_particles_step_layout_stats): `static` with the C3 group's compile-time
        layout between two time levels, `runtime` all others (the run-time slot layout, and the on-level static layout
        that step_onlevel_stats counts on its own)."""
        return self._counters('odr_particles_step_layout_stats', ('runtime', 'static'))

    def step_onlevel_stats(self):
        """Launches of the fused step kernel with the C3 group's compile-time layout on a step whose time sits on a reader
        level (odr_particles_step_onlevel_stats)."""
        return self._counters('odr_particles_step_onlevel_stats', ('launches',))['launches']

    def vmix_layout_stats(self):
        """Launches of the mixing kernels (odr_particles_vmix_layout_stats): the K-column kernel with the run-time configuration,
        with C3's compile-time one, and the other mixing kernels."""
        return self._counters('odr_particles_vmix_layout_stats', ('runtime', 'static', 'other'))

    def vmix_kplane_stats(self):
        """Where the K-column / window mixing launches gathered the diffusivity from (odr_particles_vmix_kplane_stats): the
        levels' K planes, or the node records."""
        return self._counters('odr_particles_vmix_kplane_stats', ('planes', 'records'))

    def vmix_window_stats(self):
        """The static 12-level K-column launches (odr_particles_vmix_window_stats): those that gathered two K quads per
        particle, those that gathered the whole column, and the elements the two-quad launches redid on the whole column."""
        return self._counters('odr_particles_vmix_window_stats', ('windowed', 'full', 'redone'))

    def vmix_skip_stats(self):
        """The tiled K-column launches (odr_particles_vmix_skip_stats) and the elements they skipped at the surface: z == 0
        on entry with no mixing and no vertical advection at the surface, for which the launch stores z = +0.0 anyway."""
        return self._counters('odr_particles_vmix_skip_stats', ('launches', 'skipped'))

    def vmix_dense_stats(self):
        """The dense mixing launches (odr_particles_vmix_dense_stats: the compaction over the whole launch, static
        configurations whose settings allow the skip) and the elements their lists held."""
        return self._counters('odr_particles_vmix_dense_stats', ('launches', 'listed'))

    def vmix_keep_stats(self):
        """Where the dense mixing launches took their keep ballots from (odr_particles_vmix_keep_stats): the step launch that
        ran right before, or k_vmix_keep's own pass; and the lists that held every element (not filled)."""
        return self._counters('odr_particles_vmix_keep_stats', ('from_step', 'from_keep', 'identity'))

    def reduce_global(self, combine, wind_drift_depth=0.1, relative_wind=False):
        """Sharded run: this set's raw reductions -> combine(raw16) over the ranks (counts summed, maxima maximised) ->
        installed for the movers that follow, until reduce_unpin()."""
        raw = np.empty(16)
        check(self.lib.odr_reduce_local(self.ctx.h, self.h, float(wind_drift_depth), int(relative_wind), raw.ctypes.data_as(_dp)))
        g = np.ascontiguousarray(combine(raw), dtype=np.float64)
        check(self.lib.odr_reduce_install(self.ctx.h, self.h, g.ctypes.data_as(_dp)))
        return g

    def reduce_local(self, wind_drift_depth=0.1, relative_wind=False):
        """The 16 raw reduction slots of THIS rank's active elements (status 0; odr_reduce_local): slots 0 and 11 are
        counts, the others maxima (minima negated).  Combined over the ranks by the caller, then reduce_install()."""
        raw = np.empty(16)
        check(self.lib.odr_reduce_local(self.ctx.h, self.h, float(wind_drift_depth), int(relative_wind), raw.ctypes.data_as(_dp)))
        return raw

    def reduce_install(self, combined16):
        g = np.ascontiguousarray(combined16, dtype=np.float64)
        check(self.lib.odr_reduce_install(self.ctx.h, self.h, g.ctypes.data_as(_dp)))

    @staticmethod
    def reduction_dict(raw):
        d = dict(zip(REDUCTION_KEYS, raw))
        for k in ('lon_min', 'lat_min', 'z_min'):
            d[k] = -d[k]
        return d

    def reduce_unpin(self):
        check(self.lib.odr_reduce_unpin(self.ctx.h))

    def reduce_cached(self):
        """(raw16, state) as they stand on the device -- what the last mover read; nothing is reduced (odr_reduce_cached).
        state: dict(valid: a mover on this set would reuse them, extents: slots 1..6 are filled, partial: formed by the step
        launch (signs, not maxima), pinned: installed by reduce_install)."""
        raw, st = np.empty(16), C.c_int32()
        check(self.lib.odr_reduce_cached(self.ctx.h, self.h, raw.ctypes.data_as(_dp), C.byref(st)))
        return raw, dict(valid=bool(st.value & 1), extents=bool(st.value & 2), partial=bool(st.value & 4), pinned=bool(st.value & 8))

    def reduce_scalars(self, wind_drift_depth=0.1):
        out = np.empty(16)
        check(self.lib.odr_reduce_scalars(self.ctx.h, self.h, float(wind_drift_depth), out.ctypes.data_as(_dp)))
        return dict(zip(REDUCTION_KEYS, out))


_SLOW_MS = float(os.environ.get('ODR_SLOW_CALLS', 0) or 0)


def _touching(fn):
    """A call that changes the device state: what a model wrote into its `o.elements` view goes to the device first
    (oceandrift.ElementsView.flush), and views taken before the call become stale."""
    def wrapper(self, *a, **kw):
        v = self.__dict__.get('_view')
        if v is not None:
            self._view = None
            v.flush()
        self._touch = self.__dict__.get('_touch', 0) + 1
        if _SLOW_MS:     # ODR_SLOW_CALLS=<ms>: calls that keep the host longer than that (stderr)
            import sys
            import time
            t0 = time.perf_counter()
            r = fn(self, *a, **kw)
            ms = 1e3 * (time.perf_counter() - t0)
            if ms > _SLOW_MS:
                print('%s: %.3f ms' % (fn.__name__, ms), file=sys.stderr)
            return r
        return fn(self, *a, **kw)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


for _name in ('append', 'upload', 'env_sample', 'umesh_sample', 'schism_sample', 'shape_sample', 'combined_sample', 'env_upload', 'env_add_noise', 'advect', 'env_coast_advect',
              'update_positions', 'advect_wind', 'stokes_drift', 'advect_sea_ice', 'set_property', 'leeway_capsize', 'leeway', 'hdiffusion', 'movers',
              'vmix', 'vmix_analytic', 'vmix_oil', 'vertical_advection', 'vertical_buoyancy', 'coastline', 'coastline_crossing',
              'increase_age', 'deactivate_missing', 'remap_status', 'seafloor', 'deactivate', 'deactivate_outside', 'compact',
              'compact_apply', 'sort_by_cell', 'store_previous', 'oil_prepare_mixing', 'env_coast_leeway', 'egg_terminal_velocity',
              'resuspend', 'larval_update', 'larval_migrate', 'larvalx_hatch', 'larvalx_behave', 'berg_roll_over', 'berg_advect', 'ship_drift', 'radio_speciation',
              'radio_terminal_velocity', 'radio_resuspend', 'oil_weather'):
    setattr(Particles, _name, _touching(getattr(Particles, _name)))


def _reading(fn):
    """A call that only READS the device state (downloads, reductions, scans): pending writes of the `o.elements` view
    reach the device first -- `self.elements.z = ...` inside update() must be seen by the reductions of stokes_drift and
    by the stored previous positions -- but the view stays valid (nothing changed underneath it)."""
    def wrapper(self, *a, **kw):
        v = self.__dict__.get('_view')
        if v is not None and not getattr(v, '_flushing', False):
            touch = self.__dict__.get('_touch', 0)
            v.flush()                    # uploads what differs (a _touching call) ...
            self._touch = touch          # ... which does not make the view stale: it holds what it just wrote
            self._view = v
        return fn(self, *a, **kw)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


for _name in ('download', 'download_f32', 'env_download', 'get_property', 'reduce_scalars', 'reduce_global', 'reduce_local', 'oil_global_stats',
              'scan_status', 'count_status', 'solar_elevation'):
    setattr(Particles, _name, _reading(getattr(Particles, _name)))


class _Handle:
    """A device object of a context behind `ptr`, released by the library's DESTROY(ctx, ptr) -- by close(), or with the last
    reference as long as the context is still open."""
    DESTROY = None

    def close(self):
        if self.ptr and self.ctx.h:
            getattr(self.ctx.lib, self.DESTROY)(self.ctx.h, self.ptr)
        self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShipTable(_Handle):
    """Device copy of ShipDrift's class tables (odr_ship_table_create / _destroy)."""
    DESTROY = 'odr_ship_table_destroy'

    def __init__(self, ctx, table):
        t = np.ascontiguousarray(table, dtype=np.float64)
        if t.ndim != 3 or t.shape[1:] != (_abi.SHIP_TABLE_ROWS, 2) or t.shape[0] < 1:
            raise ValueError('ship class table of shape %s, expected (n_classes, %d, 2)' % (t.shape, _abi.SHIP_TABLE_ROWS))
        self.ctx, self.ptr = ctx, C.c_void_p()
        check(ctx.lib.odr_ship_table_create(ctx.h, t.ctypes.data_as(_dp), t.shape[0], C.byref(self.ptr)))
        n = C.c_int32()
        check(ctx.lib.odr_ship_table_classes(self.ptr, C.byref(n)))
        self.n_classes = n.value      # (the library keeps the count with the table)



class UMesh(_Handle):
    """Device image of a triangular mesh (odr_umesh_create / _destroy): the search indices over the nodes and the face centres,
    the box of the nodes, the sigma and depth arrays, and up to three resident time levels."""
    DESTROY = 'odr_umesh_destroy'
    SIGMA = ('siglay', 'siglev', 'siglay_center', 'siglev_center', 'h', 'h_center')

    def __init__(self, ctx, x, y, xc=None, yc=None, proj=None, **sigma):
        unknown = set(sigma) - set(self.SIGMA)
        if unknown:
            raise TypeError('unknown mesh arrays %s' % sorted(unknown))
        (x, px), (y, py) = _d(np.ravel(x)), _d(np.ravel(y))
        (xc, pxc), (yc, pyc) = _d(np.ravel([] if xc is None else xc)), _d(np.ravel([] if yc is None else yc))
        if len(x) != len(y) or len(xc) != len(yc):
            raise ValueError('%d x and %d y node coordinates, %d xc and %d yc face centres' % (len(x), len(y), len(xc), len(yc)))
        self.n_nodes, self.n_faces = len(x), len(xc)
        a = {k: (None if sigma.get(k) is None else np.ascontiguousarray(sigma[k], dtype=np.float32)) for k in self.SIGMA}
        lays = [a[k].shape[0] for k in ('siglay', 'siglay_center') if a[k] is not None and a[k].ndim == 2]
        levs = [a[k].shape[0] - 1 for k in ('siglev', 'siglev_center') if a[k] is not None and a[k].ndim == 2]
        if len(set(lays + levs)) > 1:
            raise ValueError('the sigma arrays disagree on the number of layers: %s layers, %s levels' % (lays, [k + 1 for k in levs]))
        self.n_siglay = (lays + levs + [0])[0]
        for k in self.SIGMA:      # the library reads whole arrays: their lengths are checked here
            npts = self.n_faces if k.endswith('center') else self.n_nodes
            rows = () if k.startswith('h') else ((self.n_siglay + (1 if 'siglev' in k else 0)),)
            if a[k] is not None and a[k].shape != rows + (npts,):
                raise ValueError('%s of shape %s, expected %s' % (k, a[k].shape, rows + (npts,)))
        pd = proj_desc(proj)
        self.ctx, self.ptr = ctx, C.c_void_p()
        check(ctx.lib.odr_umesh_create(ctx.h, None if pd is None else C.byref(pd), self.n_nodes, px, py, self.n_faces,
                                       pxc if self.n_faces else None, pyc if self.n_faces else None, self.n_siglay,
                                       *[None if a[k] is None else a[k].ctypes.data_as(_fp) for k in self.SIGMA], C.byref(self.ptr)))

    def set_level(self, slot, t_epoch, variable, data, on_faces):
        """One variable of one time level becomes resident in `slot`: data [points] or [levels, points] float32."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        npts = self.n_faces if on_faces else self.n_nodes
        if data.ndim not in (1, 2) or data.shape[-1] != npts:
            raise ValueError('%s of shape %s on a mesh of %d %s' % (variable, data.shape, npts, 'faces' if on_faces else 'nodes'))
        check(self.ctx.lib.odr_umesh_set_level(self.ctx.h, self.ptr, int(slot), float(t_epoch), self.ctx._vid(variable), int(bool(on_faces)),
                                               data.shape[0] if data.ndim == 2 else 0, data.ctypes.data_as(_fp)))

    def nearest(self, x, y, on_faces=False):
        """Index of the node (or face centre) nearest to each (x, y) in mesh coordinates (odr_umesh_nearest): int32, -1 for a
        point that is not finite."""
        (x, px), (y, py) = _d(np.ravel(x)), _d(np.ravel(y))
        if len(x) != len(y):
            raise ValueError('%d x and %d y' % (len(x), len(y)))
        out = np.empty(len(x), np.int32)
        check(self.ctx.lib.odr_umesh_nearest(self.ctx.h, self.ptr, int(bool(on_faces)), len(x), px, py, out.ctypes.data_as(_ip)))
        return out



class SchismMesh(_Handle):
    """Device image of a SCHISM-style mesh (odr_schism_create / _destroy): the search index over the nodes, the grid over the
    ring of their convex hull, and up to four resident time levels -- zcor [nodes, levels] and the variables' planes."""
    DESTROY = 'odr_schism_destroy'

    def __init__(self, ctx, x, y, hull_x, hull_y, n_levels=0, proj=None):
        (x, px), (y, py) = _d(np.ravel(x)), _d(np.ravel(y))
        (hx, phx), (hy, phy) = _d(np.ravel(hull_x)), _d(np.ravel(hull_y))
        if len(x) != len(y) or len(hx) != len(hy):
            raise ValueError('%d x and %d y node coordinates, %d x and %d y hull vertices' % (len(x), len(y), len(hx), len(hy)))
        self.n_nodes, self.n_levels = len(x), int(n_levels)
        pd = proj_desc(proj)
        self.ctx, self.ptr = ctx, C.c_void_p()
        check(ctx.lib.odr_schism_create(ctx.h, None if pd is None else C.byref(pd), self.n_nodes, px, py, self.n_levels, len(hx), phx, phy,
                                        C.byref(self.ptr)))

    def set_zcor(self, slot, t_epoch, zcor):
        """The vertical coordinate of the time level in `slot`: [nodes, levels] float32, NaN below the sea bed."""
        zcor = np.ascontiguousarray(zcor, dtype=np.float32)
        if zcor.shape != (self.n_nodes, self.n_levels) or not self.n_levels:      # the library reads the whole array
            raise ValueError('zcor of shape %s on a mesh of %d nodes and %d levels' % (zcor.shape, self.n_nodes, self.n_levels))
        check(self.ctx.lib.odr_schism_set_zcor(self.ctx.h, self.ptr, int(slot), float(t_epoch), zcor.ctypes.data_as(_fp)))

    def set_level(self, slot, t_epoch, variable, data):
        """One variable of one time level becomes resident in `slot`: data [nodes] or [nodes, levels] float32."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.shape not in ((self.n_nodes,), (self.n_nodes, self.n_levels)):
            raise ValueError('%s of shape %s on a mesh of %d nodes and %d levels' % (variable, data.shape, self.n_nodes, self.n_levels))
        check(self.ctx.lib.odr_schism_set_level(self.ctx.h, self.ptr, int(slot), float(t_epoch), self.ctx._vid(variable),
                                                data.shape[1] if data.ndim == 2 else 0, data.ctypes.data_as(_fp)))

    def nearest3(self, x, y, z=None, slot=0, visits=False):
        """(idx [n, 3] int64, dist [n, 3]) of the three nearest points of each (x, y) among the nodes, or of each (x, y, z) among
        node x level at the zcor of `slot`, ascending (odr_schism_nearest3); -1 / inf for a point that is not finite.
        visits=True: also the tree nodes each query formed a distance to."""
        (x, px), (y, py) = _d(np.ravel(x)), _d(np.ravel(y))
        if len(x) != len(y):
            raise ValueError('%d x and %d y' % (len(x), len(y)))
        pz = None
        if z is not None:
            z, pz = _d(np.ravel(z))
            if len(z) != len(x):
                raise ValueError('%d x and %d z' % (len(x), len(z)))
        idx, dist, seen = np.empty((len(x), 3), np.int64), np.empty((len(x), 3)), np.empty(len(x), np.int32)
        check(self.ctx.lib.odr_schism_nearest3(self.ctx.h, self.ptr, int(slot), len(x), px, py, pz, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                               dist.ctypes.data_as(_dp), seen.ctypes.data_as(_ip) if visits else None))
        return (idx, dist, seen) if visits else (idx, dist)



class Shape(_Handle):
    """Device image of coastline polygons (odr_shape_create / _destroy): the uniform grid over the box of the rings and the
    per-cell lists of edges and corner toggles."""
    DESTROY = 'odr_shape_destroy'
    STATS = ('cells', 'entries', 'longest_list', 'mean_list', 'nudges', 'bytes', 'nx', 'ny')

    def __init__(self, ctx, x1, y1, x2, y2, poly, n_polygons, proj=None, invert=False, nx=0, ny=0):
        (x1, p1), (y1, q1), (x2, p2), (y2, q2) = (_d(np.ravel(a)) for a in (x1, y1, x2, y2))
        poly, pp = _i(np.ravel(poly))
        if not (len(x1) == len(y1) == len(x2) == len(y2) == len(poly)):
            raise ValueError('edge arrays of %d, %d, %d, %d and %d elements' % (len(x1), len(y1), len(x2), len(y2), len(poly)))
        self.n_edges, self.n_polygons = len(x1), int(n_polygons)
        pd = proj_desc(proj)
        self.ctx, self.ptr = ctx, C.c_void_p()
        check(ctx.lib.odr_shape_create(ctx.h, None if pd is None else C.byref(pd), self.n_edges, p1, q1, p2, q2, pp, self.n_polygons,
                                       int(nx), int(ny), int(bool(invert)), C.byref(self.ptr)))

    def contains(self, x, y):
        """land_binary_mask at (x, y) in the polygons' coordinates (odr_shape_contains): float32 1 / 0, NaN outside the box."""
        (x, px), (y, py) = _d(np.ravel(x)), _d(np.ravel(y))
        if len(x) != len(y):
            raise ValueError('%d x and %d y' % (len(x), len(y)))
        out = np.empty(len(x), np.float32)
        check(self.ctx.lib.odr_shape_contains(self.ctx.h, self.ptr, len(x), px, py, out.ctypes.data_as(_fp)))
        return out

    def stats(self):
        a = np.zeros(len(self.STATS))
        check(self.ctx.lib.odr_shape_stats(self.ctx.h, self.ptr, a.ctypes.data_as(_dp)))
        return dict(zip(self.STATS, a.tolist()))



class Combined(_Handle):
    """The flattened program of a reader expression (odr_combined_create / _destroy; csrc/odr_combine.hip.h)."""
    DESTROY = 'odr_combined_destroy'

    def __init__(self, ctx, ops):
        ops = list(ops)
        arr = (_abi.CombineOp * max(len(ops), 1))()
        for k, (kind, index, d) in enumerate(ops):
            arr[k].kind, arr[k].index = int(kind), int(index)
            for j, v in enumerate(tuple(d)[:3]):
                arr[k].d[j] = float(v)
        self.n_ops = len(ops)
        self.ctx, self.ptr = ctx, C.c_void_p()
        check(ctx.lib.odr_combined_create(ctx.h, len(ops), arr, C.byref(self.ptr)))



def weathering_table(oil, sea_water_density):
    """odr_oil_table of an oil given as a dict (OpenOil.set_oiltype): the per-component constants of OpendriftOil.vapor_pressure
    (adios/oil.py:155-166) and of evap_decay_constant (noaa_oil_weathering.py:26) formed here with the reference's NumPy
    expressions, the two property curves, the emulsification constants."""
    boiling_point = np.asarray(oil['boiling_point'], dtype=np.float64)
    n = boiling_point.size
    if not 1 <= n <= _abi.OIL_MAXCOMP:
        raise ValueError('an oil of %d pseudo-components: the device table holds 1 .. %d (ODR_OIL_MAXCOMP)' % (n, _abi.OIL_MAXCOMP))
    D_Zb = 0.97
    R_cal = 1.987
    D_S = 8.75 + 1.987 * np.log(boiling_point)
    C_2i = 0.19 * boiling_point - 18
    t = _abi.OilTable()
    comp = np.zeros((4, _abi.OIL_MAXCOMP))
    comp[0, :n] = D_S * (boiling_point - C_2i)**2 / (D_Zb * R_cal * boiling_point)
    comp[1, :n] = C_2i
    comp[2, :n] = 1. / (boiling_point - C_2i)
    comp[3, :n] = np.asarray(oil['molecular_weight'], dtype=np.float64) / 1000.
    comp[3, n:] = 1.0
    t.ncomp = n
    t.comp[:] = comp.ravel().tolist()
    defaults = {'density_ref_temp': 288.15, 'density_k': 0.0, 'viscosity_ref_temp': 288.15, 'viscosity_B': 0.0}      # the curves are constants
    for k in ('density', 'density_ref_temp', 'density_k', 'viscosity', 'viscosity_ref_temp', 'viscosity_B'):
        setattr(t, k, float(oil[k] if k in oil else defaults[k]))
    bt = oil.get('bullwinkle_time')
    t.bulltime = -999. if bt is None or bt != bt else float(bt)        # adios/oil.py:125-130
    t.bullwinkle = float(oil['bullwinkle_fraction'])
    t.y_max = float(oil['emulsion_water_fraction_max'])
    mwf = oil.get('max_water_fraction')
    t.mwf_n = 0
    if mwf is not None:
        T, w = list(mwf['temperatures']), list(mwf['max_water_fraction'])
        if len(T) != len(w) or len(T) not in (1, 2):
            raise ValueError('max_water_fraction takes one or two temperatures with as many fractions')
        t.mwf_n = len(T)
        for k in range(len(T)):
            t.mwf_t[k], t.mwf_w[k] = float(T[k]), float(w[k])
    t.sea_water_density = float(sea_water_density)
    return t


class RadioSetup(_Handle):
    """Device copy of RadionuclideDrift's species setup with the counters ntransformations (odr_radio_create / _destroy)."""
    DESTROY = 'odr_radio_destroy'
    SPECIES = ('lmm', 'lmmcation', 'lmmanion', 'polymer', 'particle_rev', 'sediment_rev', 'particle_slow', 'sediment_slow',
               'particle_irrev', 'sediment_irrev')

    def __init__(self, ctx, rates, nspecies, lognormal=False, **members):
        r = np.asarray(rates, dtype=np.float64)
        r = r[None] if r.ndim == 2 else r
        M, A = _abi.RADIO_MAX_SPECIES, _abi.RADIO_MAX_SALINITY_INTERVALS
        if r.ndim != 3 or r.shape[0] not in (1, A) or r.shape[1:] != (nspecies, nspecies) or not 1 <= nspecies <= M:
            raise ValueError('transfer rates of shape %s for %s species (at most %d, 1 or %d salinity intervals)' % (r.shape, nspecies, M, A))
        st = _abi.RadioSetup()
        st.nspecies, st.nsalinity, st.lognormal = int(nspecies), r.shape[0], int(bool(lognormal))
        full = np.zeros((A, M, M))
        full[:r.shape[0], :nspecies, :nspecies] = r
        st.rates[:] = full.ravel().tolist()
        for k in self.SPECIES:
            setattr(st, k, int(members.pop(k, -1)))
        for k, _ in _abi.RadioSetup._fields_[-9:]:
            setattr(st, k, float(members.pop(k)))
        if members:
            raise TypeError('unknown members of the setup: %s' % sorted(members))
        self.ctx, self.ptr, self.nspecies, self.struct = ctx, C.c_void_p(), int(nspecies), st
        check(ctx.lib.odr_radio_create(ctx.h, C.byref(st), C.byref(self.ptr)))

    def counts(self, reset=False):
        """ntransformations[in][out] since creation (or the last reset); the host waits for the context's stream.  OdrError when a
        launch met an element whose species number is outside the table."""
        c = np.zeros(_abi.RADIO_MAX_SPECIES ** 2, np.int64)
        check(self.ctx.lib.odr_radio_counts(self.ctx.h, self.ptr, c.ctypes.data_as(C.POINTER(C.c_int64)), int(bool(reset))))
        return c.reshape(_abi.RADIO_MAX_SPECIES, _abi.RADIO_MAX_SPECIES)[:self.nspecies, :self.nspecies].copy()



class History:
    """Device-resident float32 result buffer (state_to_buffer, basemodel/__init__.py:2084-2105,2384-2499):
    `variables` = element property names ('lon', 'lat', 'z', 'status', ...), environment variable names, or
    ('property', slot).  record() scatters the current state at (ID, time index); flush() copies time slots to
    pinned host memory asynchronously; array(var) returns the [trajectory, time] float32 view of the last flush."""

    def __init__(self, ctx, n_trajectories, n_times, variables, id_base=0):
        self.ctx, self.lib = ctx, ctx.lib
        self.variables = list(variables)
        self._id_base = int(id_base)
        self.n_trajectories, self.n_times = int(n_trajectories), int(n_times)
        codes = []
        for v in self.variables:
            if isinstance(v, tuple):
                codes.append(_abi.HIST_PROPERTY0 + int(v[1]))
            elif v in _abi.HIST:
                codes.append(_abi.HIST[v])
            else:
                codes.append(ctx._vid(v))
        a, pa = _i(codes)
        self.h = C.c_void_p()
        check(self.lib.odr_history_create(ctx.h, self.n_trajectories, self.n_times, len(codes), pa, C.byref(self.h)))
        if self._id_base:
            check(self.lib.odr_history_set_id_base(ctx.h, self.h, self._id_base))

    def record(self, particles, time_index, only_deactivated=False, position_from_previous=False):
        check(self.lib.odr_history_record(self.ctx.h, particles.h, self.h, int(time_index), int(bool(only_deactivated)),
                                          int(position_from_previous)))      # bit 0: previous position, bit 1: snapshot properties

    def flush(self, t0=0, nt=None):
        check(self.lib.odr_history_flush(self.ctx.h, self.h, int(t0), int(self.n_times - t0 if nt is None else nt)))

    def wait(self):
        check(self.lib.odr_history_wait(self.ctx.h, self.h))

    def array(self, variable):
        """[trajectory, time] float32 view of pinned host memory (valid until the next flush)."""
        k = self.variables.index(variable)
        p, nt = _fp(), C.c_int32()
        check(self.lib.odr_history_host_ptr(self.ctx.h, self.h, k, C.byref(p), C.byref(nt)))
        return np.ctypeslib.as_array(p, shape=(self.n_trajectories, nt.value))

    def minmax(self, variable):
        lo, hi = C.c_double(), C.c_double()
        check(self.lib.odr_history_minmax(self.ctx.h, self.h, self.variables.index(variable), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def reset(self):
        check(self.lib.odr_history_reset(self.ctx.h, self.h))

    def close(self):
        if self.h:
            self.lib.odr_history_destroy(self.ctx.h, self.h)
            self.h = None


class SigmaGrid:
    """ROMS s-coordinate grid on the device (odr_sgrid_*): depths of the rho s-levels (roppy sdepth) and the
    sigma -> z regridding of 3-D variables (roppy multi_zslice) as done by reader_ROMS_native.get_variables."""

    def __init__(self, ctx, H, Hc, Cs_r, zeta=None, S=None, Vtransform=1):
        self.ctx, self.lib = ctx, ctx.lib
        H = np.ascontiguousarray(H, dtype=np.float64)
        self.ny, self.nx = H.shape
        Cs = np.ascontiguousarray(Cs_r, dtype=np.float64)
        self.N = len(Cs)
        ze = None if zeta is None else np.ascontiguousarray(zeta, dtype=np.float64)
        Sa = None if S is None else np.ascontiguousarray(S, dtype=np.float64)
        self.h = C.c_void_p()
        check(self.lib.odr_sgrid_create(ctx.h, self.ny, self.nx, self.N, H.ctypes.data_as(_dp),
                                        None if ze is None else ze.ctypes.data_as(_dp), float(Hc), Cs.ctypes.data_as(_dp),
                                        None if Sa is None else Sa.ctypes.data_as(_dp), int(Vtransform), C.byref(self.h)))

    def z_rho(self):
        out = np.empty((self.N, self.ny, self.nx))
        check(self.lib.odr_sgrid_download_zrho(self.ctx.h, self.h, out.ctypes.data_as(_dp)))
        return out

    def zslice(self, field, Z, want_float64=False, slot=0):
        """field [N, ny, nx] (float32 / float64 host array, or an int device pointer to float32) -> device pointer
        of the float32 [len(Z), ny, nx] result in result slot `slot` (0..7: one per variable of a block, for
        Context.upload_block_device) and, if asked, the float64 values."""
        Z = np.ascontiguousarray(np.atleast_1d(Z), dtype=np.float64)
        out64 = np.empty((len(Z), self.ny, self.nx)) if want_float64 else None
        dev = C.c_void_p()
        if isinstance(field, (int, np.integer)):
            check(self.lib.odr_sgrid_zslice(self.ctx.h, self.h, C.c_void_p(int(field)), 0, 1, len(Z), Z.ctypes.data_as(_dp),
                                            int(slot), C.byref(dev), None if out64 is None else out64.ctypes.data_as(_dp)))
        else:
            f = np.ascontiguousarray(field)
            if f.dtype not in (np.float32, np.float64):
                f = f.astype(np.float64)
            assert f.shape == (self.N, self.ny, self.nx), (f.shape, (self.N, self.ny, self.nx))
            check(self.lib.odr_sgrid_zslice(self.ctx.h, self.h, f.ctypes.data_as(C.c_void_p), int(f.dtype == np.float64), 0,
                                            len(Z), Z.ctypes.data_as(_dp), int(slot), C.byref(dev),
                                            None if out64 is None else out64.ctypes.data_as(_dp)))
        return (dev.value, out64) if want_float64 else dev.value

    def close(self):
        if self.h:
            self.lib.odr_sgrid_destroy(self.ctx.h, self.h)
            self.h = None
