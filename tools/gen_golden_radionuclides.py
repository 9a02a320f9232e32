"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/c30_radionuclides.npz from the REFERENCE ITSELF.

The reference's own RadionuclideDrift (opendrift/models/radionuclides.py) runs through oracle/refshim.py + oracle/refdriver.py
on a small lon/lat grid with fields that are constant in time: depth 20 - 40 m, conc3 0.5e-3 - 3.5e-3 kg/m3, a current below
radionuclide:sediment:resuspension_critvel in one patch and above it elsewhere, horizontal_diffusivity 0.  Two cases:

  (a) 'LMM + Rev + Slow rev + Irrev', isotope 241Am, slow_coeff 2e-5, particle_diameter 4e-5, LMM 0.5 / particle 0.5 / slowly 0.3,
      z uniform over the water column;
  (b) 'LMM + Colloid + Rev', isotope Al, with a salinity field that reaches all four intervals of the rate tables and a few
      elements whose salinity is exactly 0, 1, 10 and 20 (plateaus of the field).

The time steps are long (case (a) 6 h, case (b) 12 h) so that the rare transformations occur often enough in a file below 1 MB;
the mixing sub-step is 10 min.  The golden feeds kernel-level tests: every launch is replayed from the state the reference had
in front of the method it restates, so the mixing itself is not stored.

Stored per step, by element ID (all elements stay active): in front of update_speciation z0 / specie0 / moving0 / diameter0 and
the float32 environment; its draws scattered to the element they were used for (u1 for every element; u2, the diameter noise and
the desorption noise where drawn, NaN elsewhere); specie1 / moving1 / diameter1 / z1 behind it; the terminal velocity of the
first update_terminal_velocity of the step; z2 / specie2 / moving2 in front of resuspension; its two noises; specie3 / moving3 /
diameter3 / z3 behind it; z_f32, whether elements.z was still the float32 array of the seeding in front of update_speciation (the
first step: what update_speciation stores into z is rounded to it); the cumulative ntransformations behind speciation, behind the mixing and behind the step; psum of
update_speciation; transfer_rates and name_species of the four specie setups that work in the reference (setup0 .. setup3).  z1 and z3 hold NaN where the value is z0 / z2 bit for bit.  lon / lat / z at seeding and after the last step.

np.random.* is recorded by oracle.refdriver.RecordingRandom; np.random.default_rng, which set_init_diameter calls without a seed
(:297), is replaced for the duration of a step by a function that returns a seeded generator whose normal / lognormal calls are
recorded -- the reference is not edited.  Locals of update_speciation and resuspension are read by a tracer when they return.
The dtype of every intermediate the device code restates is asserted (DTYPES and the checks in step functions): Zmin = -1.*depth
is float32, Zmin + resuspension_depth and -depth + desorption_depth stay float32 under NumPy 2 and are stored into the float64 z.

Conditions asserted here so that the golden cannot hide a failure:
  (1) every non-zero entry of transfer_rates of (a) has >= 20 transformations over the run;
  (2) every non-zero entry of at least three of the four salinity tables of (b) has >= 5;
  (3) in some step >= 5 % of the elements end with moving == 0;
  (4) in some step >= 5 % are resuspended;
  (5) >= 20 element-steps lose the LMM -> sediment rate to the layer-thickness test, (6) >= 20 keep it;
  (7) >= 3 element-steps are clamped at z = 0;
  (8) >= 3 are left below the sea floor by the desorption noise;
  (9) every stored value of a present element is finite.

    python tools/gen_golden_radionuclides.py
"""
import os
import sys
from datetime import timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

assert refshim.install(), 'reference tree not found'
from oracle import gen_golden as gg  # noqa: E402
from oracle.refdriver import RefStepper, RecordingRandom  # noqa: E402
from opendrift.models.radionuclides import RadionuclideDrift  # noqa: E402

ENV = {'depth': 'sea_floor_depth_below_sea_level', 'conc3': 'conc3', 'sal': 'sea_water_salinity', 'temp': 'sea_water_temperature',
       'u': 'x_sea_water_velocity', 'v': 'y_sea_water_velocity'}
CASES = {'a': dict(N=1500, steps=7, dt=21600.0, setup='LMM + Rev + Slow rev + Irrev', isotope='241Am'),
         'b': dict(N=1000, steps=7, dt=43200.0, setup='LMM + Colloid + Rev', isotope='Al')}
DT_MIX = 600.0
# locals of update_speciation / resuspension with the dtype NumPy gives them
DTYPES = {'p': np.float64, 'psum': np.float64, 'ran1': np.float64, 'ran4': np.float64, 'Zmin': np.float32, 'speed': np.float32}


def fields(case):
    x = np.linspace(4.0, 5.0, 41)
    y = np.linspace(60.0, 60.5, 33)
    lon, lat = np.meshgrid(x, y)
    X, Y = (lon - 4.0), (lat - 60.0) * 2          # 0 .. 1
    g = {}
    g['sea_floor_depth_below_sea_level'] = 30 + 10 * np.sin(2 * np.pi * X) * np.cos(np.pi * Y)
    g['conc3'] = 2e-3 + 1.5e-3 * np.cos(2 * np.pi * Y) * np.sin(np.pi * X)
    # slow patch in the south-west: below the critical velocity of 0.01 m/s; about 0.03 m/s elsewhere
    slow = (X < 0.6) & (Y < 0.7)
    g['x_sea_water_velocity'] = np.where(slow, 0.004, 0.025 + 0.01 * Y)
    g['y_sea_water_velocity'] = np.where(slow, -0.003, 0.015 * np.cos(np.pi * X))
    g['sea_water_temperature'] = 6 + 6 * Y
    if case == 'a':
        g['sea_water_salinity'] = 30 + 5 * X
    else:   # plateaus at exactly 0, 1, 10 and 20 joined by ramps that cover all four intervals, 32 at the eastern edge
        knots_x = [0.0, 0.05, 0.20, 0.25, 0.40, 0.45, 0.60, 0.65, 0.80, 1.0]
        knots_s = [0.0, 0.0, 1.0, 1.0, 10., 10., 20., 20., 27., 32.]
        g['sea_water_salinity'] = np.interp(X, knots_x, knots_s)
    g['land_binary_mask'] = np.zeros(lon.shape)
    g = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in g.items()}
    g.update(x=x, y=y)
    return g


class RecordingGenerator:
    """What np.random.default_rng() returns during a step: a seeded generator whose draws are recorded."""

    def __init__(self, seed, draws):
        self.g, self.draws = np.random.Generator(np.random.PCG64(seed)), draws

    def normal(self, loc, scale, size):
        r = self.g.normal(loc, scale, size)
        self.draws.append(np.array(r, copy=True))
        return r

    def lognormal(self, mean, sigma, size):
        r = self.g.lognormal(mean, sigma, size=size)
        self.draws.append(np.array(r, copy=True))
        return r


class Tracer:
    """The locals of the named methods of the model's class when they return."""

    def __init__(self, *methods):
        self.codes = {m.__code__: m.__name__ for m in methods}
        self.locals = {}

    def __call__(self, frame, event, arg):
        if event == 'call' and frame.f_code in self.codes:
            return self.local
        return None

    def local(self, frame, event, arg):
        if event == 'return':
            self.locals[self.codes[frame.f_code]] = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v)
                                                     for k, v in frame.f_locals.items()}
        return self.local


def case(name, g, seed):
    C = CASES[name]
    N, STEPS, DT = C['N'], C['steps'], C['dt']
    times = [gg.T0 + timedelta(seconds=float(t)) for t in np.arange(STEPS + 2) * DT]
    one = np.ones((len(times), 1, 1), np.float32)
    o = RadionuclideDrift(loglevel=50)
    o.set_config('general:use_auto_landmask', False)
    o.add_reader(gg.GridReader('+proj=latlong', g['x'], g['y'], times, {k: one * v for k, v in g.items() if k not in 'xy'}))
    o.set_config('environment:constant:horizontal_diffusivity', 0.0)
    o.set_config('radionuclide:isotope', C['isotope'])
    o.set_config('radionuclide:specie_setup', C['setup'])
    o.set_config('vertical_mixing:timestep', DT_MIX)
    o.set_config('radionuclide:particle_diameter', 4e-5)
    o.set_config('radionuclide:particle_diameter_uncertainty', 2e-6)
    # resuspension 18 m +- 8 m above a floor at 20 - 40 m: some elements are clamped at the surface (7); desorption 1 m +- 1.2 m:
    # some are left below the floor (8)
    o.set_config('radionuclide:sediment:resuspension_depth', 18.)
    o.set_config('radionuclide:sediment:resuspension_depth_uncert', 8.)
    o.set_config('radionuclide:sediment:desorption_depth_uncert', 1.2)
    if name == 'a':
        o.set_config('radionuclide:transformations:slow_coeff', 2e-5)
        o.set_config('seed:LMM_fraction', 0.5)
        o.set_config('seed:particle_fraction', 0.5)
        o.set_config('seed:slowly_fraction', 0.3)
    else:
        o.set_config('seed:LMM_fraction', 0.3)
        o.set_config('seed:particle_fraction', 0.7)
    assert o.get_config('drift:vertical_mixing') is True and o.get_config('general:seafloor_action') == 'lift_to_seafloor'
    rng = np.random.default_rng(seed)
    lon = rng.uniform(4.1, 4.78, N)
    lat = rng.uniform(60.05, 60.4, N)
    if name == 'b':     # a few elements on each plateau of the salinity field (the plateaus are 0.05 deg wide: they leave them after a step or two)
        lon = rng.uniform(4.06, 4.78, N)
        for k, x0 in enumerate((0.025, 0.225, 0.425, 0.625)):
            lon[8 * k:8 * k + 8] = 4.0 + x0 + rng.uniform(-0.01, 0.01, 8)
            lat[8 * k:8 * k + 8] = rng.uniform(60.05, 60.3, 8)
    depth_at = 30 + 10 * np.sin(2 * np.pi * (lon - 4.0)) * np.cos(np.pi * (lat - 60.0) * 2)
    z = -rng.uniform(0.02, 0.98, N) * depth_at
    np.random.seed(seed)
    seed_rng, seed_draws = np.random.default_rng, []
    np.random.default_rng = lambda: RecordingGenerator(999 * seed, seed_draws)      # (the initial diameters: unseeded in the reference)
    try:
        o.seed_elements(lon=lon, lat=lat, z=z, time=gg.T0, number=N)
    finally:
        np.random.default_rng = seed_rng
    assert len(seed_draws) == 1
    ns = o.nspecies
    nsal = o.transfer_rates.shape[0] if o.transfer_rates.ndim == 3 else 1
    dissolved = o.num_lmmcation if name == 'b' else o.num_lmm

    rec = {'gen': [], 'tv': None}
    tracer = Tracer(RadionuclideDrift.update_speciation, RadionuclideDrift.resuspension)
    ref = dict(spec=o.update_speciation, tv=o.update_terminal_velocity, diam=o.set_init_diameter, des=o.desorption_from_sediments,
               res=o.resuspension, rates=o.update_transfer_rates)
    gen_seed = [1000 * seed]

    def default_rng(*a):
        assert not a
        gen_seed[0] += 1
        return RecordingGenerator(gen_seed[0], rec['gen'])

    def snap():
        e = o.elements
        assert e.z.dtype in (np.float32, np.float64) and e.diameter.dtype == np.float32
        return dict(z=np.array(e.z, dtype=np.float64), specie=np.array(e.specie, dtype=np.int8), moving=np.array(e.moving, dtype=np.int8),
                    diameter=np.array(e.diameter))

    def update_transfer_rates():
        ref['rates']()
        rec['rates1D'] = np.array(o.elements.transfer_rates1D)
        assert rec['rates1D'].dtype == np.float64 and rec['rates1D'].flags['C_CONTIGUOUS']

    def set_init_diameter(num, idxs, diam):
        n0 = len(rec['gen'])
        r = ref['diam'](num, idxs, diam)
        assert len(rec['gen']) == n0 + 1 and r.dtype == np.float64
        rec['diam_calls'].append((np.asarray(idxs, dtype=int), rec['gen'][-1], diam))
        return r

    def desorption(sp_in=None, sp_out=None):
        n0 = len(rec['rr'].draws)
        zb = np.array(o.elements.z)
        ref['des'](sp_in, sp_out)
        mask = (sp_out == dissolved) & (sp_in == o.num_srev)
        new = rec['rr'].draws[n0:]
        noise = np.full(len(mask), np.nan)
        if mask.any():
            new = [d for d in new if len(d[1])]
            assert len(new) == 1 and new[0][0] == 'normal' and len(new[0][1]) == mask.sum()
            noise[mask] = new[0][1]
            depth = o.environment.sea_floor_depth_below_sea_level
            base = -1. * depth[mask] + o.get_config('radionuclide:sediment:desorption_depth')
            assert base.dtype == np.float32
            # (in the step the elements are released in, z is still the float32 array of the seeding: the sum is rounded to it)
            assert np.array_equal(o.elements.z[mask], np.minimum((base.astype(np.float64) + noise[mask]).astype(o.elements.z.dtype), 0))
            rec['below_floor'] += int((o.elements.z[mask] < -depth[mask].astype(np.float64)).sum())
        else:
            assert all(len(d[1]) == 0 for d in new)      # (normal(0, std, 0) is still called)
        rec['clamped'] += int(((zb > 0) | ((noise == noise) & (o.elements.z == 0))).sum())
        rec['desorb_noise'] = noise

    def update_speciation():
        rec['s0'] = snap()
        rec['z_f32'] = o.elements.z.dtype == np.float32
        rec['env'] = {k: np.array(getattr(o.environment, v)) for k, v in ENV.items()}
        for k in rec['env'].values():
            assert k.dtype == np.float32
        rec['diam_calls'], rec['desorb_noise'] = [], np.full(len(o.elements), np.nan)
        n0 = len(rec['rr'].draws)
        sys.settrace(tracer)
        try:
            ref['spec']()
        finally:
            sys.settrace(None)
        L = tracer.locals['update_speciation']
        for k in ('p', 'psum', 'ran1'):
            assert L[k].dtype == DTYPES[k], k
        n = len(o.elements)
        rec['u1'], rec['psum'] = L['ran1'], L['psum']
        assert rec['rr'].draws[n0][0] == 'random' and np.array_equal(rec['rr'].draws[n0][1], L['ran1'])
        ph = L['phaseshift']
        u2 = np.full(n, np.nan)
        if ph.any():
            assert L['ran4'].dtype == np.float64 and np.array_equal(rec['rr'].draws[n0 + 1][1], L['ran4'])
            u2[ph] = L['ran4']
            assert L['specie_out'].max() < ns, 'a species decision ran past the table: change the seed'
        rec['u2'], rec['ph'] = u2, ph
        noise = np.full(n, np.nan)
        for idxs, draws, diam in rec['diam_calls']:
            assert np.isnan(noise[idxs]).all() and len(idxs) == len(draws)
            noise[idxs] = draws
        rec['diam_noise1'] = noise
        rec['s1'] = snap()
        rec['nt1'] = np.array(o.ntransformations)
        # the two sides of the layer-thickness test (5), (6)
        if name == 'a':
            lmm = rec['s0']['specie'] == o.num_lmm
            Zmin = -1. * rec['env']['depth']
            assert Zmin.dtype == np.float32 and (rec['s0']['z'] - Zmin).dtype == np.float64
            far = (rec['s0']['z'] - Zmin) > o.get_config('radionuclide:sediment:layer_thick')
            assert (rec['rates1D'][lmm & far, o.num_srev] == 0).all() and (rec['rates1D'][lmm & ~far, o.num_srev] > 0).all()
            rec['far'] += int((lmm & far).sum())
            rec['near'] += int((lmm & ~far).sum())
        rec['first_tv'] = True

    def update_terminal_velocity(*a, **k):
        ref['tv'](*a, **k)
        if rec.get('first_tv'):
            rec['first_tv'] = False
            tv = o.elements.terminal_velocity
            # elements.density was not given at seeding: the default seeds a FLOAT64 array, so DENSw - DENSpart and the last product
            # of W are float64 there (a density given at seeding would be float32 and W float32 throughout).  Stored rounded to
            # float32, which is what the device holds
            assert tv.dtype == np.float64 and o.elements.density.dtype == np.float64 and o.elements.diameter.dtype == np.float32
            rec['tv'] = tv.astype(np.float32)

    def resuspension():
        rec['s2'] = snap()
        assert o.elements.z.dtype == np.float64      # (the mixing has made it one)
        rec['nt2'] = np.array(o.ntransformations)
        rec['diam_calls'] = []
        n0 = len(rec['rr'].draws)
        sys.settrace(tracer)
        try:
            ref['res']()
        finally:
            sys.settrace(None)
        L = tracer.locals['resuspension']
        assert L['Zmin'].dtype == np.float32 and L['speed'].dtype == np.float32
        resusp = L['resusp']
        n = len(resusp)
        noise = np.full(n, np.nan)
        new = rec['rr'].draws[n0:]
        if resusp.any():
            assert len(new) == 1 and new[0][0] == 'normal' and len(new[0][1]) == resusp.sum()
            noise[resusp] = new[0][1]
            base = L['Zmin'][resusp] + L['resusp_depth']
            assert base.dtype == np.float32
            assert np.array_equal(o.elements.z[resusp], np.minimum(base.astype(np.float64) + noise[resusp], 0))
            rec['clamped'] += int((o.elements.z[resusp] == 0).sum())
        rec['resusp'], rec['resusp_noise'] = resusp, noise
        dn = np.full(n, np.nan)
        for idxs, draws, diam in rec['diam_calls']:
            dn[idxs] = draws
        rec['diam_noise3'] = dn
        rec['s3'] = snap()

    o.update_transfer_rates, o.update_speciation, o.update_terminal_velocity = update_transfer_rates, update_speciation, update_terminal_velocity
    o.set_init_diameter, o.desorption_from_sediments, o.resuspension = set_init_diameter, desorption, resuspension
    rec.update(far=0, near=0, clamped=0, below_floor=0)

    st = RefStepper(o, DT, STEPS)
    f64 = lambda: np.full((STEPS, N), np.nan)                    # noqa: E731
    f32 = lambda: np.full((STEPS, N), np.nan, np.float32)        # noqa: E731
    i8 = lambda: np.full((STEPS, N), -1, np.int8)                # noqa: E731
    out = {k: f64() for k in ('z0', 'z1', 'z2', 'z3', 'u1', 'u2', 'psum', 'diam_noise1', 'desorb_noise', 'diam_noise3', 'resusp_noise')}
    out.update({k: f32() for k in ('diameter0', 'diameter1', 'diameter3', 'tv') + tuple('env_' + e for e in ENV)})
    out.update({k: i8() for k in ('specie0', 'specie1', 'specie2', 'specie3', 'moving0', 'moving1', 'moving2', 'moving3')})
    out['ntrans1'], out['ntrans2'], out['ntrans3'] = (np.zeros((STEPS, ns, ns), np.int64) for _ in range(3))
    out['z_f32'] = np.zeros(STEPS, bool)
    sch = o.elements_scheduled
    out['seed_lon'], out['seed_lat'], out['seed_z'] = np.array(sch.lon), np.array(sch.lat), np.array(sch.z)
    out['seed_specie'], out['seed_diameter'] = np.array(sch.specie, dtype=np.int8), np.array(sch.diameter, dtype=np.float32)
    frac_settled, frac_resusp = 0.0, 0.0
    orig_rng = np.random.default_rng
    for s in range(STEPS):
        with RecordingRandom() as rr:
            rec['rr'] = rr
            np.random.default_rng = default_rng
            try:
                st.step()
            finally:
                np.random.default_rng = orig_rng
        ID = np.asarray(o.elements.ID, dtype=int)
        assert len(ID) == N and np.array_equal(ID, np.arange(N))       # nobody is deactivated: arrays are in ID order
        for j in '0123':
            S = rec['s' + j]
            out['z' + j][s], out['specie' + j][s], out['moving' + j][s] = S['z'], S['specie'], S['moving']
            if j != '2':
                out['diameter' + j][s] = S['diameter']
        assert np.array_equal(rec['s2']['diameter'], rec['s1']['diameter'])
        for k in ('u1', 'u2', 'psum', 'diam_noise1', 'desorb_noise', 'diam_noise3', 'resusp_noise', 'tv'):
            out[k][s] = rec[k]
        for k in ENV:
            out['env_' + k][s] = rec['env'][k]
        out['ntrans1'][s], out['ntrans2'][s], out['ntrans3'][s] = rec['nt1'], rec['nt2'], o.ntransformations
        out['z_f32'][s] = rec['z_f32']
        frac_settled = max(frac_settled, float((o.elements.moving == 0).mean()))
        frac_resusp = max(frac_resusp, float(rec['resusp'].mean()))
        # the margin of every decision: |u1 - psum| in units of the spacing of psum
        with np.errstate(invalid='ignore', divide='ignore'):
            m = np.abs(rec['u1'] - rec['psum']) / np.spacing(np.maximum(rec['psum'], 1e-300))
        rec['margin'] = min(rec.get('margin', np.inf), float(m.min()))
    lon, lat, z, status = st.state()
    assert (status == 0).all()
    out['end_lon'], out['end_lat'], out['end_z'] = lon, lat, z
    out['transfer_rates'] = np.array(o.transfer_rates)
    out['name_species'] = np.array(o.name_species)
    cfg = ('radionuclide:particle_diameter', 'radionuclide:dissolved_diameter', 'radionuclide:particle_diameter_uncertainty',
           'radionuclide:sediment:layer_thick', 'radionuclide:sediment:desorption_depth', 'radionuclide:sediment:desorption_depth_uncert',
           'radionuclide:sediment:resuspension_depth', 'radionuclide:sediment:resuspension_depth_uncert',
           'radionuclide:sediment:resuspension_critvel', 'radionuclide:transformations:slow_coeff', 'seed:LMM_fraction',
           'seed:particle_fraction', 'seed:slowly_fraction')
    out['config_keys'] = np.array(cfg)
    out['config_values'] = np.array([o.get_config(k) for k in cfg], dtype=np.float64)
    out['dt'], out['dt_mix'], out['seed'] = DT, DT_MIX, seed
    stats = dict(frac_settled=frac_settled, frac_resusp=frac_resusp, far=rec['far'], near=rec['near'], clamped=rec['clamped'],
                 below_floor=rec['below_floor'], margin=rec['margin'], nsal=nsal)
    return out, stats


def check(name, out, stats):
    nt, rates = out['ntrans3'][-1], out['transfer_rates']
    print('case %s: %s' % (name, stats))
    print(nt)
    if name == 'a':
        nz = rates > 0
        print('smallest count of a non-zero rate: %d' % nt[nz].min())
        assert nt[nz].min() >= 20, '(1)'
        assert stats['far'] >= 20, '(5)'
        assert stats['near'] >= 20, '(6)'
    else:
        # which table a transformation of update_speciation came from: the salinity interval of the element in that step
        sal = out['env_sal']
        sali = np.searchsorted([0, 1, 10, 20], sal) - 1
        changed = out['specie1'] != out['specie0']
        ok = 0
        for a in range(4):
            sel = changed & (sali == (a if a < 3 else 3)) if a < 3 else changed & ((sali == 3) | (sali == -1))
            cnt = np.zeros(rates.shape[1:], int)
            np.add.at(cnt, (out['specie0'][sel], out['specie1'][sel]), 1)
            nz = rates[a] > 0
            print('table %d: smallest count of a non-zero rate %d' % (a, cnt[nz].min()))
            ok += cnt[nz].min() >= 5
        assert ok >= 3, '(2)'
        for v in (0, 1, 10, 20):
            assert (sal == v).sum() >= 3, 'salinity exactly %s' % v
    assert stats['frac_settled'] >= 0.05, '(3)'
    assert stats['frac_resusp'] >= 0.05, '(4)'
    assert stats['clamped'] >= 3, '(7)'
    assert stats['below_floor'] >= 3, '(8)'
    assert stats['margin'] > 4, 'a species decision is marginal (u1 within 4 ulp of psum): change the seed'
    for k, v in out.items():      # (9)
        if k in ('u2', 'diam_noise1', 'desorb_noise', 'diam_noise3', 'resusp_noise', 'config_keys', 'name_species'):
            continue
        if isinstance(v, np.ndarray) and v.dtype.kind == 'f':
            assert np.isfinite(v).all(), k


def main():
    data = {}
    for name, seed in (('a', 30), ('b', 31)):
        g = fields(name)
        out, stats = case(name, g, seed)
        check(name, out, stats)
        for j, k in (('1', '0'), ('3', '2')):      # z behind a launch: NaN where it is the z in front of it, bit for bit
            same = out['z' + j].view(np.int64) == out['z' + k].view(np.int64)
            out['z' + j] = np.where(same, np.nan, out['z' + j])
        data.update({'%s_g_%s' % (name, k): v for k, v in g.items()})
        data.update({'%s_%s' % (name, k): v for k, v in out.items()})
    # transfer_rates and name_species of the four specie setups whose init_transfer_rates works in the reference ('LMM + Rev + Irrev'
    # fails there: :579 reads num_ssrev, which that setup never sets), with case (a)'s slow_coeff
    for k, (setup, isotope) in enumerate((('LMM + Rev', '137Cs'), ('LMM + Rev + Slow rev', '241Am'), ('LMM + Rev + Slow rev + Irrev', '129I'),
                                          ('LMM + Colloid + Rev', 'Al'))):
        o = RadionuclideDrift(loglevel=50)
        o.set_config('radionuclide:isotope', isotope)
        o.set_config('radionuclide:specie_setup', setup)
        o.set_config('radionuclide:transformations:slow_coeff', 2e-5)
        o.check_speciation()
        o.init_species()
        o.init_transfer_rates()
        data.update({'setup%d_name' % k: np.array(setup), 'setup%d_isotope' % k: np.array(isotope), 'setup%d_species' % k: np.array(o.name_species),
                     'setup%d_rates' % k: np.array(o.transfer_rates)})
    path = os.path.join(gg.GOLD, 'c30_radionuclides.npz')
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
