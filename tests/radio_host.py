"""TEST INFRASTRUCTURE: ctypes access to the per-element code of opendrift_amd/csrc/odr_radio.hip.h compiled for the host
(g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see radio_host.cpp; and the golden C30 as the launches
see it (setup members from its stored configuration, one step's inputs, draws and expected outputs)."""
import ctypes as C
import os

import numpy as np

from host_build import f32, f64, host_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'c30_radionuclides.npz')
_fp, _dp, _ip, _lp = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
SPECIES = {'lmm': 'LMM', 'lmmcation': 'LMMcation', 'lmmanion': 'LMManion', 'polymer': 'Polymer', 'particle_rev': 'Particle reversible',
           'sediment_rev': 'Sediment reversible', 'particle_slow': 'Particle slowly reversible', 'sediment_slow': 'Sediment slowly reversible',
           'particle_irrev': 'Particle irreversible', 'sediment_irrev': 'Sediment irreversible'}
CONFIG = {'layer_thick': 'radionuclide:sediment:layer_thick', 'particle_diameter': 'radionuclide:particle_diameter',
          'dissolved_diameter': 'radionuclide:dissolved_diameter', 'diameter_uncertainty': 'radionuclide:particle_diameter_uncertainty',
          'desorption_depth': 'radionuclide:sediment:desorption_depth', 'desorption_depth_uncert': 'radionuclide:sediment:desorption_depth_uncert',
          'resuspension_depth': 'radionuclide:sediment:resuspension_depth',
          'resuspension_depth_uncert': 'radionuclide:sediment:resuspension_depth_uncert',
          'resuspension_critvel': 'radionuclide:sediment:resuspension_critvel'}


def _lib():
    return host_lib('radio_host', ('odr_radio.hip.h', 'odr_seawater.hip.h'))


def golden_setup(G, case):
    """The members of odr_radio_setup (device.Particles.radio_setup(**members)) from the configuration stored with a case."""
    names = list(G[case + '_name_species'])
    cfg = dict(zip(G[case + '_config_keys'].tolist(), G[case + '_config_values'].tolist()))
    m = {k: (names.index(v) if v in names else -1) for k, v in SPECIES.items()}
    m.update({k: cfg[v] for k, v in CONFIG.items()})
    m.update(rates=np.array(G[case + '_transfer_rates']), nspecies=len(names), lognormal=False)
    return m


def _setup_vector(m, dt):
    return np.array([dt, m['layer_thick'], m['particle_diameter'], m['dissolved_diameter'], m['diameter_uncertainty'],
                     m['desorption_depth_uncert'], m['resuspension_depth_uncert'], m['desorption_depth'], m['resuspension_depth'],
                     m['resuspension_critvel'], m['nspecies'], 1 if np.ndim(m['rates']) == 2 else len(m['rates']), int(bool(m['lognormal']))] +
                    [m[k] for k in SPECIES], dtype=np.float64)


def _table(m):
    r = np.asarray(m['rates'], np.float64)
    r = r[None] if r.ndim == 2 else r
    t = np.zeros((4, 7, 7))
    t[:r.shape[0], :r.shape[1], :r.shape[2]] = r
    return np.ascontiguousarray(t)


def speciation(m, dt, specie, diameter, moving, z, sal, depth, conc3, u1, u2, diameter_noise, depth_noise, noise_is_final=True):
    """One odr_radio_speciation launch on the host: returns dict(specie, diameter, moving, z, counts[7, 7], bad)."""
    n = len(specie)
    sp, di, mv, zz = np.array(specie, np.float32), np.array(diameter, np.float32), np.array(moving, np.int32), np.array(z, np.float64)
    counts = np.zeros(50, np.int64)
    st, tb = _setup_vector(m, dt), _table(m)
    ins = [f32(sal, n), f32(depth, n), f32(conc3, n)]
    dr = [f64(a, n) for a in (u1, u2, diameter_noise, depth_noise)]
    _lib().radioh_speciation(C.c_longlong(n), st.ctypes.data_as(_dp), tb.ctypes.data_as(_dp), sp.ctypes.data_as(_fp), di.ctypes.data_as(_fp),
                            mv.ctypes.data_as(_ip), zz.ctypes.data_as(_dp), *[a.ctypes.data_as(_fp) for a in ins],
                            *[a.ctypes.data_as(_dp) for a in dr], C.c_int(int(noise_is_final)), counts.ctypes.data_as(_lp))
    return dict(specie=sp, diameter=di, moving=mv, z=zz, counts=counts[:49].reshape(7, 7)[:m['nspecies'], :m['nspecies']].copy(), bad=int(counts[49]))


def probabilities(m, dt, specie, z, sal, depth, conc3):
    """(p[n, 7], psum[n]) of radio_probabilities."""
    n = len(specie)
    p, ps = np.zeros((n, 7)), np.zeros(n)
    st, tb = _setup_vector(m, dt), _table(m)
    a = [f32(specie, n), f64(z, n), f32(sal, n), f32(depth, n), f32(conc3, n)]
    _lib().radioh_probabilities(C.c_longlong(n), st.ctypes.data_as(_dp), tb.ctypes.data_as(_dp), a[0].ctypes.data_as(_fp),
                               a[1].ctypes.data_as(_dp), a[2].ctypes.data_as(_fp), a[3].ctypes.data_as(_fp), a[4].ctypes.data_as(_fp),
                               p.ctypes.data_as(_dp), ps.ctypes.data_as(_dp))
    return p, ps


def terminal_velocity(temperature, salinity, diameter, density, moving):
    n = len(temperature)
    a = [f32(x, n) for x in (temperature, salinity, diameter, density)]
    mv = np.ascontiguousarray(np.broadcast_to(np.asarray(moving, np.int32), (n,)))
    w = np.empty(n, np.float32)
    _lib().radioh_terminal_velocity(C.c_longlong(n), *[x.ctypes.data_as(_fp) for x in a], mv.ctypes.data_as(_ip), w.ctypes.data_as(_fp))
    return w


def resuspend(m, specie, diameter, moving, z, u, v, depth, diameter_noise, depth_noise, noise_is_final=True):
    """One odr_radio_resuspend launch on the host: returns dict(specie, diameter, moving, z, counts[7, 7], bad)."""
    n = len(specie)
    sp, di, mv, zz = np.array(specie, np.float32), np.array(diameter, np.float32), np.array(moving, np.int32), np.array(z, np.float64)
    counts = np.zeros(50, np.int64)
    st = _setup_vector(m, 0.0)
    ins = [f32(u, n), f32(v, n), f32(depth, n)]
    dr = [f64(a, n) for a in (diameter_noise, depth_noise)]
    _lib().radioh_resuspend(C.c_longlong(n), st.ctypes.data_as(_dp), sp.ctypes.data_as(_fp), di.ctypes.data_as(_fp), mv.ctypes.data_as(_ip),
                           zz.ctypes.data_as(_dp), *[a.ctypes.data_as(_fp) for a in ins], *[a.ctypes.data_as(_dp) for a in dr],
                           C.c_int(int(noise_is_final)), counts.ctypes.data_as(_lp))
    return dict(specie=sp, diameter=di, moving=mv, z=zz, counts=counts[:49].reshape(7, 7)[:m['nspecies'], :m['nspecies']].copy(), bad=int(counts[49]))


class Golden:
    """C30 as the launches see it."""

    def __init__(self):
        self.G = np.load(GOLDEN)

    def steps(self, case):
        return len(self.G[case + '_u1'])

    def setup(self, case):
        return golden_setup(self.G, case)

    def dt(self, case):
        return float(self.G[case + '_dt'])

    def speciation_step(self, case, s):
        """(inputs, draws, expected) of update_speciation in step s.  Unused draws are 0 (the golden holds NaN there).  expected z:
        the reference's; in a step whose z array was still float32 (z_f32) what the launch stores is rounded to it."""
        G, c = self.G, case + '_'
        inp = dict(specie=G[c + 'specie0'][s].astype(np.float32), diameter=G[c + 'diameter0'][s], moving=G[c + 'moving0'][s].astype(np.int32),
                   z=G[c + 'z0'][s], sal=G[c + 'env_sal'][s], depth=G[c + 'env_depth'][s], conc3=G[c + 'env_conc3'][s])
        draws = dict(u1=G[c + 'u1'][s], u2=np.nan_to_num(G[c + 'u2'][s]), diameter_noise=np.nan_to_num(G[c + 'diam_noise1'][s]),
                     depth_noise=np.nan_to_num(G[c + 'desorb_noise'][s]))
        z1 = np.where(np.isnan(G[c + 'z1'][s]), G[c + 'z0'][s], G[c + 'z1'][s])
        exp = dict(specie=G[c + 'specie1'][s].astype(np.float32), diameter=G[c + 'diameter1'][s], moving=G[c + 'moving1'][s].astype(np.int32), z=z1,
                   counts=G[c + 'ntrans1'][s] - (G[c + 'ntrans3'][s - 1] if s else 0), z_f32=bool(G[c + 'z_f32'][s]), psum=G[c + 'psum'][s])
        return inp, draws, exp

    def resuspension_step(self, case, s):
        """(inputs, draws, expected) of the resuspension launch in step s: the species the elements had behind update_speciation
        (the mixing does not change them on the device), moving and z in front of the reference's resuspension(); expected counts:
        bottom_interaction's of the step's mixing plus resuspension's."""
        G, c = self.G, case + '_'
        inp = dict(specie=G[c + 'specie1'][s].astype(np.float32), diameter=G[c + 'diameter1'][s], moving=G[c + 'moving2'][s].astype(np.int32),
                   z=G[c + 'z2'][s], u=G[c + 'env_u'][s], v=G[c + 'env_v'][s], depth=G[c + 'env_depth'][s])
        draws = dict(diameter_noise=np.nan_to_num(G[c + 'diam_noise3'][s]), depth_noise=np.nan_to_num(G[c + 'resusp_noise'][s]))
        z3 = np.where(np.isnan(G[c + 'z3'][s]), G[c + 'z2'][s], G[c + 'z3'][s])
        exp = dict(specie=G[c + 'specie3'][s].astype(np.float32), diameter=G[c + 'diameter3'][s], moving=G[c + 'moving3'][s].astype(np.int32), z=z3,
                   counts=G[c + 'ntrans3'][s] - G[c + 'ntrans1'][s])
        return inp, draws, exp

    def terminal_velocity_step(self, case, s):
        G, c = self.G, case + '_'
        n = G[c + 'tv'].shape[1]
        inp = dict(temperature=G[c + 'env_temp'][s], salinity=G[c + 'env_sal'][s], diameter=G[c + 'diameter1'][s],
                   density=np.full(n, 2650., np.float32), moving=G[c + 'moving1'][s].astype(np.int32))
        return inp, G[c + 'tv'][s]
