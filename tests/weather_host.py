"""TEST INFRASTRUCTURE: ctypes access to the per-element code of opendrift_amd/csrc/odr_weather.hip.h compiled for the host
(g++ -ffp-contract=off, tests/hostshim in place of the HIP runtime header), see weather_host.cpp; and the golden C39 as the launches
see it (the oil of a case, one step's state in front of any of its processes, the state the reference had behind it)."""
import ctypes as C
import os

import numpy as np

from host_build import host_lib
from opendrift_amd import _abi
from opendrift_amd.device import weathering_table

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'c39_openoil_weathering.npz')
_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
REC = _abi.WEATHER_RECORD
STATE = REC[:9]                  # what a step can change
# the stages of a step in the reference's order: (golden prefix, process flag, what it changes)
STAGES = (('p', 'properties', ('density', 'viscosity', 'fraction_evaporated')), ('e', 'evaporation', ('mass_oil', 'mass_evaporated')),
          ('m', 'emulsification', ('interfacial_area', 'water_fraction')), ('d', 'dispersion', ('mass_oil', 'mass_dispersed')),
          ('b', 'biodegradation', ('mass_oil', 'mass_biodegraded')))
ENV = ('xwind', 'ywind', 'temp', 'hs', 'tp')


# Largest distance from the golden in float64 units in the last place, measured with the host build over every step of C39 and
# doubled (tests/test_weather_device_arithmetic.py prints the measured figures).  Two regimes.  NumPy evaluates float32 pow and exp
# with vector code of its own that lies one float32 ulp from libm's on 10 - 50 % of the arguments here: the mass transport
# coefficient of evaporation (ws ** 0.78) and Adcroft's tau and fraction (3 ** x, exp) carry that ulp -- 6e-8 relative -- into the
# float64 masses, through an exponential in evaporation and through 1 - exp(-1e-4) in Adcroft: 'all'.  On the elements where the
# float32 function values of the host build and NumPy agree only float64 exp / pow calls separate the two: 'same'.
# Measured: all {mass_oil 966922235, mass_evaporated 1143413952, mass_dispersed 65662775, mass_biodegraded 1996866579129,
# mass_components 17693561691, viscosity 5, interfacial_area 1, water_fraction 2}; same {mass_oil 2, mass_evaporated 128 (a sum of
# differences m - m exp(..)), mass_dispersed 3, mass_components 53, mass_biodegraded 0: taken as 1, one exp call}.
# density and fraction_evaporated pass through + - * / only: bit for bit.
BOUNDS = {'all': dict(mass_oil=1933844470, mass_evaporated=2286827904, mass_dispersed=131325550, mass_biodegraded=3993733158258,
                      mass_components=35387123382, viscosity=10, interfacial_area=2, water_fraction=4, density=0, fraction_evaporated=0),
          'same': dict(mass_oil=4, mass_evaporated=256, mass_dispersed=6, mass_biodegraded=2, mass_components=106, viscosity=10,
                       interfacial_area=2, water_fraction=4, density=0, fraction_evaporated=0)}
# 'all' is one maximum over the cases; the host build is also held to each case's own figures (measured per case over the whole step
# and every process alone, doubled; what a case leaves bit for bit stays bit for bit).  half_time's mass_biodegraded in (b) is not
# exact over the whole step because it is a fraction of the mass_oil that evaporation left.
_CASE = dict(a=dict(mass_oil=72055966, mass_evaporated=576447728, mass_dispersed=65662775, mass_components=17693561691, viscosity=5,
                    interfacial_area=1, water_fraction=2),
             b=dict(mass_oil=98680730, mass_evaporated=789445841, mass_dispersed=52149914, mass_biodegraded=45711509,
                    mass_components=16101637033, viscosity=3, interfacial_area=1, water_fraction=1),
             c=dict(mass_oil=966922235, mass_evaporated=1143413952, mass_dispersed=7798729, mass_biodegraded=1996866579129,
                    mass_components=966922235, viscosity=3, interfacial_area=1, water_fraction=2),
             d=dict(mass_oil=1, mass_dispersed=3, viscosity=2))
for _c, _m in _CASE.items():
    BOUNDS[_c] = {k: 2 * _m.get(k, 0) for k in BOUNDS['all']}


def _lib():
    return host_lib('weather_host', ('odr_weather.hip.h',))


def ulps(a, b):
    """Distance of two float64 arrays in units in the last place (0 where both are the same value, NaN with NaN included)."""
    a, b = np.ascontiguousarray(a, np.float64).ravel(), np.ascontiguousarray(b, np.float64).ravel()
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.iinfo(np.int64).min - ia[ia < 0]
    ib[ib < 0] = np.iinfo(np.int64).min - ib[ib < 0]
    d = np.abs(ia - ib).astype(np.float64)      # (exact while the two have the same sign, as masses and fractions do)
    d[np.isnan(a) & np.isnan(b)] = 0
    d[np.isnan(a) != np.isnan(b)] = np.inf
    return d


def flags_of(processes):
    f = 0
    for k in processes:
        f |= _abi.WEATHER[k]
    return f


def step(oil, rho_w, processes, dt, env, z, age, state, mc):
    """One odr_oil_weather call on the host.  env: {xwind, ywind, temp, hs, tp} float32; state: {name: float64 [n]} for the names of
    _abi.WEATHER_RECORD; mc [n, ncomp].  Returns (state, mc, reduction {name: value}, temperature in Kelvin)."""
    n = len(z)
    t = weathering_table(oil, rho_w)
    rec = np.zeros((n, _abi.WEATHER_RECORD_N))
    for k, name in enumerate(REC):
        rec[:, k] = state[name]
    rows = np.array(mc, dtype=np.float64, order='C')
    assert rows.shape == (n, t.ncomp)
    e = [np.ascontiguousarray(env[k], np.float32) for k in ENV]
    zz, aa = np.ascontiguousarray(z, np.float64), np.ascontiguousarray(age, np.float64)
    red, tk = np.zeros(8), np.zeros(n, np.float32)
    _lib().weatherh_step(C.c_longlong(n), C.byref(t), C.c_int(flags_of(processes)), C.c_double(dt), *[a.ctypes.data_as(_fp) for a in e],
                         zz.ctypes.data_as(_dp), aa.ctypes.data_as(_dp), rec.ctypes.data_as(_dp), rows.ctypes.data_as(_dp),
                         red.ctypes.data_as(_dp), tk.ctypes.data_as(_fp))
    return {name: rec[:, k].copy() for k, name in enumerate(REC)}, rows, dict(zip(_abi.WEATHER_REDUCTION, red)), tk


def row_sums(a):
    a = np.ascontiguousarray(a, np.float64)
    out = np.zeros(a.shape[0])
    _lib().weatherh_row_sums(C.c_longlong(a.shape[0]), C.c_int(a.shape[1]), a.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    return out


def mass_transport(ws):
    """noaa.mass_transport_coeff as the launch forms it, float32."""
    ws = np.ascontiguousarray(ws, np.float32)
    out = np.zeros(ws.size, np.float32)
    _lib().weatherh_mass_transport(C.c_longlong(ws.size), ws.ctypes.data_as(_fp), out.ctypes.data_as(_fp))
    return out


def adcroft_fraction(temp_k, dt):
    """fraction_biodegraded of biodegradation_adcroft as the launch forms it, float32."""
    t = np.ascontiguousarray(temp_k, np.float32)
    out = np.zeros(t.size, np.float32)
    _lib().weatherh_adcroft_fraction(C.c_longlong(t.size), t.ctypes.data_as(_fp), C.c_double(dt), out.ctypes.data_as(_fp))
    return out


class Golden:
    """C39 as the launches see it."""
    CASES = 'abcd'

    def __init__(self):
        self.G = np.load(GOLDEN)

    def g(self, case, name):
        return self.G[case + '_' + name]

    def steps(self, case):
        return len(self.g(case, 's0_present'))

    def steps_of_run(self, case):
        return len(self.g(case, 'end_status'))

    def dt(self, case):
        return float(self.g(case, 'dt'))

    def rho_w(self, case):
        return float(self.g(case, 'sea_water_density'))

    def oil(self, case):
        keys = ('mass_fraction', 'boiling_point', 'molecular_weight', 'density', 'density_ref_temp', 'density_k', 'viscosity',
                'viscosity_ref_temp', 'viscosity_B', 'bullwinkle_fraction', 'bullwinkle_time', 'emulsion_water_fraction_max',
                'oil_water_interfacial_tension')
        oil = {k: (self.g(case, 'oil_' + k).tolist()) for k in keys}
        if oil['bullwinkle_time'] != oil['bullwinkle_time']:
            oil['bullwinkle_time'] = None
        if case + '_mwf_temperatures' in self.G.files:
            oil['max_water_fraction'] = {'temperatures': self.g(case, 'mwf_temperatures').tolist(),
                                         'max_water_fraction': self.g(case, 'mwf_max_water_fraction').tolist()}
        return oil

    def processes(self, case):
        """The names of the processes of the case in the reference's order, biodegradation as its method."""
        out = [k for k in ('evaporation', 'emulsification', 'dispersion') if bool(self.g(case, 'process_' + k))]
        if bool(self.g(case, 'process_biodegradation')):
            out.append(str(self.g(case, 'method')))
        return out

    def present(self, case, s):
        return np.flatnonzero(self.g(case, 's0_present')[s])

    def _stage_prefix(self, process):
        return {'properties': 'p', 'evaporation': 'e', 'emulsification': 'm', 'dispersion': 'd', 'half_time': 'b', 'Adcroft': 'b'}[process]

    def mc(self, case, s, behind):
        """mass_components [n_total, ncomp] behind the stage `behind` of step s (None: in front of the step)."""
        with_mc = [q for q in (self._stage_prefix(p) for p in self.processes(case)) if q != 'm']
        if behind is not None:
            upto = [q for q in with_mc if 'pemdb'.index(q) <= 'pemdb'.index(behind)]
            if upto:
                return self.g(case, upto[-1] + '_mc')[s]
        return self.g(case, 'mc_init') if s == 0 else self.g(case, with_mc[-1] + '_mc')[s - 1]

    def state(self, case, s, behind):
        """{name: [n_total]} behind the stage `behind` ('p', 'e', 'm', 'd', 'b') of step s, None: in front of the step."""
        st = {k: np.array(self.g(case, 's0_' + k)[s]) for k in REC}
        if behind is None:
            return st
        ran = ['p'] + [self._stage_prefix(p) for p in self.processes(case)]
        for prefix, _, names in STAGES:
            if prefix in ran:
                for k in names:
                    st[k] = np.array(self.g(case, prefix + '_' + k)[s])
            if prefix == behind:
                break
        return st

    def inputs(self, case, s):
        """(ids, env, z, age) of the elements present in step s."""
        ids = self.present(case, s)
        env = {k: self.g(case, 's0_env_' + k)[s][ids] for k in ENV}
        # the reference takes the period from the second-moment variable it derives from the wind and stores as float32 when no reader
        # delivers one (physics_methods.py:876-883): the device has no such variable and derives the same value
        assert np.nanmax(self.g(case, 's0_env_tp')) == 0
        return ids, env, self.g(case, 's0_z')[s][ids], self.g(case, 's0_age_seconds')[s][ids]
