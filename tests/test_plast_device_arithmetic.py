"""CPU: the per-element arithmetic of csrc/odr_plast.hip.h, compiled for the host (plast_host.cpp), against what the REFERENCE's
own PlastDrift computed (golden c40_plastdrift.npz, tools/gen_golden_plastdrift.py): the Stokes drift and the wave height behind
get_environment for the three fetches, bit for bit in float32; z behind update_particle_depth from the recorded draws, bit for bit
in float64 (the precision the particle set holds z at, and the reference's behind that call).  DESIGN.md section 7j."""
import json
import os

import numpy as np
import pytest

from conftest import golden

import plast_host

FETCH_OF = {'a': '25000', 'b5': '5000', 'b50': '50000'}


def tables():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stokes_tables.json')) as fh:
        return json.load(fh)


def environment_case(g, case):
    """x_wind, y_wind and the reference's Stokes x / y / wave height of every (step, element) present, flattened."""
    ok = np.isfinite(g[case + '_xw'])
    return tuple(g['%s_%s' % (case, k)][ok] for k in ('xw', 'yw', 'sx', 'sy', 'hs'))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and np.array_equal(a.view('u%d' % a.dtype.itemsize), b.view('u%d' % b.dtype.itemsize))


@pytest.mark.parametrize('case', sorted(FETCH_OF))
def test_stokes_drift_and_wave_height_reproduce_the_reference_bit_for_bit(case):
    g = golden('c40_plastdrift.npz')
    xw, yw, sx, sy, hs = environment_case(g, case)
    t = tables()[FETCH_OF[case]]
    assert len(t['stokes']) == (4 if case == 'b5' else 7) and len(t['hs']) == 2
    speed = np.hypot(xw.astype(np.float64), yw)
    assert (speed > 30).sum() >= 10 and (speed < 30).sum() >= 10 and (speed == 0).sum() >= 3      # both sides of the cap, and calm
    gx, gy, gh = plast_host.stokes_from_wind(xw, yw, t['stokes'], t['hs'])
    assert sx.dtype == np.float32 and same_bits(gx, sx) and same_bits(gy, sy) and same_bits(gh, hs)
    assert (gx[speed == 0] == 0).all() and (gh[speed == 0] == np.float32(t['hs'][1])).all()


def test_wind_speed_is_capped_at_30():
    t = tables()['25000']
    a = plast_host.stokes_from_wind(np.float32([30, 50, 0, 24]), np.float32([0, 0, 40, 18]), t['stokes'], t['hs'])
    assert a[2][0] == a[2][1] == a[2][2] == a[2][3]                     # the wave height depends on the capped speed only
    assert abs(a[0][1] / a[0][0] - 50 / 30) < 1e-6                      # ... and the drift is the uncapped component times the factor
    assert np.isnan(plast_host.stokes_from_wind(np.float32([np.nan]), np.float32([1]), t['stokes'], t['hs'])[2][0])


@pytest.mark.parametrize('case', ['a', 'd'])
def test_depth_from_the_recorded_draws_is_the_reference_s_bit_for_bit(case):
    g = golden('c40_plastdrift.npz')
    K, E, zd = g[case + '_K'], g[case + '_E'], g[case + '_zd']
    w = np.broadcast_to(g[case + '_tv'], K.shape)
    ok = np.isfinite(E)
    assert ok.sum() >= 8 * 50 and zd.dtype == np.float64 and K.dtype == np.float32 and w.dtype == np.float32
    z, refused = plast_host.depth(K[ok], w[ok], E[ok])
    assert not refused and same_bits(z, zd[ok])
    if case == 'a':
        assert (-z).max() / (-z)[z < 0].min() > 100          # more than two decades of depth


def test_scales_numpy_refuses_and_the_edges():
    E = np.array([0.5, 1.5, 2.5])
    before = np.array([-1.0, -2.0, -3.0])
    z, refused = plast_host.depth([0.02, 0.02, 0.02], [0.01, -0.01, 0.01], E, before)      # a sinking element
    assert refused and np.array_equal(z, before)
    z, refused = plast_host.depth([0.0, 0.02, 0.02], [-0.01, 0.01, 0.01], E, before)       # -0.0: NumPy looks at the sign bit
    assert refused and np.array_equal(z, before)
    z, refused = plast_host.depth([0.0, 0.0, 0.02], [0.01, 0.0, 0.0], E, before)            # K = 0: -0.0; 0 / 0: NaN; K / 0: -inf
    assert not refused and z[0] == 0 and np.signbit(z[0]) and np.isnan(z[1]) and z[2] == -np.inf
    for K, w in (([0.02], [-0.01]), ([0.0], [-0.01])):                                      # what NumPy itself says
        with pytest.raises(ValueError, match='scale < 0'):
            np.random.exponential(scale=np.float32(K) / np.float32(w), size=1)
