"""GPU: a plain `OpenOil()` run -- no `weathering_model` -- is bit for bit the run of the commit in front of the oil weathering.

Golden c40 (tools/gen_golden_openoil_plain_run.py) is that commit's run on an MI355X in OpenOil's DEFAULT configuration on the
scenario of golden c14 (tests/openoil_plain_run.py): current uncertainty in the main sample and in every Runge-Kutta stage, wind
uncertainty, Stokes drift, vertical mixing with the oil physics, through the `OpenOil` class itself.  c14's own trajectories cannot
be the yardstick of a model run: `OpenOil.run(rng='numpy')` draws one intrusion number per element and sub-step where the reference
draws them compacted (module docstring of opendrift_amd/openoil.py), so the np.random stream is consumed differently and, at the
default uncertainties, every position depends on it.  The c14 replay with the recorded draws stays where it is
(tests/test_gpu_noise.py, tests/test_gpu_stage_math.py)."""
import numpy as np
import pytest

import openoil_plain_run as R
from conftest import golden
from opendrift_amd import readers
from opendrift_amd._abi import OdrError
from opendrift_amd.openoil import OpenOil

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('rng', R.RNGS)
def test_plain_openoil_run_is_the_run_in_front_of_the_weathering(rng):
    rec = golden('c40_openoil_plain_run.npz')
    o, out = R.plain_run(OpenOil, readers, golden('c14_openoil_defaults.npz'), rng)
    assert sorted(rng + '_' + k for k in out) == sorted(k for k in rec.files if k.startswith(rng + '_'))
    for k, v in out.items():
        exp = rec[rng + '_' + k]
        assert v.dtype == exp.dtype and np.array_equal(v, exp, equal_nan=v.dtype.kind == 'f'), k
    # the run is the one the golden is for: mixing has moved elements both ways, the noise is in
    z0 = golden('c14_openoil_defaults.npz')['z'][0]
    assert ((out['z'] < 0) & (z0 == 0)).sum() >= 5 and ((out['z'] == 0) & (z0 < 0)).sum() >= 5
    # and there is no weathering state: no table, no launch, no oil mass
    with pytest.raises(OdrError, match='no weathering table'):
        o.P.oil_budget(1)
    with pytest.raises(AttributeError):
        o.elements.mass_oil
    with pytest.raises(NotImplementedError):
        o.get_oil_budget()
    o.P.close()


def test_the_two_random_number_modes_differ():
    """(or the recording would hold one run twice)"""
    rec = golden('c40_openoil_plain_run.npz')
    assert not np.array_equal(rec['device_lon'], rec['numpy_lon'])
