"""GPU: the one check of the property slots a model's entry point is handed (property_slots, csrc/odr_host.h), through one entry
point of each translation unit that uses it (ship_drift has its own cases in tests/test_gpu_shipdrift.py).  Every call here is
refused on the host, before any launch."""
import numpy as np
import pytest

from opendrift_amd._abi import OdrError

pytestmark = pytest.mark.gpu
T, S = 'sea_water_temperature', 'sea_water_salinity'
# entry point -> (the environment variables it wants sampled, the slots of a valid call, the call with those slots)
ENTRY = {
    'egg_terminal_velocity': ((T, S), (0, 1), lambda P, s: P.egg_terminal_velocity(*s)),
    'larval_update': ((T, ), (2, 3, 5, 4), lambda P, s: P.larval_update(600.0, *s)),
    'larvalx_hatch': ((), (0, 1), lambda P, s: P.larvalx_hatch(0.01, *s)),
    'berg_roll_over': ((), (0, 1, 2, 3), lambda P, s: P.berg_roll_over(*s)),
    'radio_terminal_velocity': ((T, S), (0, 2), lambda P, s: P.radio_terminal_velocity(*s)),
}
NEVER_SET = 7


@pytest.mark.parametrize('entry', list(ENTRY))
def test_bad_slots_are_refused_before_any_launch(ctx, entry):
    env, slots, call = ENTRY[entry]
    P = ctx.particles(8)
    P.append(np.linspace(3, 4, 8), np.full(8, 60.0), z=-np.arange(8.0))
    for v in env:
        P.env_upload(v, np.full(8, 8.0, np.float32))
    for k in slots:
        P.set_property(k, np.ones(8, np.float32))
    before = P.download()
    with pytest.raises(ValueError):                     # ODR_ERR_INVALID: no such slot
        call(P, (9, ) + slots[1:])
    with pytest.raises(ValueError):                     # the same slot given twice
        call(P, (slots[1], ) + slots[1:])
    with pytest.raises(OdrError, match='property slot %d ' % NEVER_SET) as e:
        call(P, (NEVER_SET, ) + slots[1:])
    assert e.value.code == -4                           # ODR_ERR_STATE
    after = P.download()
    assert sorted(after) == sorted(before) and len(after['lon']) == 8
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    P.close()
