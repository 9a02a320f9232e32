"""A sharded run issues the same collectives in the same order on every rank, whatever the number of elements a rank holds:
a rank whose elements are all gone goes on taking part (or the other ranks wait in a collective it never enters).  CPU test:
the collectives of opendrift_amd.distributed are recorded, the device particle set is a stand-in.

The step's other collectives are gated by rank-invariant inputs only: _global_counts / _step_summary / _global_scan run on every
rank (_resolve_status scans an empty set as flags 0), _with_global_reduction and the movers' early-outs test the global active
count (_g_active) or readers / fallbacks, report_missing_variables calls odr_deactivate_missing on every rank when sharded."""
from types import SimpleNamespace

import numpy as np
import pytest

from opendrift_amd import distributed as D
from opendrift_amd.oceandrift import OceanDrift


class _Particles:
    """Particles stand-in: n active elements, the deepest at `deepest` m."""

    def __init__(self, n, deepest):
        self.n, self.deepest = n, deepest

    def __len__(self):
        return self.n

    def reduce_local(self, wind_drift_depth=0.1, relative_wind=False):
        raw = np.zeros(16)
        raw[0] = self.n
        raw[5] = self.deepest if self.n else -np.inf      # max(-z) over no element
        return raw


@pytest.fixture()
def recorded(monkeypatch):
    calls = []

    def rec(name, result):
        def f(values, *a, **kw):
            calls.append((name, len(values)) + a + tuple(sorted(kw.items())))
            return result(values)
        return f

    # every rank but this one has an element 120 m down
    monkeypatch.setattr(D, 'allreduce_scalars', rec('allreduce_scalars', lambda v: np.maximum(np.asarray(v, float), 120.0)))
    monkeypatch.setattr(D, 'allgather_vector', rec('allgather_vector', lambda v: np.vstack([v, v])))
    monkeypatch.setattr(D, 'start_allgather_vector', rec('start_allgather_vector', lambda v: None))
    monkeypatch.setattr(D, 'barrier', lambda *a, **kw: calls.append(('barrier',)))
    return calls


def _model(n, deepest):
    """A two-rank model with drift:truncate_ocean_model_below_m and a reader that hands out K profiles on 8 z levels."""
    o = OceanDrift.__new__(OceanDrift)
    o._config = {'drift:truncate_ocean_model_below_m': {'value': 40.0}, 'drift:profiles_depth': {'value': 50.0}}
    reader = SimpleNamespace(z=np.array([0.0, -5, -10, -20, -30, -50, -75, -100]), verticalbuffer=1)
    o.readers = {'k': SimpleNamespace(sid=0, reader=reader)}
    o.priority_list = {'ocean_vertical_diffusivity': ['k']}
    o._world, o._rank = 2, 1
    o._timing_collectives = 0
    o.P = _Particles(n, deepest)
    return o


def test_profile_level_cut_issues_the_same_collectives_with_and_without_elements(recorded):
    with_elements = _model(500, 10.0)
    cut_full = with_elements._profile_level_cut()
    seq_full = list(recorded)
    del recorded[:]
    empty = _model(0, 0.0)
    cut_empty = empty._profile_level_cut()
    seq_empty = list(recorded)
    assert seq_full == [('allreduce_scalars', 1, 'max')]
    assert seq_empty == seq_full
    assert empty._timing_collectives == with_elements._timing_collectives == 1
    # both ranks use the all-rank depth (120 m -> truncated at 40 m: the block ends one level and the buffer below -50 m)
    assert cut_empty == cut_full == 7


def test_profile_level_cut_without_truncation_or_profiles_makes_no_collective(recorded):
    o = _model(0, 0.0)
    o._config['drift:truncate_ocean_model_below_m'] = {'value': None}
    assert o._profile_level_cut() == 0
    o = _model(0, 0.0)
    o.readers['k'].reader.always_delivers_all_levels = True
    assert o._profile_level_cut() == 0
    assert recorded == []


def test_one_process_run_makes_no_collective(recorded):
    o = _model(0, 0.0)
    o._world = 1
    o._profile_level_cut()
    assert recorded == [] and o._timing_collectives == 0
