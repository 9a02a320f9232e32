"""GPU: what a plain `bench.py` run prints and what `--full` adds.  A plain run measures the headline alone; `--full` runs the
other legs after the headline's steps and its dump, so both leave the same particle state behind (C3, small block)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('roofline', 'roofline_algorithmic', 'stage_math_exact', 'lds_tile', 'cpu_baseline', 'model_api', 'pcie_inclusive')


def _bench(args, dump):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'c3', '--small', '--particles', '200000',
           '--steps', '8', '--warmup', '2', '--dump-outputs', dump] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_full_adds_the_legs(tmp_path):
    plain = _bench([], str(tmp_path / 'plain'))
    for k in HEADLINE:
        assert k in plain, k
    assert plain['steps'] == 8 and plain['warmup'] == 2 and plain['value'] > 0 and plain['ms_per_step'] > 0
    assert not [k for k in FULL_ONLY if k in plain]
    full = _bench(['--full', '--no-cpu'], str(tmp_path / 'full'))
    for k in HEADLINE:
        assert k in full, k
    assert full['roofline']['kernel_ms'] > 0 and full['roofline']['second_kernel']['kernel_ms'] > 0
    assert full['stage_math_exact']['ms_per_step'] > 0 and 'launches' in full['lds_tile']
    assert 'cpu_baseline' not in full and 'model_api' not in full      # --no-cpu; the small block has no model_api leg
    assert {k: plain[k] for k in ('metric', 'unit', 'dtype', 'config')} == {k: full[k] for k in ('metric', 'unit', 'dtype', 'config')}
    # the legs of --full come after the dump: the state the timed steps left is the same with and without them
    names = sorted(os.listdir(tmp_path / 'plain'))
    assert names == sorted(os.listdir(tmp_path / 'full')) and 'lon.npy' in names
    for f in names:
        a, b = np.load(tmp_path / 'plain' / f), np.load(tmp_path / 'full' / f)
        assert np.array_equal(a, b, equal_nan=True), f
