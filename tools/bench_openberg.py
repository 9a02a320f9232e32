"""Milliseconds per OpenBerg model step and solver attempts per step at 1 M bergs on C28-shaped fields (the population and the
fields of tools/gen_golden_openberg.py, tiled).  The tool does not split the time into prepare, attempts, reduction read-back and
finish itself:

    python tools/bench_openberg.py [--n 1000000] [--steps 3]

the split comes from the library's own kernel timeline: run it under `rocprofv3 --kernel-trace --stats -- python
tools/bench_openberg.py` for the per-kernel times (k_berg_prepare, k_berg_attempt, k_berg_fold, k_berg_finish); the host-side
figure printed here is wall time per call and, from it and the attempt count, the time per attempt including its read-back.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from opendrift_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--steps', type=int, default=3)
    a = ap.parse_args()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'c28_openberg.npz'))
    m = g['grounded'][1] >= 0
    reps = -(-a.n // int(m.sum()))
    tile = lambda v: np.ascontiguousarray(np.tile(v[m], reps)[:a.n])      # noqa: E731
    ctx = Context(device=0, seed=0)
    P = ctx.particles(a.n)
    P.append(np.linspace(20, 24, a.n), tile(g['adv_lat'][1]), z=np.zeros(a.n), moving=tile(g['moving_before'][1]).astype(np.int32))
    import berg_host
    for k in berg_host.ENV:
        P.env_upload(k, tile(g['env_' + k][1]))
    for slot, k in enumerate(('sail', 'draft', 'length', 'width')):
        P.set_property(slot, tile(g[k + '_before'][1]))
    P.berg_roll_over()
    P.berg_advect(3600.0, wave_from_direction=200.0, sea_ice_thickness=1.0)      # warm-up: scratch allocation
    ctx.sync()
    ms, att = [], []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        P.berg_roll_over()
        na, nr = P.berg_advect(3600.0, wave_from_direction=200.0, sea_ice_thickness=1.0)
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
        att.append((na, nr))
    print(json.dumps(dict(n=a.n, ms_per_step=ms, attempts=att, ms_per_attempt_with_readback=[t / max(1, n_[0]) for t, n_ in zip(ms, att)])))
    P.close()
    ctx.close()


if __name__ == '__main__':
    main()
