"""MI355X: how many elements the two-quad mixing launch (csrc/odr_kernels.hip.h VMixC3W) redoes on the whole column over a C3
run of bench.py's size -- 10 M elements, 48 steps, the full-size field -- from odr_particles_vmix_window_stats.

  python tools/vmix_redo_count.py [elements] [steps]"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from opendrift_amd.device import Context

if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    fields = bench.make_fields('c3')
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    wl = bench.Workload('c3', ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles('c3', fields, n, np.random.default_rng(1000))
    P = ctx.particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    for k in range(steps):
        wl.step(P, k)
    s = P.vmix_window_stats()
    print('C3, %d elements, %d steps: two-quad launches %d, whole-column static launches %d, elements redone %d (%.3g of the '
          'element-steps)' % (n, steps, s['windowed'], s['full'], s['redone'], s['redone'] / float(n * steps)))
    P.close()
    ctx.close()
