"""MI355X: the share of elements at the surface (z == 0) in front of steps 203, 303, 403, 503 and 603 of a C3 run of bench.py's
size -- 10 M elements, the full-size field, bench.Workload('c3').step -- i.e. over the timed window of a plain benchmark run and
beyond; and what the tiled mixing launch (csrc/odr_kernels.hip.h k_vmix_col) skipped over the steps in between, from
odr_particles_vmix_skip_stats.

  python tools/vmix_surface_share.py [elements] [last step]"""
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from opendrift_amd.device import Context

if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 603
    marks = [k for k in (203, 303, 403, 503, 603) if k <= last]
    fields = bench.make_fields('c3')
    ctx = Context(0, seed=0)
    ctx.set_stage_math('fast')
    wl = bench.Workload('c3', ctx, fields, (0, 0, 1), via_torch=False)
    lon, lat, z = bench.seed_particles('c3', fields, n, np.random.default_rng(1000))
    P = ctx.particles(n)
    P.append(lon, lat, z=z, id=np.arange(n, dtype=np.int32))
    before = P.vmix_skip_stats()
    for k in range(last + 1):
        if k in marks:
            zz = P.download()['z']
            s = P.vmix_skip_stats()
            dl, ds = s['launches'] - before['launches'], s['skipped'] - before['skipped']
            print('C3, %d elements, in front of step %d: %d active, z == 0 for %d (%.4f); since the last mark %d mixing launches '
                  'skipped %d elements (%.4f of their elements)'
                  % (n, k, len(zz), int((zz == 0).sum()), float((zz == 0).mean()), dl, ds, ds / max(1.0, float(dl) * len(zz))),
                  flush=True)
            before = s
        wl.step(P, k)
    P.close()
    ctx.close()
