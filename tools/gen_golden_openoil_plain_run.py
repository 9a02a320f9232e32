"""Records tests/golden/c40_openoil_plain_run.npz: a plain `OpenOil()` run (no `weathering_model`) in its default configuration on
the scenario of golden c14 (tests/openoil_plain_run.py), with both random-number modes.  It is a recording of THIS project's run,
made on an MI355X with the tree of the commit in front of the oil weathering, so that tests/test_gpu_openoil_plain_run.py can hold
every later commit to those bits: the plain model must not change when weathering is added.

    python tools/gen_golden_openoil_plain_run.py [--package-root TREE] [--out FILE]

TREE is a built checkout of the commit to record (default: this one).  Every run is made twice and must repeat bit for bit."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--package-root', default=ROOT)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'c40_openoil_plain_run.npz'))
    a = ap.parse_args()
    tree = os.path.abspath(a.package_root)
    sys.path[:0] = [tree, os.path.join(ROOT, 'tests')]
    readers = importlib.import_module('opendrift_amd.readers')
    OpenOil = importlib.import_module('opendrift_amd.openoil').OpenOil
    assert os.path.dirname(os.path.dirname(os.path.abspath(readers.__file__))) == tree, readers.__file__
    import openoil_plain_run as R
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'c14_openoil_defaults.npz'))
    out = {}
    for rng in R.RNGS:
        runs = []
        for _ in range(2):
            o, r = R.plain_run(OpenOil, readers, g, rng)
            o.P.close()
            runs.append(r)
        for k in runs[0]:
            assert np.array_equal(runs[0][k], runs[1][k], equal_nan=runs[0][k].dtype.kind == 'f'), (rng, k)
            out[rng + '_' + k] = runs[0][k]
        z = runs[0]['z']
        print(rng, 'at the surface at the end', int((z == 0).sum()), 'of', len(z), 'deepest', float(np.nanmin(z)),
              'statuses', list(runs[0]['categories']))
    np.savez_compressed(a.out, **out)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
