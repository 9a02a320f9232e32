"""Per-dispatch kernel times of the mixing launches from a rocprofv3 kernel trace: the whole-run average and the mean of the LAST
N dispatches (a plain bench.py run times its last 400 steps, so the last 400 mixing dispatches are the timed window) of

    mixing      k_vmix_col / k_vmix_dense (every instantiation), and split by instantiation
    keep        k_vmix_keep        keep_scan   k_vmix_keep_scan        keep_fill   k_vmix_keep_fill
    step        k_step_grid (every instantiation)

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python bench.py --gpus 1
    python tools/vmix_dispatch_times.py OUT/**/*_kernel_trace.csv [--last 400]
"""
import argparse
import csv
import re
from collections import defaultdict

GROUPS = [('mixing', r'k_vmix_(col|dense)<'), ('keep', r'k_vmix_keep\('), ('keep_scan', r'k_vmix_keep_scan\('),
          ('keep_fill', r'k_vmix_keep_fill\('), ('step', r'k_step_grid<')]


def rows(path):
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            yield r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace', nargs='+')
    ap.add_argument('--last', type=int, default=400)
    a = ap.parse_args()
    found = defaultdict(list)
    for path in a.trace:
        for name, t0, t1 in rows(path):
            for g, pat in GROUPS:
                if re.search(pat, name):
                    found[g].append((t0, (t1 - t0) * 1e-3, name))
    print('%-12s %8s %12s %12s   (us; last = the last %d dispatches of the group)' % ('group', 'calls', 'avg_all', 'avg_last', a.last))
    for g, _ in GROUPS:
        d = sorted(found[g])
        if not d:     # (k_vmix_keep: absent where the step launch left the keep ballots)
            print('%-12s %8d %12s %12s' % (g, 0, '-', '-'))
            continue
        last = d[-a.last:]
        print('%-12s %8d %12.1f %12.1f' % (g, len(d), sum(x[1] for x in d) / len(d), sum(x[1] for x in last) / len(last)))
        if g == 'mixing':
            by = defaultdict(list)
            for _, us, name in last:
                by[re.sub(r'\(.*', '', name)].append(us)
            for name, v in sorted(by.items()):
                print('  last: %-60s %6d %10.1f' % (name[:60], len(v), sum(v) / len(v)))


if __name__ == '__main__':
    main()
