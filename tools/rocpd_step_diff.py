"""Per-step kernel table from two rocprofv3 (rocpd SQLite) kernel traces of the same program that differ only in the number of
timed steps: everything outside the steps (imports, set-up, warm-up, packing) cancels, and the difference divided by the extra
steps is what ONE step dispatches.

usage: python tools/rocpd_step_diff.py short/pt_results.db long/pt_results.db <extra steps> > profiles/<name>.txt"""
import re
import sqlite3
import sys


def load(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    nc = 'name' if 'name' in cols else [c for c in cols if 'name' in c][0]
    return {r[0]: (r[1], r[2]) for r in db.execute(f"select {nc}, count(*), sum(end-start) from kernels group by {nc}")}


def main(short, long, steps):
    a, b = load(short), load(long)
    rows = []
    for k in set(a) | set(b):
        c = b.get(k, (0, 0))[0] - a.get(k, (0, 0))[0]
        t_us = (b.get(k, (0, 0))[1] - a.get(k, (0, 0))[1]) / steps / 1e3       # timestamps in ns
        if c:
            rows.append((t_us, c / steps, k))
    rows.sort(reverse=True)
    tot_c, tot_t = sum(r[1] for r in rows), sum(r[0] for r in rows)
    print(f'dispatches per step: {tot_c:.1f}; summed kernel time per step: {tot_t / 1e3:.3f} ms')
    print(f"{'kernel':100s} {'per_step':>8s} {'us/step':>9s} {'%':>6s}")
    for t, c, k in rows:
        k = re.sub(r'\(anonymous namespace\)::', '', k)
        k = k if len(k) <= 100 else k[:97] + '...'
        print(f'{k:100s} {c:8.2f} {t:9.1f} {100 * t / tot_t:6.2f}')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]))
