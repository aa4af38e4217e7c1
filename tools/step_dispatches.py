#!/usr/bin/env python3
"""One training step of a `rocprofv3 --kernel-trace` CSV as its dispatches IN ORDER -- what the --stats table cannot show.

    python tools/step_dispatches.py TRACE_kernel_trace.csv [--grep igemm,transpose,splitconv] > step.txt

The steady state of bench.py launches the same kernels in the same order every step, so the trace ends in repetitions of one
period: the tool finds the shortest P with names[-P:] == names[-2P:-P] == names[-3P:-2P], lines the last repetitions up and
prints, per position of the step, the kernel, its grid and the median (min .. max) duration over those steps.  --grep keeps the
positions whose kernel name holds one of the words, with their position numbers, and prints their sum per step."""
import argparse
import csv
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace')
    ap.add_argument('--grep', default='')
    ap.add_argument('--width', type=int, default=96)
    args = ap.parse_args()
    rows = sorted(csv.DictReader(open(args.trace)), key=lambda r: int(r['Start_Timestamp']))
    names = [r['Kernel_Name'] for r in rows]
    dur = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows]
    # what follows the last step (the final reductions, a dump) is not part of the period: drop a tail of up to 2000 dispatches
    period = None
    for drop in range(0, min(2000, len(names) // 4)):
        n = len(names) - drop
        period = next((P for P in range(50, n // 3) if names[n - 1] == names[n - 1 - P] and names[n - P:n] == names[n - 2 * P:n - P] == names[n - 3 * P:n - 2 * P]), None)
        if period is not None:
            break
    if period is None:
        raise SystemExit('no period found: no three consecutive steps launch the same kernels')
    rows, names, dur = rows[:n], names[:n], dur[:n]
    reps = 1
    while (reps + 1) * period <= n and names[n - (reps + 1) * period:n - reps * period] == names[n - period:]:
        reps += 1
    # rotate so that the listing starts where the step does: at the longest idle gap inside the period
    start = n - reps * period
    gaps = [int(rows[start + i]['Start_Timestamp']) - int(rows[start + i - 1]['End_Timestamp']) for i in range(1, period + 1)]
    rot = 1 + max(range(period), key=lambda i: gaps[i])
    if start + rot + (reps - 1) * period > n:
        rot = 0
    reps_used = reps - 1 if rot else reps
    words = [w for w in args.grep.split(',') if w]
    print('# %d dispatches in the trace; a step is %d dispatches; %d steady steps lined up' % (n, period, reps_used))
    total = kept = 0.0
    for i in range(period):
        at = [start + rot + i + k * period for k in range(reps_used)]
        v = [dur[j] for j in at]
        r = rows[at[0]]
        med = statistics.median(v)
        total += med
        if words and not any(w in r['Kernel_Name'] for w in words):
            continue
        kept += med
        grid = 'x'.join(r.get(k, '') for k in ('Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z')) if 'Grid_Size_X' in r else r.get('Grid_Size', '')
        print('%5d  %9.1f us (%8.1f .. %8.1f)  grid %-16s %s' % (i, med, min(v), max(v), grid, r['Kernel_Name'][:args.width]))
    print('# sum of the medians: %.1f us listed, %.1f us per step in all' % (kept if words else total, total))


if __name__ == '__main__':
    main()
