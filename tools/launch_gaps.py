#!/usr/bin/env python3
"""What the launch boundaries inside one split learn call cost: from a `rocprofv3 --kernel-trace` CSV of the interfrl bench step
(tools/kstats.sh keeps only the --stats table; this needs the trace with its per-dispatch start and end timestamps), per learn call:
the duration of every kernel of the chain from front_kernel to the last finalize, and the gap from its end to the start of the next
dispatch of the chain. Medians over the learn calls of the trace (the first `skip` calls dropped).
usage: tools/launch_gaps.py KERNEL_TRACE_CSV [skip=20]"""
import csv
import statistics
import sys


def short(n):
    n = n.replace("void ", "").replace("avd::fsplit::", "").replace("avd::fset::", "").replace("avd::", "")
    return n.split("(")[0][:48]


def main():
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = list(csv.DictReader(open(sys.argv[1], newline="")))
    col = {k.lower(): k for k in rows[0]}
    rows.sort(key=lambda r: int(r[col["start_timestamp"]]))
    ev = [(r[col["kernel_name"]], int(r[col["start_timestamp"]]), int(r[col["end_timestamp"]])) for r in rows]
    # a learn call: from a front_kernel to the finalize_t1_kernel behind it
    calls, cur = [], None
    for e in ev:
        if "fsplit::front_kernel" in e[0]:
            cur = [e]
        elif cur is not None:
            cur.append(e)
            if "finalize_t1_kernel" in e[0]:
                calls.append(cur)
                cur = None
    calls = calls[skip:]
    shape = [short(e[0]) for e in calls[0]]
    calls = [c for c in calls if [short(e[0]) for e in c] == shape]
    med = statistics.median
    print(f"{len(calls)} learn calls of {len(shape)} launches each; medians in us")
    print(f"{'kernel':50s} {'duration':>9s} {'gap to next':>12s}")
    tot_d = tot_g = 0.0
    for i, name in enumerate(shape):
        d = med((c[i][2] - c[i][1]) / 1e3 for c in calls)
        g = med((c[i + 1][1] - c[i][2]) / 1e3 for c in calls) if i + 1 < len(shape) else 0.0
        tot_d += d
        tot_g += g
        print(f"{name:50s} {d:9.2f} {g:12.2f}")
    span = med((c[-1][2] - c[0][1]) / 1e3 for c in calls)
    print(f"{'sum':50s} {tot_d:9.2f} {tot_g:12.2f}")
    print(f"first start to last end of a learn call: {span:.2f} us")


if __name__ == "__main__":
    main()
