#!/usr/bin/env python3
"""Per dispatch of a steady-state call: tools/call_trace.py KERNEL_TRACE.csv [min_headline_us]

Reads the per-dispatch CSV of `rocprofv3 --kernel-trace` (the runtime's fills and copies included), takes the classify kernels of at least
min_headline_us (default 1000) as the calls' headline kernels, and cuts the trace into windows from one headline kernel's start to the
next one's.  The windows with the most frequent sequence of kernel names are the steady state; per position of that sequence it prints the
average duration, the average start relative to the window's headline kernel's start and end, and the average idle time in front of the
dispatch (its start minus the latest end of everything before it; negative: it started while something else ran)."""
import collections
import csv
import re
import sys


def short(name):
    name = re.sub(r"^void ", "", name)
    name = name.replace("shk::", "")
    m = re.match(r"([A-Za-z_0-9]+(<[^(]*>)?)", name)
    return (m.group(1) if m else name)[:100]


def main():
    path = sys.argv[1]
    min_us = float(sys.argv[2]) if len(sys.argv) > 2 else 1000.0
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]),
                         int(r.get("Workgroup_Size") or r.get("Workgroup_Size_X") or 0), int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0), r.get("Queue_Id", "")))
    rows.sort()
    heads = [i for i, r in enumerate(rows) if r[2].startswith("classify_") and (r[1] - r[0]) >= min_us * 1000.0]
    windows = collections.defaultdict(list)
    for a, b in zip(heads, heads[1:]):
        windows[tuple(r[2] for r in rows[a:b])].append((a, b))
    if not windows:
        print("no headline kernel found")
        return
    seq, wins = max(windows.items(), key=lambda kv: len(kv[1]))
    print("%d dispatches, %d headline kernels, %d distinct window sequences; steady state: %d windows of %d dispatches" %
          (len(rows), len(heads), len(windows), len(wins), len(seq)))
    period = sum(rows[b][0] - rows[a][0] for a, b in wins) / len(wins) / 1000.0
    print("start to start of the headline kernel: %.2f us" % period)
    print("%3s %-100s %10s %12s %12s %10s %8s %10s %s" % ("#", "kernel", "avg us", "from start", "from end", "idle us", "wg", "grid", "queue"))
    total_other = 0.0
    for pos in range(len(seq)):
        dur = off_s = off_e = idle = 0.0
        queues = set()
        for a, b in wins:
            r = rows[a + pos]
            dur += r[1] - r[0]
            off_s += r[0] - rows[a][0]
            off_e += r[0] - rows[a][1]
            # (the latest end among the dispatches in front: the eight before it are enough, a call has thirteen dispatches at most and only
            #  the check of a speculated batch runs beside another one; the trace's very first dispatch has nothing in front)
            if a + pos:
                idle += r[0] - max(x[1] for x in rows[max(0, a + pos - 8):a + pos])
            queues.add(r[5])
        k = len(wins) * 1000.0
        r = rows[wins[0][0] + pos]
        if pos:
            total_other += dur / k
        print("%3d %-100s %10.2f %12.2f %12.2f %10.2f %8d %10d %s" % (pos, seq[pos], dur / k, off_s / k, off_e / k, idle / k, r[3], r[4], ",".join(sorted(queues))))
    print("sum of the durations outside the headline kernel: %.2f us" % total_other)


if __name__ == "__main__":
    main()
