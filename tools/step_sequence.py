#!/usr/bin/env python3
"""The kernels of ONE warm step in dispatch order, from a rocprofv3 --kernel-trace CSV: name (shortened), duration, gap to the
previous kernel's end (negative: the kernel began while the previous one was still running -- the grouped forward's two streams).
The last complete step is taken: the trace is cut at launches of MARKER (default pack_input_kernel, the first kernel of a forward);
PER_STEP (default 1) is the number of MARKER launches in a step, 2 for a forward of two image groups.  With more than one queue in
the step every row also names its queue, and `busy` is the time at least one kernel was running.
usage: step_sequence.py TRACE_DIR [MARKER [PER_STEP]]"""
import csv, glob, os, re, sys

root = sys.argv[1]
marker = sys.argv[2] if len(sys.argv) > 2 else "pack_input_kernel"
per_step = int(sys.argv[3]) if len(sys.argv) > 3 else 1
f = max(glob.glob(f"{root}/**/*kernel_trace.csv", recursive=True), key=os.path.getmtime)
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
starts = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
if len(starts) < 2 * per_step:
    sys.exit(f"marker {marker} seen {len(starts)} times")
seq = rows[starts[-2 * per_step]:starts[-per_step]]
t0 = int(seq[0]["Start_Timestamp"])
queues = sorted({r.get("Queue_Id", "") for r in seq})
prev_end, busy = None, 0
for r in seq:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("mgu::", "").replace("(anonymous namespace)::", "")
    gap = (s - prev_end) / 1e3 if prev_end is not None else 0.0
    q = f"  q{queues.index(r.get('Queue_Id', ''))}" if len(queues) > 1 else ""
    print(f"{(s - t0) / 1e3:9.1f} us  {(e - s) / 1e3:8.2f} us  gap {gap:6.2f}{q}  {name[:80]}")
    busy += e - s if prev_end is None else max(0, e - max(s, prev_end))
    prev_end = e if prev_end is None else max(prev_end, e)
print(f"step span {(prev_end - t0) / 1e3:.1f} us, busy {busy / 1e3:.1f} us, {len(seq)} kernels")
