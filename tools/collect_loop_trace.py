"""The collection phase of the last iteration in a rocprofv3 kernel-trace CSV of bench.py: every env_collect launch
(the collection loop, one per iteration) with its duration, and what ran between the last one's start and end -- it
must be alone there: no env_kernel and no mlp_infer launches -- then the kernels of the whole trace by summed time.

usage: python tools/collect_loop_trace.py <kernel_trace.csv>
"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
iv = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows]
loops = [x for x in iv if "env_collect" in x[2]]
print(f"{len(iv)} kernel launches in the trace; env_collect launches: {len(loops)}")
for s, e, k in loops:
    print(f"  env_collect: {(e - s) / 1e6:8.3f} ms")
if not loops:
    sys.exit("no env_collect launch in the trace")
s0, e0, _ = loops[-1]
inside = collections.Counter(k[:60] for s, e, k in iv if s < e0 and e > s0)
print("launches overlapping the last env_collect launch:", dict(inside))
for pat in ("env_kernel", "mlp_infer"):
    n = sum(1 for s, e, k in iv if s < e0 and e > s0 and pat in k)
    print(f"  {pat} launches inside the collection: {n}")
agg = collections.defaultdict(lambda: [0, 0.0])
for s, e, k in iv:
    agg[k[:70]][0] += 1
    agg[k[:70]][1] += (e - s) / 1e6
print("kernels by summed time (whole trace):")
for k, (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:12]:
    print(f"  n={n:5d} {ms:9.3f} ms  {k}")
