"""Concurrency of env-kernel launches in a rocprofv3 kernel trace: for the env kernels, the queue each ran on,
their durations, and how much of their summed duration overlapped another env launch; then, per queue that ran
env launches, the chain it executed inside the collection window (first env start to last env end): env and
inference launch counts and mean durations, the mean gap from an env launch's end to the next inference launch's
start and from that launch's end to the next env launch's start, and the share of the window the queue was busy.

usage: python tools/trace_overlap.py <kernel_trace.csv>
"""
import csv
import sys
from collections import Counter, defaultdict

allrows = list(csv.DictReader(open(sys.argv[1])))
rows = [r for r in allrows if "env_kernel" in r["Kernel_Name"]]
if rows:
    print("columns:", list(rows[0].keys()))
grid_key = next((k for k in (rows[0].keys() if rows else []) if k.startswith("Grid_Size")), None)
iv = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", r.get("Stream_Id", "?")),
             int(r[grid_key]) if grid_key else 0) for r in rows)
print(len(iv), "env launches; queues:", Counter(q for _, _, q, _ in iv).most_common(), "grids:", Counter(g for *_, g in iv))
tot = sum(e - s for s, e, *_ in iv)
# time covered by at least one env launch vs summed durations
cover, cur_s, cur_e = 0, None, None
for s, e, *_ in iv:
    if cur_e is None or s > cur_e:
        if cur_e is not None:
            cover += cur_e - cur_s
        cur_s, cur_e = s, e
    else:
        cur_e = max(cur_e, e)
cover += cur_e - cur_s
print(f"summed env-launch time {tot / 1e6:.2f} ms, covered {cover / 1e6:.2f} ms -> mean concurrency {tot / cover:.2f}")
other = [r for r in allrows if "mlp_infer" in r["Kernel_Name"]]
print(len(other), "inference launches, mean", sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in other) / max(1, len(other)) / 1e3, "us",
      "queues:", Counter(r.get("Queue_Id", "?") for r in other).most_common())

# the chains: per env queue, inside the window of the most common env grid (the collection's launches)
main_grid = Counter(g for *_, g in iv).most_common(1)[0][0]
w0 = min(s for s, _, _, g in iv if g == main_grid)
w1 = max(e for _, e, _, g in iv if g == main_grid)
print(f"collection window {(w1 - w0) / 1e6:.2f} ms (env grid {main_grid})")
per = defaultdict(list)
for r in allrows:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if s >= w0 and e <= w1:
        kind = "env" if "env_kernel" in r["Kernel_Name"] else "infer" if "mlp_infer" in r["Kernel_Name"] else "other"
        per[r.get("Queue_Id", "?")].append((s, e, kind))
for q in sorted(per):
    ks = sorted(per[q])
    if not any(k == "env" for *_, k in ks):
        continue
    dur = defaultdict(list)
    gaps = defaultdict(list)
    for i, (s, e, k) in enumerate(ks):
        dur[k].append(e - s)
        if i:
            gaps[ks[i - 1][2] + ">" + k].append(s - ks[i - 1][1])
    busy = sum(e - s for s, e, _ in ks)
    line = f"queue {q}: busy {busy / (w1 - w0):.3f} of the window;"
    for k in ("env", "infer", "other"):
        if dur[k]:
            line += f" {len(dur[k])} {k} mean {sum(dur[k]) / len(dur[k]) / 1e3:.1f} us;"
    for k in ("env>infer", "infer>env"):
        if gaps[k]:
            line += f" gap {k} mean {sum(gaps[k]) / len(gaps[k]) / 1e3:.1f} us;"
    print(line)
