"""From a rocprofv3 kernel trace CSV: time during which a k_expand_items dispatch overlaps a k_hash_probe or
k_commit_items dispatch, and per-kernel average durations alone and overlapped (chunk look-ahead, DESIGN.md
section 4).  Usage: tools/trace_overlap.py <..._kernel_trace.csv> of
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python bench.py --steps 2 --warmup 1"""
import csv, sys, bisect
path = sys.argv[1]
rows = []
with open(path, newline="") as f:
    r = csv.DictReader(f)
    for x in r:
        rows.append((x["Kernel_Name"], int(x["Start_Timestamp"]), int(x["End_Timestamp"])))
def cls(n):
    if "k_expand_items" in n: return "expand"
    if "k_hash_probe" in n: return "probe"
    if "k_commit_items" in n: return "commit"
    return None
iv = {"expand": [], "probe": [], "commit": []}
for n, s, e in rows:
    c = cls(n)
    if c: iv[c].append((s, e))
for c in iv: iv[c].sort()
def overlap_with(a, others):
    """per interval of a: ns overlapped with the (non-overlapping, sorted) intervals in others"""
    st = [s for s, _ in others]
    out = []
    for s, e in a:
        i = max(bisect.bisect_right(st, s) - 1, 0)
        o = 0
        while i < len(others) and others[i][0] < e:
            o += max(0, min(e, others[i][1]) - max(s, others[i][0]))
            i += 1
        out.append(o)
    return out
pc = sorted(iv["probe"] + iv["commit"])
t0 = min(s for _, s, _ in rows); t1 = max(e for _, _, e in rows)
print("trace", path, "dispatches", len(rows), "span_s", (t1 - t0) / 1e9)
ov = overlap_with(iv["expand"], pc)
print("expand_overlap_with_probe_or_commit_s", sum(ov) / 1e9, "of expand total_s", sum(e - s for s, e in iv["expand"]) / 1e9)
def report(name, a, o):
    al = [e - s for (s, e), x in zip(a, o) if x == 0]
    ovl = [e - s for (s, e), x in zip(a, o) if x > 0]
    f = lambda v: (len(v), round(sum(v) / len(v) / 1e6, 4) if v else None)
    print(name, "alone (n, avg ms)", f(al), "overlapped (n, avg ms)", f(ovl))
report("k_expand_items", iv["expand"], ov)
report("k_hash_probe", iv["probe"], overlap_with(iv["probe"], iv["expand"]))
report("k_commit_items", iv["commit"], overlap_with(iv["commit"], iv["expand"]))
