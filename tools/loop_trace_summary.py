"""The window pass's three launches inside a loop of handles taking turns, from a rocprofv3 --kernel-trace csv
(tools/collect_profiles.sh with PPP_PROFILE_HANDLES=3): per launch kind the duration (mean, standard deviation, min .. max), the
gap from the end of a launch to the start of the next one on the same queue, and how many launches of each kind are in flight
at the moment a per-slice launch starts.  Only passes of the loop's own forms count (a per-slice launch of --slice-threads
threads with the binning and the finish launch around it on the same queue); the launches of plans, warm-up passes alone and
the profile passes are left out by that.
usage: python3 tools/loop_trace_summary.py <dir or kernel_trace.csv> [--slice-threads 512]"""
import csv, glob, os, statistics, sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
slice_t = "512"
if "--slice-threads" in sys.argv:
    slice_t = sys.argv[sys.argv.index("--slice-threads") + 1]
path = args[0]
if os.path.isdir(path):
    found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not found:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    path = found[0]
rows = list(csv.DictReader(open(path)))
if not rows:
    raise SystemExit("%s holds no launches" % path)
qcol = next((c for c in ("Stream_Id", "Queue_Id") if c in rows[0] and len({r[c] for r in rows}) > 1), "Queue_Id")


def kind(name):
    if "k_win_scatter" in name: return "binning"
    if "k_win_slice" in name: return "per-slice"
    if "k_win_finish" in name: return "finish"
    return None


ev = []
for r in rows:
    k = kind(r["Kernel_Name"])
    if k:
        ev.append({"kind": k, "name": r["Kernel_Name"], "q": r[qcol], "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                   "wg": int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", "0")) or 0)})
ev.sort(key=lambda e: e["t0"])
by_q = {}
for e in ev:
    by_q.setdefault(e["q"], []).append(e)
# a pass of the loop: binning, per-slice, finish one behind the other on one queue, the per-slice launch in the loop's form
passes = []
for q, L in by_q.items():
    for i in range(len(L) - 2):
        a, b, c = L[i], L[i + 1], L[i + 2]
        if (a["kind"], b["kind"], c["kind"]) != ("binning", "per-slice", "finish"): continue
        if b["wg"] != int(slice_t) and ("<%s>" % slice_t) not in b["name"]: continue
        nxt = L[i + 3] if i + 3 < len(L) and L[i + 3]["kind"] == "binning" else None
        passes.append((a, b, c, nxt))
# the loop proper: passes that start while a pass on ANOTHER queue is still running (the plans and the passes alone do not)
loop = []
for p in passes:
    t0, t1 = p[0]["t0"], p[2]["t1"]
    if any(o[0]["q"] != p[0]["q"] and o[0]["t0"] < t1 and o[2]["t1"] > t0 for o in passes):
        loop.append(p)
print("%s: %d window launches on %d queues (%s), %d passes in the loop's form, %d of them beside a pass of another queue" %
      (os.path.basename(path), len(ev), len(by_q), qcol, len(passes), len(loop)))
if not loop:
    raise SystemExit("no passes side by side in this trace")


def line(label, v):
    v = [x / 1000.0 for x in v]
    sd = statistics.pstdev(v) if len(v) > 1 else 0.0
    q = sorted(v)
    print("  %-34s n %4d  mean %7.2f  sd %5.2f  min %7.2f  median %7.2f  p90 %7.2f  max %7.2f us" %
          (label, len(v), sum(v) / len(v), sd, q[0], q[len(q) // 2], q[int(0.9 * (len(q) - 1))], q[-1]))


print("durations in the loop:")
for j, k in enumerate(("binning", "per-slice", "finish")):
    line(k, [p[j]["t1"] - p[j]["t0"] for p in loop])
line("sum of the three", [sum(p[j]["t1"] - p[j]["t0"] for j in range(3)) for p in loop])
line("chain: binning start .. finish end", [p[2]["t1"] - p[0]["t0"] for p in loop])
print("gaps on the same queue (end of a launch .. start of the next):")
line("binning -> per-slice", [p[1]["t0"] - p[0]["t1"] for p in loop])
line("per-slice -> finish", [p[2]["t0"] - p[1]["t1"] for p in loop])
g = [p[3]["t0"] - p[2]["t1"] for p in loop if p[3]]
if g: line("finish -> next pass's binning", g)
line("the two gaps inside a pass", [p[1]["t0"] - p[0]["t1"] + p[2]["t0"] - p[1]["t1"] for p in loop])
span = max(p[2]["t1"] for p in loop) - min(p[0]["t0"] for p in loop)
print("  the loop: %d passes in %.1f us, %.3f us per pass" % (len(loop), span / 1000.0, span / 1000.0 / len(loop)))
print("launches of OTHER passes in flight at the start of a per-slice launch:")
flat = [(e, p[0]["t0"]) for p in loop for e in p[:3]]
for k in ("binning", "per-slice", "finish"):
    cnt = [sum(1 for e, pid in flat if e["kind"] == k and pid != p[0]["t0"] and e["t0"] <= p[1]["t0"] < e["t1"]) for p in loop]
    hist = {c: cnt.count(c) for c in sorted(set(cnt))}
    print("  %-10s mean %.2f   %s" % (k, sum(cnt) / len(cnt), "  ".join("%d: %d" % kv for kv in hist.items())))
print("share of a per-slice launch's time during which launches of OTHER passes run (summed over them: two at once count twice):")
for k in ("binning", "per-slice", "finish"):
    sh = []
    for p in loop:
        a0, a1 = p[1]["t0"], p[1]["t1"]
        ov = sum(max(0, min(a1, e["t1"]) - max(a0, e["t0"])) for e, pid in flat if e["kind"] == k and pid != p[0]["t0"])
        sh.append(ov / float(max(1, a1 - a0)))
    print("  %-10s mean %.2f" % (k, sum(sh) / len(sh)))
