"""From a rocprofv3 --kernel-trace CSV dir of a run with passes in flight: how long the launches of a slot wait for a hardware
queue, and how much the slots overlap.    tools/queue_wait.py <dir> [skip ms]

A slot is recognised by its stream, the one that carries begin_frame_kernel; the launches of a graph's parallel branches keep
the Stream_Id of the stream the graph was launched on and differ in Queue_Id.  Within a pass every launch depends on launches
of its own slot only, so the time between the end of everything the slot has run so far and the start of its next launch is
time that launch was ready and not running: per slot and per kind (material = shade_scan_kernel, trace = the closest-hit and
any-hit launches of the bounces) the sum of these waits, and how much of it passed while a launch of ANOTHER slot was running
on the hardware queue the waiting launch then ran on — the in-order queue it stood in.  (begin_frame / generate / primary trace
are left out: the gap in front of a pass is the host's.)
Then, over the extent of the launches looked at: the share of the time in which launches of more than one slot are resident,
and the streams every hardware queue served.  The first `skip` ms (set-up, warm-up; default: the first half of the kernels' time
span) are left out."""
import collections, csv, glob, re, statistics, sys

f = glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "nxd::" in r["Kernel_Name"]]
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["n"] = re.sub(r"[(].*", "", r["Kernel_Name"]).replace("void ", "").replace("nxd::", "")
t0, t1 = min(r["s"] for r in rows), max(r["e"] for r in rows)
skip = float(sys.argv[2]) * 1e6 if len(sys.argv) > 2 else (t1 - t0) / 2
rows = sorted((r for r in rows if r["s"] >= t0 + skip), key=lambda r: r["s"])
slots = sorted({r["Stream_Id"] for r in rows if r["n"].startswith("begin_frame")})
by_stream, by_queue = collections.defaultdict(list), collections.defaultdict(list)
for r in rows:
    by_stream[r["Stream_Id"]].append(r)
    by_queue[r["Queue_Id"]].append(r)
extent = max(r["e"] for r in rows) - rows[0]["s"]
print("%d launches over %.1f ms, slot streams %s, all streams %s" % (len(rows), extent / 1e6, slots, sorted(by_stream)))
print("hardware queue -> streams: " + ", ".join("%s -> %s" % (q, sorted({r["Stream_Id"] for r in rs})) for q, rs in sorted(by_queue.items())))


def kind(r):
    if r["n"].startswith("shade_scan"):
        return "material"
    m = re.match(r"trace_kernel<(\d+)u>", r["n"])
    if m and not int(m.group(1)) & 4:  # (a set of trace features, nx_variants.h — bit 2: the primary launch's entry instance)
        return "trace"
    return None


def covered(a, b, r):  # ns of [a, b] in which a launch of another stream runs on r's hardware queue
    spans = sorted((max(a, t["s"]), min(b, t["e"])) for t in by_queue[r["Queue_Id"]] if t["Stream_Id"] != r["Stream_Id"] and t["e"] > a and t["s"] < b)
    total, at = 0, a
    for s, e in spans:
        if e > at:
            total += e - max(s, at)
            at = e
    return total


for sid in slots:
    waits, blocked = collections.defaultdict(list), collections.defaultdict(float)
    done = None  # the end of everything the slot has run so far
    for r in by_stream[sid]:
        k = kind(r)
        if k and done is not None:
            w = max(0, r["s"] - done)
            waits[k].append(w / 1e3)
            if w:
                blocked[k] += covered(done, r["s"], r) / 1e6
        done = r["e"] if done is None else max(done, r["e"])
    for k in ("material", "trace"):
        if waits[k]:
            print("slot stream %s, %-8s: %3d launches ready and waiting: median %6.0f us, max %7.0f us, in all %6.1f ms, of which %6.1f ms behind another slot's launch on the same hardware queue"
                  % (sid, k, len(waits[k]), statistics.median(waits[k]), max(waits[k]), sum(waits[k]) / 1e3, blocked[k]))
events = []
for r in rows:
    if r["Stream_Id"] in slots:
        events += [(r["s"], 1, r["Stream_Id"]), (r["e"], -1, r["Stream_Id"])]
events.sort()
live = collections.Counter()
at = events[0][0]
share = collections.Counter()
for t, d, sid in events:
    share[min(sum(1 for v in live.values() if v > 0), 4)] += t - at
    live[sid] += d
    at = t
span = events[-1][0] - events[0][0]
print("slots with a launch resident, share of the time: " + ", ".join("%d: %.1f %%" % (n, 100.0 * share[n] / span) for n in range(5)) +
      "; two or more: %.1f %%" % (100.0 * sum(share[n] for n in (2, 3, 4)) / span))
