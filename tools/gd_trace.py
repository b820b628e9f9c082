#!/usr/bin/env python3
"""Reads a rocprofv3 --kernel-trace CSV of a bench.py run and reports, per loss-launch shape, how a GD chain fills the GPU.

  usage: python3 tools/gd_trace.py <dir or kernel_trace.csv> [--json out.json]

A chain is a run of loss launches of one shape (same kernel, same grid) whose neighbours lie less than a launch apart.  Per shape:
  - loss_us              median duration of a loss launch
  - gap_us               median time with NO pcl_* kernel running between the end of one loss launch and the start of the next one of
                         the same chain (single-stream chains: epilogue + two kernel boundaries; split chains: what the other half
                         does not cover)
  - idle_gap_share       gap / (loss + gap)
and the seconds per point-pose of profiles/roofs.json's cfg5 entry: 1 - poses x N x that / loss_us is what a launch loses to its ramp
and tail against a launch of 38 rounds.
Split chains (two half-chains on two streams) show as TWO interleaved sequences of the half shape on two queues: for
those the tool also prints, per queue, where the loss launch of iterations 1, 50 and 99 starts inside the launch the other half is running
(offset / that launch's duration; median over the chains, and how many chains) and the share of a chain's wall time during which no
pcl_* kernel runs at all.
"""
import bisect
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def rows_of(path):
    files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    out = []
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "pcl_" not in name:
                continue
            out.append({"name": name.split("(")[0].replace("void ", ""), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                        "grid": int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0), "wg": int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256),
                        "q": r.get("Stream_Id") or r.get("Queue_Id") or "0"})
    out.sort(key=lambda r: r["t0"])
    return out


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else float("nan")


def busy_union(rows, lo, hi):
    """nanoseconds of [lo, hi) covered by at least one kernel of rows"""
    cov, end = 0, lo
    for r in rows:
        a, b = max(r["t0"], end), min(r["t1"], hi)
        if b > a:
            cov += b - a
            end = b
    return cov


def chains_of(seq):
    """split one queue's loss launches of one shape into chains: a neighbour more than two launch durations away starts a new one"""
    chains, cur = [], []
    for r in seq:
        if cur and r["t0"] - cur[-1]["t1"] > 2 * (cur[-1]["t1"] - cur[-1]["t0"]) + 20000:
            chains.append(cur)
            cur = []
        cur.append(r)
    if cur:
        chains.append(cur)
    return [c for c in chains if len(c) >= 20]


def main(argv):
    path, jout = argv[1], None
    if "--json" in argv:
        jout = argv[argv.index("--json") + 1]
    rows = rows_of(path)
    loss = [r for r in rows if r["name"].startswith("pcl_loss")]
    starts = [r["t0"] for r in rows]

    def window(lo, hi):
        # kernels that overlap [lo, hi): none of this library's runs longer than 20 ms
        return [r for r in rows[bisect.bisect_left(starts, lo - 20_000_000):bisect.bisect_left(starts, hi)] if r["t1"] > lo]
    per_point_pose = None
    roofs = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "roofs.json")
    if os.path.exists(roofs):
        e = json.load(open(roofs)).get("cfg5/poses64/f16")
        if e:
            per_point_pose = e["avg_duration_us_kernel_trace"] * 1e-6 / (64 * 10_000_000)
    shapes = defaultdict(lambda: defaultdict(list))               # (kernel, blocks) -> queue -> launches
    for r in loss:
        shapes[(r["name"], r["grid"] // max(1, r["wg"]))][r["q"]].append(r)                      # (rocprofv3's grid size counts threads)
    report = {}
    for (name, blocks), queues in sorted(shapes.items(), key=lambda kv: -sum(len(v) for v in kv[1].values())):
        chains = [c for q in queues.values() for c in chains_of(q)]
        if not chains:
            continue
        durs, gaps = [], []
        for c in chains:
            for a, b in zip(c[1:-1], c[2:]):                       # all but the first and last iteration
                durs.append(a["t1"] - a["t0"])
                between = [r for r in window(a["t1"], b["t0"]) if r is not a and r is not b]
                gaps.append((b["t0"] - a["t1"]) - busy_union(between, a["t1"], b["t0"]))
        e = {"kernel": name, "blocks": blocks, "queues": len(queues), "chains": len(chains), "launches": sum(len(c) for c in chains),
             "loss_us": median(durs) / 1e3, "gap_us": median(gaps) / 1e3}
        e["idle_gap_share"] = e["gap_us"] / (e["loss_us"] + e["gap_us"])
        report["%s/%d" % (name, blocks)] = e
        # split chains: where does a launch of one queue start inside the launch the other queue is running?
        if len(queues) >= 2:
            every = sorted((r for q in queues.values() for r in q), key=lambda r: r["t0"])
            t0s = [r["t0"] for r in every]
            offs = defaultdict(lambda: defaultdict(list))
            idle = []
            for c in chains:
                for it in (1, 50, 99):
                    k = it if len(c) >= 100 else it - 1            # (half A's first iteration goes out as two smaller launches)
                    if not 0 <= k < len(c):
                        continue
                    other = [r for r in every[max(0, bisect.bisect_right(t0s, c[k]["t0"]) - 4):bisect.bisect_right(t0s, c[k]["t0"])]
                             if r["q"] != c[k]["q"] and r["t1"] > c[k]["t0"]]
                    if other:
                        offs[c[k]["q"]][it].append((c[k]["t0"] - other[-1]["t0"]) / float(other[-1]["t1"] - other[-1]["t0"]))
                lo, hi = c[1]["t0"], c[-2]["t1"]
                idle.append(1.0 - busy_union(window(lo, hi), lo, hi) / float(hi - lo))
            e["start_inside_the_other_halfs_launch"] = {"queue %s" % q: {str(it): [round(median(v), 3), len(v)] for it, v in sorted(d.items())}
                                                        for q, d in sorted(offs.items())}
            e["nothing_running_share"] = median(idle)
    # (poses per launch are the caller's knowledge: loss_us against poses x points x this figure is the ramp-and-tail share)
    if per_point_pose:
        print("seconds per point-pose of the cfg5 entry: %.4g" % per_point_pose)
    for k, e in report.items():
        print(k, json.dumps(e, sort_keys=True))
    if jout:
        json.dump(report, open(jout, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv)
