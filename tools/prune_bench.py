#!/usr/bin/env python3
"""Pruned against full refinement chains, timing: the same refinement with and without cfg.prune_iters / cfg.prune_keep,
on the same build, timed alternately (full pruned full pruned ...), medians of --reps, with the spread of the full form; next to the time
ratio the work ratio sum(candidates_s x iterations_s) / (B x num_iter) of the schedule, and per candidate count of the schedule the time
of one iteration of the chain at that count (median of --reps runs of 40 iterations: what a segment costs per iteration), which is
what explains a time ratio above the work ratio.

    python tools/prune_bench.py [--reps 9] [--shapes cfg2,shipped,rooms8] [--out file.json]

Shapes: cfg2 = 1M points x 32 candidates, 2048 x 1024, schedule 20:16, 40:8; shipped = 166,667 x 6, schedule 20:4; rooms8 = 8 rooms of
166,667 points x 6 candidates (omniloc_batch_rooms), schedule 20:4.  100 iterations.  Prints one JSON object per line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from piccolo_amd import ops, synth  # noqa: E402
from piccolo_amd import omniloc as po  # noqa: E402

H, W, ITERS = 1024, 2048, 100
SHAPES = {"cfg2": (1, 1_000_000, 32, [20, 40], [16, 8]), "shipped": (1, 166_667, 6, [20], [4]), "rooms8": (8, 166_667, 6, [20], [4])}


class Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def scene(R, n, per):
    rooms = [(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()) for x, c in synth.rooms_side_by_side([n] * R, seed=R)]
    t_gt, ypr = synth.room_gt_pose(0, 1)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(rooms[0][0], torch.from_numpy(t_gt), torch.from_numpy(ypr)), rooms[0][1], (H, W)))
    starts = []
    for r in range(R):
        t, y = synth.room_gt_pose(r, 1)
        tr, ro = synth.start_poses(t, y, per, seed=r, sigma_t=0.4, sigma_r=0.2)
        starts.append((torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()))
    return rooms, img, starts


def per_iteration_us(rooms, img, starts, cfg, per, reps, span=40):
    """one iteration of the chain with `per` candidates per room, us: the engine the surface would run (eager or replayed by its rule)"""
    R = len(rooms)
    tr, ro = torch.cat([s[0][:per] for s in starts]), torch.cat([s[1][:per] for s in starts])
    args = po._engine_args(cfg)
    if R == 1:
        pano = po.packed_pano(img, n_points=rooms[0][0].shape[0])
        gd = ops.GradientDescent(po.packed_cloud(*rooms[0]), pano, tr, ro, po.quantile_box_of(rooms[0][0], 0.05), **args)
        points = rooms[0][0].shape[0]
    else:
        pano = po.packed_pano(img, n_points=max(x.shape[0] for x, _ in rooms))
        gd = ops.GradientDescentRooms([(po.packed_cloud(x, c), po.quantile_box_of(x, 0.05)) for x, c in rooms], pano, tr, ro, **args)
        gd.set_panos([pano])
        points = sum(x.shape[0] for x, _ in rooms)
    run = gd.run_graph if po._replays_graph(cfg, points * per, False) else gd.run
    run(span)
    return round(statistics.median(once(lambda: run(span)) for _ in range(reps)) / span * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="cfg2,shipped,rooms8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.shapes.split(","):
        R, n, per, p_iters, p_keep = SHAPES[name]
        rooms, img, starts = scene(R, n, per)
        base = dict(lr=0.1, num_iter=ITERS, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=per)
        cfgs = {"full": Cfg(**base), "pruned": Cfg(prune_iters=p_iters, prune_keep=p_keep, **base)}
        sched = po.prune_schedule(cfgs["pruned"], per)

        def form(cfg):
            if R == 1:
                return [po.omniloc_batch(img, rooms[0][0], rooms[0][1], starts[0][0].clone(), starts[0][1].clone(), cfg, {})]
            return po.omniloc_batch_rooms(img, rooms, [s[0].clone() for s in starts], [s[1].clone() for s in starts], cfg)
        res = {k: form(c) for k, c in cfgs.items()}                  # warm-up: packing, engines, graph capture
        res = {k: form(c) for k, c in cfgs.items()}
        runs = {"full": [], "pruned": []}
        for _ in range(args.reps):                                   # alternately: drift falls on both forms alike
            for k in ("full", "pruned"):
                runs[k].append(once(lambda: form(cfgs[k])))
        med = {k: statistics.median(v) for k, v in runs.items()}
        rec = {"shape": name, "rooms": R, "points": n, "per_room": per, "iters": ITERS, "schedule": sched,
               "full_ms": round(med["full"], 3), "pruned_ms": round(med["pruned"], 3),
               "full_spread": round((max(runs["full"]) - min(runs["full"])) / med["full"], 4),
               "pruned_spread": round((max(runs["pruned"]) - min(runs["pruned"])) / med["pruned"], 4),
               "time_ratio": round(med["pruned"] / med["full"], 3),
               "work_ratio": round(sum(k * c for k, c in sched) / (per * ITERS), 3),
               "loss_ratio_max": round(max(float(p[2]) / float(f[2]) for p, f in zip(res["pruned"], res["full"])), 5),
               "iteration_us": {str(c): per_iteration_us(rooms, img, starts, cfgs["full"], c, args.reps) for _, c in sched}}
        rec["faster_than_spread"] = bool(1.0 - rec["time_ratio"] > rec["full_spread"])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del rooms, img, starts
        po._cache.clear()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
