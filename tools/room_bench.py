#!/usr/bin/env python3
"""Room search timing: one query panorama refined against R rooms in ONE launch chain (omniloc_batch_rooms) against
the sum of R omniloc_batch calls the way the harness runs them (each side replays a captured graph where the product's rule says so:
batched_graph / sequential_graph in the output), both with the packed clouds already cached (the room
clouds of an area are read once), and the whole localize_in_rooms (colour preprocessing + make_input per room + the chain).

    python tools/room_bench.py [--reps 5] [--rooms 1,4,8,16,32] [--out file.json]

Shipped shape: rooms of 166,667 points, 6 candidates, 2048 x 1024 panorama, 100 iterations; plus one 1M-point x 32-candidate line with
R = 4.  Prints one JSON object per line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from piccolo_amd import localize, ops, synth  # noqa: E402
from piccolo_amd import omniloc as po  # noqa: E402


class Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fn, reps):
    out = [once(fn) for _ in range(reps)]
    return statistics.median(out), out


def timed_ab(fa, fb, reps):
    """medians of A and B timed alternately (A B A B ...): clock and cache drift over the run falls on both sides alike"""
    a, b = [], []
    for _ in range(reps):
        a.append(once(fa))
        b.append(once(fb))
    return statistics.median(a), a, statistics.median(b), b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rooms", default="1,4,8,16,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-localize", action="store_true")
    args = ap.parse_args()
    # every room's packed cloud, order and box stay cached for both forms (a room search of an area reuses them for every image)
    for k in ("cloud", "order", "box"):
        po._CAPACITY[k] = 128
    H, W, iters = 1024, 2048, 100
    lines = []
    shapes = [(int(r), 166_667, 6) for r in args.rooms.split(",")] + [(4, 1_000_000, 32)]
    for R, n, per_room in shapes:
        rooms = [(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()) for x, c in synth.rooms_side_by_side([n] * R, seed=R)]
        t_gt, ypr = synth.room_gt_pose(0, 1)
        xyz0, rgb0 = rooms[0]
        img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(xyz0, torch.from_numpy(t_gt), torch.from_numpy(ypr)), rgb0, (H, W)))
        starts = []
        for r in range(R):
            t, y = synth.room_gt_pose(r, 2 + r)
            tr, ro = synth.start_poses(t, y, per_room, seed=r, sigma_t=0.4, sigma_r=0.2)
            starts.append((torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()))
        cfg = Cfg(lr=0.1, num_iter=iters, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=per_room)

        def batched():
            return po.omniloc_batch_rooms(img, rooms, [t.clone() for t, _ in starts], [r.clone() for _, r in starts], cfg)

        def sequential():
            return [po.omniloc_batch(img, x, c, t.clone(), r.clone(), cfg, {}) for (x, c), (t, r) in zip(rooms, starts)]
        batched()                                           # warm-up: packing, engines, graph capture
        sequential()
        same = all(all(torch.equal(a, b) for a, b in zip(x, y)) for x, y in zip(batched(), sequential()))
        tb, allb, ts, alls = timed_ab(batched, sequential, args.reps)
        # which side replays a captured graph (omniloc._rooms_chain / _refine's rule: points x candidates of the chain <= GRAPH_POINT_POSES)
        graph_b = R > 1 and R * n * per_room <= po.GRAPH_POINT_POSES or R == 1 and n * per_room <= po.GRAPH_POINT_POSES
        rec = {"rooms": R, "points": n, "per_room": per_room, "iters": iters, "batched_graph": graph_b,
               "sequential_graph": n * per_room <= po.GRAPH_POINT_POSES, "batched_ms": round(tb, 3), "sequential_ms": round(ts, 3),
               "ratio": round(tb / ts, 3), "batched_us_per_iter": round(1e3 * tb / iters, 2),
               "sequential_us_per_iter_per_room": round(1e3 * ts / iters / R, 2), "identical": bool(same),
               "batched_runs_ms": [round(v, 3) for v in allb], "sequential_runs_ms": [round(v, 3) for v in alls]}
        if not args.no_localize and per_room == 6:
            icfg = Cfg(dataset="Stanford2D-3D-S", num_trans=50, xy_only=False, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4,
                       criterion="loss_histogram", num_intermediate=50, num_input=6, num_split_h=4, num_split_w=4, lr=0.1, num_iter=iters,
                       patience=5, factor=0.8, out_of_room_quantile=0.05, parallel=True, sharpen_color=True, num_bins=256)
            init = localize.get_init_dict(icfg)
            localize.localize_in_rooms(img, img, rooms, icfg, init)
            tl, _ = timed(lambda: localize.localize_in_rooms(img, img, rooms, icfg, init), max(1, args.reps // 2))
            rec["localize_in_rooms_ms"] = round(tl, 3)
            rec["localize_minus_refinement_ms_per_room"] = round((tl - tb) / R, 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del rooms
        po._cache.clear()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
