#!/usr/bin/env python3
"""The Levenberg-Marquardt polish of the R x I winners of a rooms x images chain: ONE gauss_newton_refine_rooms_at_winners
against the fastest route there was, one gauss_newton_refine_images_at_winners per room; and a polished room search
(omniloc_batch_rooms_images_polished) against the plain one (omniloc_batch_rooms_images), ms per image.  Same build, same process, timed
alternately.

Shapes: 8 rooms x 166,667 points x 8 images (shared colours, and a colour set per image) and 4 rooms x 1M points x 5 images (shared colours);
rooms side by side (synth.rooms_side_by_side), 2048 x 1024 panoramas, image i rendered in room i mod R, the texel format of the largest
room's refinement.  The polish's start poses are near each room's ground truth.

Per shape: us per LM iteration of all R x I poses — (a call of --iters iterations - a call of 0 iterations) / iters — and ms per image of
a whole polish of --polish iterations (host call to completion, outputs and workspace allocated per call), median of --reps rounds of
--launches back-to-back calls with the spread, and the ratio batched / per room; then ms per image of the room search (6 candidates per
(room, image), 100 iterations; gn_iters = --polish with pose_covariance), median of --reps.

Not a test and not part of bench.py.

    python tools/gn_rooms_bench.py [--reps 9] [--launches 10] [--iters 10] [--polish 5] [--shapes a,b,c]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from piccolo_amd import omniloc as po, ops, synth  # noqa: E402

H, W = 1024, 2048


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fns, reps):
    """every function timed in turn, `reps` rounds: clock and cache drift over the run falls on all alike -> one list of ms per function"""
    runs = [[] for _ in fns]
    for _ in range(reps):
        for r, f in zip(runs, fns):
            r.append(once(f))
    return runs


def stat(ms, scale):
    return {"median": round(scale * statistics.median(ms), 3), "min": round(scale * min(ms), 3), "max": round(scale * max(ms), 3)}


def shape(n, R, I, sets, args):
    scenes = synth.rooms_side_by_side((n,) * R, seed=1)
    rooms = [(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()) for x, c in scenes]
    fmt = ops.refine_texels(n, H, W)
    imgs = []
    for i in range(I):
        t_gt, ypr = synth.room_gt_pose(i % R, 1 + i)
        X, C = rooms[i % R]
        imgs.append(synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W))))
    panos = [ops.Pano(im, fmt=fmt) for im in imgs]
    wins = torch.zeros(R * I, 16, device="cuda")
    for r in range(R):
        for i in range(I):
            t_gt, ypr = synth.room_gt_pose(r, 1 + i)
            tr, ro = synth.start_poses(t_gt, ypr, 1, seed=1 + 17 * r + i, sigma_t=0.02, sigma_r=0.01)
            wins[r * I + i, 0:3], wins[r * I + i, 13:16] = torch.from_numpy(tr[0]).cuda(), torch.from_numpy(ro[0]).cuda()
    if sets:
        rng = np.random.default_rng(5)
        cols = [[(C * torch.from_numpy((0.9 + 0.2 * rng.random(3)).astype(np.float32)).cuda()).clamp(0, 1).contiguous() for _ in range(I)]
                for _, C in rooms]
        clouds = [ops.Cloud.with_color_sets(X, cols[r]) for r, (X, _) in enumerate(rooms)]
        search_rooms = [(X, cols[r]) for r, (X, _) in enumerate(rooms)]
    else:
        clouds = [ops.Cloud(X, C) for X, C in rooms]
        search_rooms = rooms
    per_room = [wins[r * I:(r + 1) * I].contiguous() for r in range(R)]
    L, K, P = args.launches, args.iters, args.polish

    def batched(iters):
        def f():
            for _ in range(L):
                ops.gauss_newton_refine_rooms_at_winners(clouds, panos, wins, iters=iters)
        return f

    def separate(iters):
        def f():
            for _ in range(L):
                for r in range(R):
                    ops.gauss_newton_refine_images_at_winners(clouds[r], panos, per_room[r], iters=iters)
        return f
    fns = [batched(0), separate(0), batched(K), separate(K), batched(P), separate(P)]
    for f in fns:
        f()
    b0, s0, bk, sk, bp, sp = timed(fns, args.reps)
    b_it, s_it = [(a - b) / K for a, b in zip(bk, b0)], [(a - b) / K for a, b in zip(sk, s0)]
    res = ops.gauss_newton_refine_rooms_at_winners(clouds, panos, wins, iters=K)
    same = all(torch.equal(res["trans"][r * I:(r + 1) * I], ops.gauss_newton_refine_images_at_winners(clouds[r], panos, per_room[r], iters=K)["trans"])
               for r in range(R))
    out = {"points": n, "rooms": R, "images": I, "colour_sets": bool(sets), "texels": fmt,
           "lm_iteration_us_all_poses": {"batched": stat(b_it, 1e3 / L), "per_room": stat(s_it, 1e3 / L),
                                         "ratio": round(statistics.median(b_it) / statistics.median(s_it), 3)},
           "polish_%d_iters_ms_per_image" % P: {"batched": stat(bp, 1.0 / (L * I)), "per_room": stat(sp, 1.0 / (L * I)),
                                                "ratio": round(statistics.median(bp) / statistics.median(sp), 3)},
           "status_0": int((res["status"] == 0).sum()), "rows_equal_the_per_room_calls": bool(same)}

    # the room search, plain and polished: 6 candidates per (room, image), the shipped chain
    base = dict(num_iter=100, num_input=6, lr=0.1, patience=5, factor=0.8, out_of_room_quantile=0.05)
    plain_cfg, polished_cfg = SimpleNamespace(**base), SimpleNamespace(**base, gn_iters=P, pose_covariance=True)
    starts = []
    for r in range(R):
        row = []
        for i in range(I):
            t_gt, ypr = synth.room_gt_pose(r, 1 + i)
            tr, ro = synth.start_poses(t_gt, ypr, 6, seed=3 + 7 * r + 101 * i, sigma_t=0.4, sigma_r=0.2)
            row.append((torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()))
        starts.append(row)

    def lists():
        return [[t.clone() for t, _ in row] for row in starts], [[r.clone() for _, r in row] for row in starts]

    def plain():
        po.omniloc_batch_rooms_images(imgs, search_rooms, *lists(), plain_cfg)

    def polished():
        po.omniloc_batch_rooms_images_polished(imgs, search_rooms, *lists(), polished_cfg)
    for f in (plain, polished):
        f()
    pl, pol = timed([plain, polished], args.reps)
    out["room_search_ms_per_image"] = {"plain": stat(pl, 1.0 / I), "polished": stat(pol, 1.0 / I),
                                       "ratio": round(statistics.median(pol) / statistics.median(pl), 3),
                                       "one_chain": bool(po.rooms_images_chain_pays(n * R, 6))}
    return out


SHAPES = {"rooms8_shared": (166_667, 8, 8, False), "rooms8_colour_sets": (166_667, 8, 8, True), "rooms4_1m_shared": (1_000_000, 4, 5, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--polish", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    out = {}
    for name in args.shapes.split(","):
        out[name] = shape(*SHAPES[name], args)
        po._cache.clear()                                   # (the next shape's clouds and panoramas: not beside this one's)
    out["note"] = ("host call to completion of %d back-to-back polishes of all rooms x images, outputs and workspace allocated per call; an LM "
                   "iteration is (a call of %d iterations - a call of 0) / %d; batched: one gauss_newton_refine_rooms_at_winners, per_room: one "
                   "gauss_newton_refine_images_at_winners per room; room search: omniloc_batch_rooms_images against "
                   "omniloc_batch_rooms_images_polished with gn_iters = %d and pose_covariance, 6 candidates, 100 iterations"
                   % (args.launches, args.iters, args.iters, args.polish))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
