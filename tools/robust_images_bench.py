#!/usr/bin/env python3
"""Robust refinement of several query images of one room: ms per image of a robust chain (--iters iterations, re-weighted
after --robust-iters) with I images in ONE launch chain (ops.GradientDescent(weight_sets=I): pcl_gd_run_weight_sets, one weight plane per
image) against I single-image robust chains one after another, on the same build:

  shipped         166,667 points x 6 candidates per image, 2048 x 1024, RGBA8 texels, 8 images, shared colours, graph replay
  shipped_sets    the same with a colour set per image
  cfg2            1M points x 32 candidates per image, fp16 texels, 5 images, shared colours, eager

The two routes are timed alternately (A B A B ...), median of --reps runs with the spread (min .. max).  Every route's result is checked once
against the other's (the same bits per image).

    python tools/robust_images_bench.py [--reps 9] [--iters 100] [--robust-iters 20,40] [--only shipped,shipped_sets,cfg2]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from piccolo_amd import ops, synth  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fns, reps):
    """every function timed in turn, `reps` rounds: clock and cache drift over the run falls on all alike -> [(median, min, max), ...]"""
    runs = [[] for _ in fns]
    for _ in range(reps):
        for r, f in zip(runs, fns):
            r.append(once(f))
    return [(statistics.median(r), min(r), max(r)) for r in runs]


def stat(t, per):
    return {"median": round(t[0] / per, 3), "min": round(t[1] / per, 3), "max": round(t[2] / per, 3)}


def shape(n, per, I, sets, graph, args):
    H, W = 1024, 2048
    xyz, rgb = synth.box_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    fmt = ops.refine_texels(n, H, W)
    panos, starts = [], []
    for i in range(I):
        t_gt, ypr = synth.gt_pose(1 + i)
        img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
        panos.append(ops.Pano(img, fmt=fmt))
        tr, ro = synth.start_poses(t_gt, ypr, per, seed=1 + i)
        starts.append((torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()))
    # a fifth of the cloud recoloured after the render (per image another fifth under colour sets): something for the weights to drop
    gen = torch.Generator(device="cuda").manual_seed(5)

    def recolour():
        hit = torch.rand(n, device="cuda", generator=gen) < 0.2
        return torch.where(hit[:, None], torch.rand(n, 3, device="cuda", generator=gen), C)
    rgbs = [recolour() for _ in range(I)] if sets else [recolour()] * I
    singles = [ops.Cloud(X, rgbs[0])]
    singles += [ops.Cloud(X, r, order=singles[0].order) for r in rgbs[1:]] if sets else singles * (I - 1)
    cloud = ops.Cloud.with_color_sets(X, rgbs, order=singles[0].order) if sets else singles[0]
    box = ops.quantile_box(X, 0.05)
    hyper = dict(lr=0.1, patience=5, factor=0.8)
    tr_all, ro_all = torch.cat([t for t, _ in starts]), torch.cat([r for _, r in starts])
    multi = ops.GradientDescent(cloud, panos[0], tr_all, ro_all, box, weight_sets=I, **hyper)
    alone = [ops.GradientDescent(singles[i], panos[i], starts[i][0], starts[i][1], box, **hyper) for i in range(I)]

    def one_chain():
        multi.reset(tr_all, ro_all)
        multi.set_pano_groups(panos)
        multi.run_robust(args.iters, args.robust_iters, "trunc", 2.5, graph=graph)
        return multi.winners(I)

    def one_at_a_time():
        out = []
        for g, (t, r) in zip(alone, starts):
            g.reset(t, r)
            g.run_robust(args.iters, args.robust_iters, "trunc", 2.5, graph=graph)
            out.append(g.winner(1))
        return torch.cat(out)
    a, b = one_chain(), one_at_a_time()                        # warm-up (graph capture, caches) and the check
    same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    ta, tb = timed([one_chain, one_at_a_time], args.reps)
    dropped = float((multi.weight_planes()[:, :n] == 0).float().mean())
    nch, G, fused = ops.ctypes.c_int(), ops.ctypes.c_int(), ops.ctypes.c_int()
    ops._lib.load().pcl_gd_plan_weight_sets(n, I * per, I, ops.ctypes.byref(multi.hyper), ops.ctypes.byref(nch), ops.ctypes.byref(G),
                                            ops.ctypes.byref(fused))
    return {"points": n, "candidates_per_image": per, "images": I, "color_sets": I if sets else 1, "graph": bool(graph), "iters": args.iters,
            "robust_iters": args.robust_iters, "texels": panos[0].fmt, "chunks": nch.value, "poses_per_block": G.value, "fused": fused.value,
            "ms_per_image": {"one_chain": stat(ta, I), "one_at_a_time": stat(tb, I), "ratio": round(ta[0] / tb[0], 4)},
            "same_bits_per_image": same, "weight_zero_fraction_after_last_reweight": round(dropped, 4)}


SHAPES = {"shipped": (166_667, 6, 8, False, True), "shipped_sets": (166_667, 6, 8, True, True), "cfg2": (1_000_000, 32, 5, False, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--robust-iters", type=lambda s: [int(v) for v in s.split(",")], default=[20, 40])
    ap.add_argument("--only", type=lambda s: s.split(","), default=list(SHAPES))
    args = ap.parse_args()
    out = {name: shape(*SHAPES[name], args) for name in args.only}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
