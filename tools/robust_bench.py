#!/usr/bin/env python3
"""Robust re-weighting timing, at cfg 2 (1M points x 32 candidates, 2048 x 1024, eager) and at the shipped shape
(166,667 points x 6 candidates, graph replay):

  launch  the residual launch pcl_point_residuals at B = 1 (packed order; and the caller's order) against the forward-only loss launch
          pcl_sampling_loss at B = 1 of the same build, `--launches` calls per timed run; and one pcl_robust_weights call (its six launches)
  chain   a robust chain (--iters iterations, re-weighted after --robust-iters) against the plain chain of the same length

Each pair is timed alternately (A B A B ...), median of --reps runs with the spread (min .. max).

    python tools/robust_bench.py [--reps 9] [--iters 100] [--robust-iters 20,40] [--launches 50]

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


def stat(t, per, unit_scale=1e3):
    return {"median": round(unit_scale * t[0] / per, 2), "min": round(unit_scale * t[1] / per, 2), "max": round(unit_scale * t[2] / per, 2)}


def shape(n, B, graph, args):
    H, W = 1024, 2048
    xyz, rgb = synth.box_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    t_gt, ypr = synth.gt_pose(1)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
    tr, ro = synth.start_poses(t_gt, ypr, B, seed=1)
    tr, ro = torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()
    cloud = ops.Cloud(X, C)
    pano, box = ops.Pano(img, fmt=ops.refine_texels(n, H, W)), ops.quantile_box(X, 0.05)
    t1, r1 = tr[:1].contiguous(), ro[:1].contiguous()
    row = ops.point_residuals(cloud, pano, t1, r1, packed=True)[0]
    plane, scale = ops.robust_weights(cloud, row)
    L = args.launches

    def many(f):
        def g():
            for _ in range(L):
                f()
        return g
    loss = many(lambda: ops.sampling_loss(cloud, pano, t1, r1, with_grad=False))
    packed = many(lambda: ops.point_residuals(cloud, pano, t1, r1, packed=True))
    caller = many(lambda: ops.point_residuals(cloud, pano, t1, r1))
    weights = many(lambda: ops.robust_weights(cloud, row, plane=plane, scale=scale))
    for f in (loss, packed, caller, weights):
        f()
    tl, tp, tc, tw = timed([loss, packed, caller, weights], args.reps)

    plain_gd, robust_gd = (ops.GradientDescent(cloud, pano, tr, ro, box, lr=0.1, patience=5, factor=0.8) for _ in range(2))

    def plain():
        plain_gd.reset(tr, ro)
        plain_gd.run_graph(args.iters) if graph else plain_gd.run(args.iters)

    def robust():
        robust_gd.reset(tr, ro)
        robust_gd.run_robust(args.iters, args.robust_iters, "trunc", 2.5, graph=graph)
    plain(), robust()                                          # warm-up: graph capture, caches
    ta, tb = timed([plain, robust], args.reps)
    dropped = float((robust_gd._robust["plane"][:n] == 0).float().mean())
    return {"points": n, "candidates": B, "graph": bool(graph), "iters": args.iters, "robust_iters": args.robust_iters, "texels": pano.fmt,
            "launch_us": {"sampling_loss_forward_B1": stat(tl, L), "point_residuals_packed_B1": stat(tp, L), "point_residuals_caller_B1": stat(tc, L),
                          "robust_weights": stat(tw, L), "note": "host call to completion of %d back-to-back calls, per call" % L},
            "chain_ms": {"plain": stat(ta, 1, 1.0), "robust": stat(tb, 1, 1.0), "ratio": round(tb[0] / ta[0], 4)},
            "weight_zero_fraction_after_last_reweight": round(dropped, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--robust-iters", type=lambda s: [int(v) for v in s.split(",")], default=[20, 40])
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    out = {"cfg2": shape(1_000_000, 32, False, args), "shipped": shape(166_667, 6, True, args)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
