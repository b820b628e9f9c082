#!/usr/bin/env python3
"""Per-point weights timing: microseconds per GD iteration of the WEIGHTED refinement chain against the unweighted one of
the same build, at cfg 2 (1M points x 32 candidates, 2048 x 1024, eager, two launches per iteration) and at the shipped shape
(166,667 points x 6 candidates, fused, graph replay).  The two forms are timed alternately (A B A B ...), median of --reps runs each.

    python tools/weights_bench.py [--reps 9] [--iters 100]

The weights are random levels (0, 0.3, 1, 1.7, 4.5): their values do not change the work.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from piccolo_amd import ops, synth  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed_ab(fa, fb, reps):
    """medians of A and B timed alternately: clock and cache drift over the run falls on both sides alike"""
    a, b = [], []
    for _ in range(reps):
        a.append(once(fa))
        b.append(once(fb))
    return statistics.median(a), a, statistics.median(b), b


def shape(n, B, graph, iters, reps):
    H, W = 1024, 2048
    xyz, rgb = synth.box_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    t_gt, ypr = synth.gt_pose(1)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
    tr, ro = synth.start_poses(t_gt, ypr, B, seed=1)
    tr, ro = torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()
    w = torch.from_numpy(np.array([0.0, 0.3, 1.0, 1.7, 4.5], np.float32)[np.random.default_rng(3).integers(0, 5, size=n)]).cuda()
    plain = ops.Cloud(X, C)
    weighted = ops.Cloud(X, C, order=plain.order, weights=w)
    pano, box = ops.Pano(img), ops.quantile_box(X, 0.05)
    engines = [ops.GradientDescent(c, pano, tr, ro, box, lr=0.1, patience=5, factor=0.8) for c in (plain, weighted)]

    def run(gd):
        def f():
            gd.reset(tr, ro)
            gd.run_graph(iters) if graph else gd.run(iters)
        return f
    fa, fb = run(engines[0]), run(engines[1])
    fa(), fb()                                                 # warm-up: graph capture, caches
    ta, alla, tb, allb = timed_ab(fa, fb, reps)
    return {"points": n, "candidates": B, "graph": bool(graph), "fused": _fused(n, B), "iters": iters,
            "unweighted_us_per_iter": round(1e3 * ta / iters, 2), "weighted_us_per_iter": round(1e3 * tb / iters, 2), "ratio": round(tb / ta, 4),
            "unweighted_runs_ms": [round(v, 3) for v in alla], "weighted_runs_ms": [round(v, 3) for v in allb]}


def _fused(n, B):
    """does the chain of this shape run one launch per iteration (pcl_gd_plan's answer, which the engines' default fuse setting follows)"""
    f = ctypes.c_int(0)
    ops._lib.load().pcl_gd_plan(n, B, None, None, ctypes.byref(f))
    return f.value == 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    out = {"cfg2": shape(1_000_000, 32, False, args.iters, args.reps), "shipped": shape(166_667, 6, True, args.iters, args.reps)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
