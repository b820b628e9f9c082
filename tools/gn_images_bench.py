#!/usr/bin/env python3
"""The Levenberg-Marquardt polish of the I winners of a shared chain: ONE gauss_newton_refine_images_at_winners against I
separate gauss_newton_refine_at_winners calls, same build, same process, timed alternately.

Shapes: the shipped shape (166,667 points, I = 8; shared colours, and a colour set per image) and cfg 2 (1M points, I = 5, shared colours),
2048 x 1024 panoramas rendered at different poses, the refinement's texel format.  The winners rows are start poses near the ground truth,
so that no pose freezes.

Per shape: us per LM iteration of all I poses — (a call of --iters iterations - a call of 0 iterations) / iters — and ms per image of a
whole polish of --polish iterations (host call to completion, outputs and workspace allocated per call), median of --reps rounds of
--launches back-to-back calls with the spread, and the ratio batched / separate.

Not a test and not part of bench.py.

    python tools/gn_images_bench.py [--reps 9] [--launches 10] [--iters 10] [--polish 5]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from piccolo_amd import ops, synth  # noqa: E402

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


def shape(n, I, sets, args):
    xyz, rgb = synth.box_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    fmt = ops.refine_texels(n, H, W)
    panos, wins = [], torch.zeros(I, 16, device="cuda")
    for i in range(I):
        t_gt, ypr = synth.gt_pose(1 + i)
        img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
        panos.append(ops.Pano(img, fmt=fmt))
        tr, ro = synth.start_poses(t_gt, ypr, 1, seed=1 + i, sigma_t=0.02, sigma_r=0.01)
        wins[i, 0:3], wins[i, 13:16] = torch.from_numpy(tr[0]).cuda(), torch.from_numpy(ro[0]).cuda()
    if sets:
        rng = np.random.default_rng(5)
        rgbs = [torch.from_numpy(np.clip(rgb * (0.9 + 0.2 * rng.random(3)), 0, 1).astype(np.float32)).cuda() for _ in range(I)]
        singles = [ops.Cloud(X, c) for c in rgbs]
        cloud = ops.Cloud.with_color_sets(X, rgbs, order=singles[0].order)
    else:
        cloud = ops.Cloud(X, C)
        singles = [cloud] * I
    rows = [wins[i:i + 1].contiguous() for i in range(I)]
    L, K, P = args.launches, args.iters, args.polish

    def batched(iters):
        def f():
            for _ in range(L):
                ops.gauss_newton_refine_images_at_winners(cloud, panos, wins, iters=iters)
        return f

    def separate(iters):
        def f():
            for _ in range(L):
                for i in range(I):
                    ops.gauss_newton_refine_at_winners(singles[i], panos[i], rows[i], iters=iters)
        return f
    fns = [batched(0), separate(0), batched(K), separate(K), batched(P), separate(P)]
    for f in fns:
        f()
    b0, s0, bk, sk, bp, sp = timed(fns, args.reps)
    b_it, s_it = [(a - b) / K for a, b in zip(bk, b0)], [(a - b) / K for a, b in zip(sk, s0)]
    res = ops.gauss_newton_refine_images_at_winners(cloud, panos, wins, iters=K)
    same = all(torch.equal(res["trans"][i:i + 1], ops.gauss_newton_refine_at_winners(singles[i], panos[i], rows[i], iters=K)["trans"]) for i in range(I))
    return {"points": n, "images": I, "colour_sets": bool(sets), "texels": fmt,
            "lm_iteration_us_all_images": {"batched": stat(b_it, 1e3 / L), "separate": stat(s_it, 1e3 / L),
                                           "ratio": round(statistics.median(b_it) / statistics.median(s_it), 3)},
            "polish_%d_iters_ms_per_image" % P: {"batched": stat(bp, 1.0 / (L * I)), "separate": stat(sp, 1.0 / (L * I)),
                                                 "ratio": round(statistics.median(bp) / statistics.median(sp), 3)},
            "status_0": int((res["status"] == 0).sum()), "rows_equal_the_single_calls": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--polish", type=int, default=5)
    args = ap.parse_args()
    out = {"shipped_shared": shape(166_667, 8, False, args), "shipped_colour_sets": shape(166_667, 8, True, args),
           "cfg2_shared": shape(1_000_000, 5, False, args)}
    out["note"] = ("host call to completion of %d back-to-back polishes of all images, outputs and workspace allocated per call; an LM iteration is "
                   "(a call of %d iterations - a call of 0) / %d; batched: one gauss_newton_refine_images_at_winners, separate: one "
                   "gauss_newton_refine_at_winners per image" % (args.launches, args.iters, args.iters))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
