#!/usr/bin/env python3
"""Pose information timing: pcl_pose_information (its two launches) against the loss launch with gradient,
pcl_sampling_loss, of the same build at the same shape — B = 1 and B = 32 poses, at the shipped shape (166,667 points) and at cfg 2
(1M points), 2048 x 1024 panorama, the refinement's texel format; unweighted and with a weight plane.

Each group is timed alternately (A B C A B C ...), `--launches` back-to-back calls per timed run, median of --reps runs with the spread
(min .. max).  Not part of bench.py: the call runs once per image, after the refinement.

    python tools/info_bench.py [--reps 9] [--launches 50]

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
    return {"median": round(1e3 * t[0] / per, 2), "min": round(1e3 * t[1] / per, 2), "max": round(1e3 * t[2] / per, 2)}


def shape(n, args):
    H, W = 1024, 2048
    xyz, rgb = synth.box_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    t_gt, ypr = synth.gt_pose(1)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
    cloud = ops.Cloud(X, C)
    weighted = cloud.weighted_view(torch.ones(ops._lib.load().pcl_cloud_stride(n), dtype=torch.float32, device="cuda"))
    pano = ops.Pano(img, fmt=ops.refine_texels(n, H, W))
    L, out = args.launches, {"points": n, "texels": pano.fmt}
    for B in (1, 32):
        tr, ro = synth.start_poses(t_gt, ypr, B, seed=1)
        tr, ro = torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()

        def many(f):
            def g():
                for _ in range(L):
                    f()
            return g
        loss = many(lambda: ops.sampling_loss(cloud, pano, tr, ro, with_grad=True))
        info = many(lambda: ops.pose_information(cloud, pano, tr, ro))
        info_w = many(lambda: ops.pose_information(weighted, pano, tr, ro))
        for f in (loss, info, info_w):
            f()
        tl, ti, tw = timed([loss, info, info_w], args.reps)
        status = ops.pose_information(cloud, pano, tr, ro)[2][:, 4]
        out["B%d" % B] = {"sampling_loss_with_grad_us": stat(tl, L), "pose_information_us": stat(ti, L), "pose_information_weighted_us": stat(tw, L),
                          "ratio": round(ti[0] / tl[0], 3), "status_0": int((status == 0).sum())}
    out["note"] = "host call to completion of %d back-to-back calls, per call (allocation of the outputs and the workspace included)" % L
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    out = {"shipped": shape(166_667, args), "cfg2": shape(1_000_000, args)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
