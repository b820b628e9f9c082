#!/usr/bin/env python3
"""The LM polish and the pose information under the depth mask: what they cost next to the plain forms of the same build,
and what cfg.depth_polish does to the pose error of the depth chain.  synth.furnished_room at the shipped shape (166,667 points) and at
cfg 2 (1M points), 2048 x 1024 panorama, the refinement's texel format, the default depth grid, tolerance and stride.

(a) us per LM evaluation under the mask and plain, B = 1 and B = 32 ((a call of --iters iterations - a call of 0) / --iters), and us per
    pose_information call under the mask and plain; timed alternately, median of --reps runs of --launches back-to-back calls with the
    spread.  Start poses far from the minimum, so that none freezes.
(b) the split of a masked pose_information call: the z pass alone (ops.depth_mask on the same grid: records, fill, z pass and a mark pass)
    against the whole call; the point pass is what is left.
(c) over --seeds furnished_room scenes: omniloc_batch with cfg.depth_mask, with and without cfg.depth_polish + gn_iters = 5: median
    translation / rotation error against the ground truth, ms per image (the second of two runs) and the share of images where the
    polish accepted a step.

Not a test and not part of bench.py.  Nothing is asserted.

    python tools/depth_polish_bench.py [--reps 9] [--launches 20] [--iters 10] [--seeds 32] [--shapes shipped,cfg2]

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

from piccolo_amd import omniloc as po  # noqa: E402
from piccolo_amd import ops, synth  # noqa: E402

H, W = 1024, 2048


class Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


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


def stat(ms, per):
    return {"median": round(1e3 * statistics.median(ms) / per, 2), "min": round(1e3 * min(ms) / per, 2), "max": round(1e3 * max(ms) / per, 2)}


def scene(n, seed):
    xyz, rgb = synth.furnished_room(n, seed=seed)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    t_gt, ypr = synth.gt_pose(seed)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
    return X, C, img, t_gt, ypr


def evaluation_cost(n, args):
    X, C, img, t_gt, ypr = scene(n, 1)
    cloud, pano = ops.Cloud(X, C), ops.Pano(img, fmt=ops.refine_texels(n, H, W))
    dh, dw, tau, st = ops.default_depth(n, H, W)
    L, K = args.launches, args.iters
    out = {"depth_grid": [dh, dw], "depth_tau": round(tau, 4), "depth_stride": st}
    for B in (1, 32):
        tr, ro = synth.start_poses(t_gt, ypr, B, seed=1)
        tr, ro = torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()

        def many(f):
            def g():
                for _ in range(L):
                    f()
            return g
        fns = [many(lambda: ops.pose_information(cloud, pano, tr, ro)), many(lambda: ops.pose_information(cloud, pano, tr, ro, depth=True)),
               many(lambda: ops.depth_mask(cloud, tr, ro, (dh, dw), tau=tau, stride=st)),
               many(lambda: ops.gauss_newton_refine(cloud, pano, tr, ro, iters=0)), many(lambda: ops.gauss_newton_refine(cloud, pano, tr, ro, iters=K)),
               many(lambda: ops.gauss_newton_refine(cloud, pano, tr, ro, iters=0, depth=True)),
               many(lambda: ops.gauss_newton_refine(cloud, pano, tr, ro, iters=K, depth=True))]
        for f in fns:
            f()
        ti, tid, tz, p0, pk, d0, dk = timed(fns, args.reps)
        plain = [(a - b) / K for a, b in zip(pk, p0)]
        masked = [(a - b) / K for a, b in zip(dk, d0)]
        res = ops.gauss_newton_refine(cloud, pano, tr, ro, iters=K, depth=True)
        out["B%d" % B] = {"pose_information_us": stat(ti, L), "pose_information_depth_us": stat(tid, L),
                          "depth_mask_call_us (records + fill + z pass + mark pass)": stat(tz, L),
                          "lm_evaluation_us": stat(plain, L), "lm_evaluation_depth_us": stat(masked, L),
                          "masked_to_plain_evaluation": round(statistics.median(masked) / statistics.median(plain), 3),
                          "masked_to_plain_pose_information": round(statistics.median(tid) / statistics.median(ti), 3),
                          "status_0": int((res["status"] == 0).sum()), "accepted_mean": round(float(res["accepted"].mean()), 2)}
    return out


def polish_effect(n, B, args):
    base = dict(lr=0.1, num_iter=100, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=B, depth_mask=True)
    rows = {"depth chain": [], "depth chain + depth_polish": []}
    took = []
    for s in range(args.seeds):
        seed = 300 + s
        X, C, img, t_gt, ypr = scene(n, seed)
        R_gt = synth.rot_from_ypr_np(ypr)
        trans, rot = synth.start_poses(t_gt, ypr, B, seed=seed)
        ts = {}
        for key, cfg in (("depth chain", Cfg(**base)), ("depth chain + depth_polish", Cfg(depth_polish=True, gn_iters=5, **base))):
            ms = None
            for _ in range(2):
                t, r = torch.from_numpy(trans.copy()).cuda(), torch.from_numpy(rot.copy()).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = po.omniloc_batch(img, X, C, t, r, cfg, {})
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            rows[key].append(synth.pose_errors(res[0].numpy().reshape(3), res[1].numpy(), t_gt, R_gt) + (ms, float(res[2])))
            ts[key] = res[0].clone()
        took.append(not torch.equal(ts["depth chain"], ts["depth chain + depth_polish"]))      # (no accepted step: the chain's own entries)
        po._cache.clear()
    out = {"images": args.seeds, "candidates": B, "share_with_an_accepted_step": round(float(np.mean(took)), 3)}
    for key, r in rows.items():
        r = np.array(r)
        out[key] = {"t_err_m_median": round(float(np.median(r[:, 0])), 5), "r_err_deg_median": round(float(np.median(r[:, 1])), 4),
                    "t_err_m_mean": round(float(r[:, 0].mean()), 5), "ms_per_image_median": round(float(np.median(r[:, 2])), 3),
                    "loss_median": round(float(np.median(r[:, 3])), 6)}
    a, b = np.array(rows["depth chain"]), np.array(rows["depth chain + depth_polish"])
    out["images_where_t_err_fell"] = int((b[:, 0] < a[:, 0]).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--shapes", default="shipped,cfg2")
    args = ap.parse_args()
    out = {}
    for name, n, B in (("shipped", 166_667, 6), ("cfg2", 1_000_000, 32)):
        if name not in args.shapes.split(","):
            continue
        out[name] = {"points": n, "evaluation": evaluation_cost(n, args)}
        if name == "shipped" and args.seeds > 0:
            out[name]["polish"] = polish_effect(n, B, args)
    out["note"] = ("evaluation: host call to completion of %d back-to-back calls, per call, outputs and workspace allocated per call; an LM evaluation "
                   "is (a call of %d iterations - a call of 0) / %d; under the mask it is records + fill + z pass + gated pass + step"
                   % (args.launches, args.iters, args.iters))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
