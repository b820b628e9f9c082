#!/usr/bin/env python3
"""Score maps: what the two launches cost, where the table should live, and whether the weights help.

  launches  ops.score_maps (prepare + points launch) and ops.score_weight_plane against the histogram stage that precedes them
            (ops.hist_trim_scores at the same poses and split), at the shipped shape (166,667 points, 50 poses) and at cfg-2 size
            (1M points, 64 poses), 2048 x 1024, splits 4 x 4 and 16 x 32; the L2-resident global table (shipped) against chunks of poses
            staged in LDS (experiments build, PCL_SCORE_LDS=1) in the same process, timed alternately, median of --reps with the spread
  accuracy  --rooms synthetic box rooms with a planted change — a region of the cloud recoloured with uniform random colours AFTER the
            query was rendered —, each initialised with make_input_scored and refined from the same starting poses with and without
            omniloc.score_weights of its maps: median and mean translation / rotation error of either

    python tools/score_map_bench.py [--reps 9] [--rooms 32] [--skip-accuracy] [--skip-launches]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PCL_SCORE_LDS", "0")      # (a C knob: tools/_knobs.py then loads the experiments build, the only one that has the LDS form)
import _knobs  # noqa: E402,F401

import numpy as np  # noqa: E402
import torch  # noqa: E402

from piccolo_amd import omniloc as po, ops, synth, utils  # noqa: E402
from piccolo_amd.localize import pose_errors  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fns, reps):
    """every function timed in turn, `reps` rounds -> [{median, min, max} in us]"""
    runs = [[] for _ in fns]
    for _ in range(reps):
        for r, f in zip(runs, fns):
            r.append(once(f))
    return [{"median": round(1e3 * statistics.median(r), 1), "min": round(1e3 * min(r), 1), "max": round(1e3 * max(r), 1)} for r in runs]


def launches(n, K, reps):
    H, W = 1024, 2048
    xyz, rgb = synth.box_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    t_gt, ypr = synth.gt_pose(1)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
    tr, ro = synth.start_poses(t_gt, ypr, K, seed=1, sigma_t=0.5, sigma_r=0.4)
    tr, ro = torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()
    cloud = ops.Cloud(X, C)
    out = {}
    for nsh, nsw in ((4, 4), (16, 32)):
        _, inter, nproj, nimg = ops.hist_trim_scores(img, cloud, tr, ro, nsh, nsw, return_parts=True)
        s3, c3, _, _ = ops.score_maps(cloud, tr, ro, H, W, nsh, nsw, inter, nproj, nimg, packed=True)

        def maps(lds):
            def f():
                os.environ["PCL_SCORE_LDS"] = lds
                ops.score_maps(cloud, tr, ro, H, W, nsh, nsw, inter, nproj, nimg, packed=True)
            return f
        fns = [lambda: ops.hist_trim_scores(img, cloud, tr, ro, nsh, nsw, return_parts=True), maps("0"), maps("1"),
               lambda: ops.score_weight_plane(n, s3, c3)]
        for f in fns:
            f()
        os.environ["PCL_SCORE_LDS"] = "1"
        lds = ops.score_maps(cloud, tr, ro, H, W, nsh, nsw, inter, nproj, nimg, packed=True)
        os.environ["PCL_SCORE_LDS"] = "0"
        same = bool(torch.equal(lds[0], s3) and torch.equal(lds[1], c3))
        hist, glob, ldst, plane = timed(fns, reps)
        out["%dx%d" % (nsh, nsw)] = {"hist_stage_us": hist, "score_maps_global_table_us": glob, "score_maps_lds_chunks_us": ldst,
                                    "score_weight_plane_us": plane, "lds_equals_global_bit_for_bit": same,
                                    "voted_share": round(float((c3 > 0).float().mean()), 4)}
    return out


INIT = dict(max_yaw=2 * np.pi, min_yaw=0, max_pitch=2 * np.pi, min_pitch=0, max_roll=2 * np.pi, min_roll=0, z_prior=None, sample_rate_for_init=None,
            trans_init_mode="quantile", x_max=None, x_min=None, y_max=None, y_min=None, z_max=None, z_min=None, num_split_h=4, num_split_w=4,
            xy_only=False, num_trans=50, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4, dataset="Stanford2D-3D-S")


class Cfg:
    lr, num_iter, patience, factor, out_of_room_quantile, num_input, parallel = 0.1, 100, 5, 0.8, 0.05, 6, True


def accuracy(rooms, n, H, W, split, share, floor):
    errs = {"plain": [], "scored": []}
    changed_w, kept_w = [], []
    for k in range(rooms):
        xyz, rgb = synth.box_room(n, seed=100 + k)
        t_gt, ypr = synth.gt_pose(100 + k)
        X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
        img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
        # the planted change: the points of one corner region of the room (about `share` of the cloud) recoloured after the render
        rng = np.random.default_rng(100 + k)
        lo, hi = xyz.min(axis=0), xyz.max(axis=0)
        corner = (xyz[:, 0] > lo[0] + (1.0 - 2.0 * share) * (hi[0] - lo[0])) & (xyz[:, 1] > lo[1] + 0.5 * (hi[1] - lo[1]))
        rgb2 = rgb.copy()
        rgb2[corner] = rng.uniform(0.0, 1.0, size=(int(corner.sum()), 3)).astype(np.float32)
        C2 = torch.from_numpy(rgb2).cuda()
        tr, ro, maps = utils.make_input_scored(img, X, C2, Cfg.num_input, dict(INIT), "loss_histogram", 64, score_split=split)
        w = po.score_weights(maps, floor=floor)
        changed_w.append(float(w[torch.from_numpy(corner).cuda()].mean()))
        kept_w.append(float(w[torch.from_numpy(~corner).cuda()].mean()))
        for name, weights in (("plain", None), ("scored", w)):
            t, R, _ = po.omniloc_batch(img, X, C2, tr.clone(), ro.clone(), Cfg, {}, weights=weights)
            errs[name].append(pose_errors(t, R, t_gt, synth.rot_from_ypr_np(ypr)))
    out = {"rooms": rooms, "points": n, "pano": [H, W], "score_split": list(split), "changed_share": share, "floor": floor,
           "mean_weight_changed_region": round(float(np.mean(changed_w)), 4), "mean_weight_elsewhere": round(float(np.mean(kept_w)), 4)}
    for name, e in errs.items():
        e = np.asarray(e, np.float64)
        out[name] = {"t_err_m_median": round(float(np.median(e[:, 0])), 4), "t_err_m_mean": round(float(e[:, 0].mean()), 4),
                     "r_err_deg_median": round(float(np.median(e[:, 1])), 4), "r_err_deg_mean": round(float(e[:, 1].mean()), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--skip-accuracy", action="store_true")
    ap.add_argument("--skip-launches", action="store_true")
    args = ap.parse_args()
    out = {"tool": "score_map_bench", "library": os.environ.get("PCL_SO", "shipped")}
    if not args.skip_launches:
        out["shipped_167k_x50"] = launches(166_667, 50, args.reps)
        out["cfg2_1M_x64"] = launches(1_000_000, 64, args.reps)
    if not args.skip_accuracy:
        out["accuracy"] = accuracy(args.rooms, 40_000, 256, 512, (16, 32), 0.2, 0.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
