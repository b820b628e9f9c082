#!/usr/bin/env python3
"""Voxel grid: what the three operations cost against a torch-only composition, and whether density weights or a
voxel-down-sampled cloud change the pose error on density-skewed scenes.

  ops       ops.VoxelGrid (grid), .centroids and .weights at 166,667, 1M and 10M points of synth.scanned_room, 2 cm and 5 cm voxels, against
            the torch-only composition in the same process — the packed 63-bit keys, torch.unique(sorted, return_inverse, return_counts),
            first points by scatter_reduce(amin), the first-occurrence renumbering, index_add_ of float64 values, count gather and divide —,
            timed alternately after a warm-up of every shape: a sample is a loop of back-to-back calls at least 50 ms long between two device
            synchronises, reported per call, median of --reps samples with the spread (the grid and the centroids read a word back per call:
            that is part of the operation).
            The torch composition sums in float64, so its centroids are NOT the rule's bits; it is a yardstick for time only.
  accuracy  --rooms scanned_room scenes at the shipped shape (166,667 points, 6 candidates) and at cfg 2's (1M points, 32 candidates), 2048 x 1024,
            100 iterations, each localised the way the dataset loops do it — make_input, then omniloc_batch from its starting poses — on (a) the plain
            cloud, (b) the plain cloud with the refinement under density_weights(voxel) (the initialisation takes no weights), (c) the cloud
            voxel_downsample(voxel) leaves, which has as many points as (b) has voxels: median / mean pose error and ms per image
            (make_input + omniloc_batch from empty pack caches — each figure includes sorting and packing the variant's cloud and packing the
            panorama —, timed after one untimed image; the grid itself is paid once per room and timed under `ops`).

    python tools/voxel_bench.py [--reps 9] [--rooms 32] [--voxel 0.05] [--sizes 166667,1000000,10000000] [--shapes shipped,cfg2]
                                 [--skip-accuracy] [--skip-ops]

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

from piccolo_amd import omniloc as po, ops, synth, utils  # noqa: E402
from piccolo_amd.localize import pose_errors  # noqa: E402


WINDOW_MS = 50.0       # a timed sample is a loop of calls at least this long: a single 30 us call would measure the clock and the launch


def once(fn, calls=1):
    """ms per call over `calls` back-to-back calls between two device synchronises"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def timed(fns, reps):
    """every function timed in turn, `reps` rounds of a WINDOW_MS loop each -> [{median, min, max} in us per call, calls per sample]"""
    calls = [max(1, int(np.ceil(WINDOW_MS / max(once(f, 3), 1e-3)))) for f in fns]
    runs = [[] for _ in fns]
    for _ in range(reps):
        for r, f, c in zip(runs, fns, calls):
            r.append(once(f, c))
    return [{"median": round(1e3 * statistics.median(r), 1), "min": round(1e3 * min(r), 1), "max": round(1e3 * max(r), 1), "calls_per_sample": c}
            for r, c in zip(runs, calls)]


# ------------------------------------------------------------------------------------------------ the torch-only yardstick
def torch_grid(X, voxel):
    """(cell, count, first) by torch alone, the library's numbering: voxels in first-occurrence order"""
    n = X.shape[0]
    c = torch.floor(X.double() / voxel).long() + (1 << 20)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, inverse, count = torch.unique(key, sorted=True, return_inverse=True, return_counts=True)
    V = count.numel()
    first = torch.full((V,), n, dtype=torch.int64, device=X.device).scatter_reduce_(0, inverse, torch.arange(n, device=X.device), "amin")
    by_first = torch.argsort(first)
    rank = torch.empty_like(by_first)
    rank[by_first] = torch.arange(V, device=X.device)
    return rank[inverse].int(), count[by_first].int(), first[by_first]


def torch_centroids(X, C, cell, count):
    V = count.numel()
    idx = cell.long()
    den = count.double()[:, None]
    sx = torch.zeros(V, 3, dtype=torch.float64, device=X.device).index_add_(0, idx, X.double())
    sc = torch.zeros(V, 3, dtype=torch.float64, device=X.device).index_add_(0, idx, C.double())
    return (sx / den).float(), (sc / den).float()


def torch_weights(cell, count, cap):
    cnt = count[cell.long()].double()
    return torch.where(cnt <= cap, torch.ones_like(cnt), cap / cnt).float()


def operations(n, voxel, reps):
    xyz, rgb = synth.scanned_room(n, seed=1)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    g = ops.VoxelGrid(X, voxel)
    t_cell, t_count, t_first = torch_grid(X, voxel)
    same = bool(torch.equal(g.cell, t_cell) and torch.equal(g.count, t_count) and torch.equal(g.first, t_first))
    hx, hc = g.centroids(C)
    tx, tc = torch_centroids(X, C, t_cell, t_count)
    fns = [lambda: ops.VoxelGrid(X, voxel), lambda: torch_grid(X, voxel), lambda: g.centroids(C), lambda: torch_centroids(X, C, t_cell, t_count),
           lambda: g.weights(1), lambda: torch_weights(t_cell, t_count, 1)]
    for f in fns:                                       # warm-up of every shape the timed window uses
        f()
        f()
    hip_grid, th_grid, hip_cen, th_cen, hip_w, th_w = timed(fns, reps)
    return {"points": n, "voxel": voxel, "voxels": g.nvoxels, "max_count": int(g.count.max()), "median_count": float(g.count.float().median()),
            "grid_equals_torch": same, "centroid_max_abs_diff_vs_torch_f64": float(max((hx - tx).abs().max(), (hc - tc).abs().max())),
            "weights_equal_torch": bool(torch.equal(g.weights(1), torch_weights(t_cell, t_count, 1))),
            "workspace_bytes_per_point": round(ops._lib.load().pcl_voxel_workspace_bytes(n) / n, 2),
            "grid_us": {"hip": hip_grid, "torch": th_grid}, "centroids_us": {"hip": hip_cen, "torch": th_cen},
            "weights_us": {"hip": hip_w, "torch": th_w}}


# ------------------------------------------------------------------------------------------------ pose error and time per image
INIT = dict(max_yaw=2 * np.pi, min_yaw=0, max_pitch=2 * np.pi, min_pitch=0, max_roll=2 * np.pi, min_roll=0, z_prior=None, sample_rate_for_init=None,
            trans_init_mode="quantile", x_max=None, x_min=None, y_max=None, y_min=None, z_max=None, z_min=None, num_split_h=4, num_split_w=4,
            xy_only=False, num_trans=50, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4, dataset="Stanford2D-3D-S")


class Cfg:
    lr, num_iter, patience, factor, out_of_room_quantile, num_input, parallel = 0.1, 100, 5, 0.8, 0.05, 6, True


SHAPES = {"shipped": (166_667, 6), "cfg2": (1_000_000, 32)}           # points, candidates


def accuracy(rooms, n, H, W, voxel, num_input):
    cfg = type("Cfg", (Cfg,), {"num_input": num_input})
    errs = {"plain": [], "density_weights": [], "voxel_size": []}
    ms = {k: [] for k in errs}
    kept = []
    for k in range(-1, rooms):                          # (room -1: the untimed first image — code objects, allocator, caches)
        seed = 200 + max(k, 0)
        xyz, rgb = synth.scanned_room(n, seed=seed)
        t_gt, ypr = synth.gt_pose(seed)
        X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
        img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (H, W)))
        dX, dC, _, _ = utils.voxel_downsample(X, C, voxel)
        w = utils.density_weights(X, voxel)
        kept.append(dX.shape[0] / n)
        for name, (cx, cc, weights) in (("plain", (X, C, None)), ("density_weights", (X, C, w)), ("voxel_size", (dX, dC, None))):
            def image():
                tr, ro = utils.make_input(img, cx, cc, cfg.num_input, dict(INIT), "loss_histogram", 64)
                return po.omniloc_batch(img, cx, cc, tr, ro, cfg, {}, weights=weights)
            po._cache.clear()                           # every variant packs its own cloud and panorama: none rides on another's caches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t, R, _ = image()
            torch.cuda.synchronize()
            if k >= 0:
                ms[name].append((time.perf_counter() - t0) * 1e3)
                errs[name].append(pose_errors(t, R, t_gt, synth.rot_from_ypr_np(ypr)))
    out = {"rooms": rooms, "points": n, "pano": [H, W], "voxel": voxel, "candidates": cfg.num_input, "num_iter": cfg.num_iter,
           "voxels_per_point": round(float(np.mean(kept)), 4)}
    for name, e in errs.items():
        e = np.asarray(e, np.float64)
        out[name] = {"t_err_m_median": round(float(np.median(e[:, 0])), 4), "t_err_m_mean": round(float(e[:, 0].mean()), 4),
                     "r_err_deg_median": round(float(np.median(e[:, 1])), 4), "r_err_deg_mean": round(float(e[:, 1].mean()), 4),
                     "ms_per_image_median": round(statistics.median(ms[name]), 2), "ms_per_image_min": round(min(ms[name]), 2),
                     "ms_per_image_max": round(max(ms[name]), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--sizes", default="166667,1000000,10000000")
    ap.add_argument("--shapes", default="shipped,cfg2")
    ap.add_argument("--skip-accuracy", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    args = ap.parse_args()
    out = {"tool": "voxel_bench"}
    if not args.skip_ops:
        out["ops"] = [operations(int(n), voxel, args.reps) for n in args.sizes.split(",") for voxel in (0.02, 0.05)]
    if not args.skip_accuracy:
        out["accuracy"] = {name: accuracy(args.rooms, SHAPES[name][0], 1024, 2048, args.voxel, SHAPES[name][1]) for name in args.shapes.split(",")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
