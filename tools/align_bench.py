#!/usr/bin/env python3
"""Alignment stages: what moments, normals and the vote cost against a torch-only composition.

  VoxelGrid.moments, ops.voxel_normals_of and ops.align_vote (with the wall direction) at 166,667, 1M and 10M points of synth.scanned_room,
  10 cm voxels, against torch alone in the same process — index_add_ of float64 offsets and outer products per voxel for the moments, the
  covariance and a batched torch.linalg.eigh for the normals; torch has no counterpart of the vote, which is timed alone —, timed
  alternately after a warm-up of every shape: a sample is a loop of back-to-back calls at least 50 ms long between two device
  synchronises, reported per call, median of --reps samples with the spread (moments and the vote read a word back per call: that is
  part of the operation).  The torch composition sums in float64 about the voxel's first point: its normals are compared, not its bits.

    python tools/align_bench.py [--reps 9] [--voxel 0.1] [--sizes 166667,1000000,10000000] [--min-count 8]

Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from piccolo_amd import ops, synth  # noqa: E402
from voxel_bench import timed  # noqa: E402  (tools/ is the script's directory)


def torch_moments(X, cell, first, V):
    """(S1 (V, 3), S2 (V, 3, 3)) float64 about the voxel's first point"""
    idx = cell.long()
    d = X.double() - X.double()[first][idx]
    s1 = torch.zeros(V, 3, dtype=torch.float64, device=X.device).index_add_(0, idx, d)
    s2 = torch.zeros(V, 9, dtype=torch.float64, device=X.device).index_add_(0, idx, (d[:, :, None] * d[:, None, :]).reshape(-1, 9))
    return s1, s2.view(V, 3, 3)


def torch_normals(s1, s2, count, min_count):
    c = count.double()[:, None, None]
    cov = s2 / c - (s1[:, :, None] * s1[:, None, :]) / (c * c)
    lam, vec = torch.linalg.eigh(cov)
    ok = (count >= min_count) & (lam[:, 2] > 0)
    normal = torch.where(ok[:, None], vec[:, :, 0], torch.zeros_like(vec[:, :, 0]))
    planarity = torch.where(ok, (lam[:, 1] - lam[:, 0]) / lam[:, 2].clamp_min(1e-300), torch.zeros_like(lam[:, 0]))
    return normal.float(), planarity.float()


def operations(n, voxel, min_count, reps):
    X = torch.from_numpy(synth.scanned_room(n, seed=1)[0]).cuda()
    g = ops.VoxelGrid(X, voxel)
    V = g.nvoxels
    m = g.moments()
    normal, planarity = ops.voxel_normals_of(m, g.count, min_count)
    s1, s2 = torch_moments(X, g.cell, g.first, V)
    t_normal, t_planarity = torch_normals(s1, s2, g.count, min_count)
    fit = planarity > 1e-3
    cos = (normal[fit] * t_normal[fit]).sum(dim=1).abs().clamp(max=1.0)
    fns = [lambda: g.moments(), lambda: torch_moments(X, g.cell, g.first, V), lambda: ops.voxel_normals_of(m, g.count, min_count),
           lambda: torch_normals(s1, s2, g.count, min_count), lambda: ops.align_vote(normal, planarity, g.count, yaw=True)]
    for f in fns:                                       # warm-up of every shape the timed window uses
        f()
        f()
    hip_m, th_m, hip_n, th_n, hip_v = timed(fns, reps)
    info = ops.align_vote(normal, planarity, g.count, yaw=True)
    return {"points": n, "voxel": voxel, "voxels": V, "fitted_voxels": int((planarity > 0).sum()),
            "normals_max_angle_vs_torch_rad": float(torch.acos(cos).max()) if cos.numel() else None,
            "planarity_max_abs_diff_vs_torch": float((planarity - t_planarity).abs().max()),
            "tilt_deg": round(float(torch.rad2deg(torch.tensor(info["tilt"]))), 4), "status": info["status"],
            "moments_us": {"hip": hip_m, "torch": th_m}, "normals_us": {"hip": hip_n, "torch": th_n}, "vote_us": {"hip": hip_v}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--min-count", type=int, default=8)
    ap.add_argument("--sizes", default="166667,1000000,10000000")
    args = ap.parse_args()
    out = {"tool": "align_bench", "window_ms": 50.0, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "operations": [operations(int(n), args.voxel, args.min_count, args.reps) for n in args.sizes.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
