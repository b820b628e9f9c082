#!/usr/bin/env python3
"""The panorama pyramid and the coarse-to-fine chain on the MI355X.  Medians over --reps loops of at least 50 ms each.

(a) Build time: ONE pcl_pano_pyramid call (ops.PanoPyramid over a packed level 0, float images off) at 2048 x 1024 and 4096 x 2048 for
    1 .. 4 levels against the composition it replaces: the rule in torch ops on the device, level by level, plus one ops.Pano per level.
(b) Iteration time per level: us per GD iteration of a plain engine over level 0, 1, 2 of a 2048 x 1024 panorama at cfg 2 (1M points x 32
    candidates) and at the shipped shape (166,667 x 6), refine_texels' format per level, for poses spread all over the room (what
    make_input hands over) and for poses near the truth.
(c) Pose error: median translation / rotation error and the reference's success count (0.1 m, 5 degrees) over --seeds synth scenes at both
    shapes, starting poses synth.start_poses with (sigma_t, sigma_r) = (0.3, 0.15) — today's —, (0.6, 0.3) and (1.0, 0.6), the same total
    num_iter = 100 for every variant: the plain chain, one coarse level (pyramid_iters = 30) and two (10, 30), each with and without
    pyramid_reset.

Not a test and not part of bench.py.  Nothing is promised about which variant wins, and nothing about real data.

    python tools/pyramid_bench.py [--parts abc] [--reps 7] [--seeds 32]

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
SHAPES = (("cfg2", 1_000_000, 32), ("shipped", 166_667, 6))


class Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def loop_ms(fn, reps):
    """median, min, max ms per call of fn over `reps` loops, each as many calls as fill 50 ms"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    count = max(1, int(0.05 / max(time.perf_counter() - t0, 1e-6)) + 1)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / count)
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "calls_per_loop": count}


def scene_image(n, seed, h=H, w=W):
    xyz, rgb = synth.box_room(n, seed=seed)
    X, C = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    t_gt, ypr = synth.gt_pose(seed)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, torch.from_numpy(t_gt), torch.from_numpy(ypr)), C, (h, w)))
    return X, C, img, t_gt, ypr


def torch_level(k):
    """the rule in torch ops: (h, w, 3) int32 levels -> (h / 2, w / 2, 3)"""
    h, w = k.shape[0] // 2, k.shape[1] // 2
    b = k.view(h, 2, w, 2, 3).permute(0, 2, 1, 3, 4).reshape(h, w, 4, 3)
    cnt = (b != 0).any(dim=3).sum(dim=2)
    sums = b.sum(dim=2)
    c = cnt.clamp(min=1).unsqueeze(2)
    out = torch.div(sums + torch.div(c, 2, rounding_mode="floor"), c, rounding_mode="floor")
    fix = (cnt > 0) & ~out.any(dim=2)
    out = torch.where(fix.unsqueeze(2), (sums == sums.max(dim=2, keepdim=True).values).to(out.dtype), out)
    return torch.where((cnt == 0).unsqueeze(2), torch.zeros_like(out), out)


def build_times(args):
    out = {}
    lut = (torch.arange(256, dtype=torch.float32) / 255.0).cuda()
    for h, w in ((1024, 2048), (2048, 4096)):
        _, _, img, _, _ = scene_image(1_000_000, 3, h, w)
        p0 = ops.Pano(img)
        for levels in (1, 2, 3, 4):
            def kernel():
                ops.PanoPyramid(img, levels, fmts="f16", pano0=p0)

            def composition():
                k = torch.round(img * 255.0).to(torch.int32)
                for _ in range(levels):
                    k = torch_level(k)
                    ops.Pano(synth.mark_levels(lut[k.long()]), fmt="f16")
            a, b = loop_ms(kernel, args.reps), loop_ms(composition, args.reps)
            # the two agree (the composition is the model's rule once more)
            pyr = ops.PanoPyramid(img, levels, fmts="f16", pano0=p0, images=True)
            k = torch.round(img * 255.0).to(torch.int32)
            for l in range(levels):
                k = torch_level(k)
                assert torch.equal(pyr.images[l], lut[k.long()]), (h, w, l)
            out["%dx%d_levels%d" % (w, h, levels)] = {"pyramid_call_ms": a, "torch_rule_plus_pack_ms": b, "ratio": round(b["median"] / a["median"], 2)}
            print(json.dumps({"%dx%d_levels%d" % (w, h, levels): out["%dx%d_levels%d" % (w, h, levels)]}), file=sys.stderr, flush=True)
    return out


def spread_poses(B, seed):
    rng = np.random.default_rng(seed)
    trans = ((rng.random((B, 3)) - 0.5) * 0.8 * synth.ROOM).astype(np.float32)
    rot = np.stack([rng.uniform(-np.pi, np.pi, B), rng.normal(0, 0.1, B), rng.normal(0, 0.1, B)], axis=1).astype(np.float32)
    return trans, rot


def iteration_times(args):
    out, iters = {}, 20
    for name, n, B in SHAPES:
        X, C, img, t_gt, ypr = scene_image(n, 5)
        cloud, box = ops.Cloud(X, C), ops.quantile_box(X, 0.05)
        pyr = ops.PanoPyramid(img, 2, n=n, pano0=ops.Pano(img, fmt=ops.refine_texels(n, H, W)))
        for kind, (tr, ro) in (("spread", spread_poses(B, 7)), ("near", synth.start_poses(t_gt, ypr, B, seed=7, sigma_t=0.05, sigma_r=0.02))):
            for l in (0, 1, 2):
                gd = ops.GradientDescent(cloud, pyr.panos[l], torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda(), box, lr=1e-12)

                def run():
                    gd.run_graph(iters)                    # (a vanishing lr: every iteration evaluates the same poses)
                r = loop_ms(run, args.reps)
                out["%s_%s_level%d" % (name, kind, l)] = {"us_per_iteration": round(r["median"] * 1e3 / iters, 2), "min": round(r["min"] * 1e3 / iters, 2),
                                                          "max": round(r["max"] * 1e3 / iters, 2), "texels": {0: "f32", 1: "u8", 2: "f16"}[pyr.panos[l].fmt]}
                print(json.dumps({"%s_%s_level%d" % (name, kind, l): out["%s_%s_level%d" % (name, kind, l)]}), file=sys.stderr, flush=True)
    return out


VARIANTS = (("plain", {}), ("one_level", dict(pyramid_iters=30)), ("one_level_reset", dict(pyramid_iters=30, pyramid_reset=True)),
            ("two_levels", dict(pyramid_iters=[10, 30])), ("two_levels_reset", dict(pyramid_iters=[10, 30], pyramid_reset=True)))
SCATTERS = ((0.3, 0.15), (0.6, 0.3), (1.0, 0.6))


def pose_errors(args):
    out = {}
    for name, n, B in SHAPES:
        base = dict(lr=0.1, num_iter=100, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=B)
        rows = {(sc, key): [] for sc in SCATTERS for key, _ in VARIANTS}
        for s in range(args.seeds):
            seed = 300 + s
            X, C, img, t_gt, ypr = scene_image(n, seed)
            R_gt = synth.rot_from_ypr_np(ypr)
            for sc in SCATTERS:
                trans, rot = synth.start_poses(t_gt, ypr, B, seed=seed, sigma_t=sc[0], sigma_r=sc[1])
                for key, kw in VARIANTS:
                    t, r = torch.from_numpy(trans.copy()).cuda(), torch.from_numpy(rot.copy()).cuda()
                    res = po.omniloc_batch(img, X, C, t, r, Cfg(**base, **kw), {})
                    rows[(sc, key)].append(synth.pose_errors(res[0].numpy().reshape(3), res[1].numpy(), t_gt, R_gt) + (float(res[2]),))
            po._cache.clear()
        out[name] = {"images": args.seeds, "candidates": B}
        for sc in SCATTERS:
            cell = {}
            for key, _ in VARIANTS:
                r = np.array(rows[(sc, key)])
                cell[key] = {"t_err_m_median": round(float(np.median(r[:, 0])), 5), "r_err_deg_median": round(float(np.median(r[:, 1])), 4),
                             "success": int(((r[:, 0] < 0.1) & (r[:, 1] < 5.0)).sum()), "loss_median": round(float(np.median(r[:, 2])), 6)}
            out[name]["sigma_t%.1f_r%.2f" % sc] = cell
            print(json.dumps({name: {"sigma_t%.1f_r%.2f" % sc: cell}}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seeds", type=int, default=32)
    args = ap.parse_args()
    out = {}
    if "a" in args.parts:
        out["build"] = build_times(args)
    if "b" in args.parts:
        out["iteration"] = iteration_times(args)
    if "c" in args.parts:
        out["pose_error"] = pose_errors(args)
    out["note"] = ("medians over %d loops of at least 50 ms; build: host call to completion, buffers allocated per call; iteration: a replayed graph of "
                   "20 iterations at lr 0; pose error: omniloc_batch, num_iter 100 for every variant, success = below 0.1 m and 5 degrees" % args.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
