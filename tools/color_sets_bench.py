#!/usr/bin/env python3
"""Per-image cloud colours (sharpen_color: color_mod gives every query image its own equalised colours) — one image at a time against
the images of a room sharing their launches through per-image colour sets (experiment aid, modelled on tools/pipe8.py).

    python tools/color_sets_bench.py [n_points] [H] [W] [num_input] [num_intermediate] [images] [groups]

Per query image, ms (medians over `groups` groups of `images` images after one untimed group; (a) and (b) alternate inside every group):
  (a) today's path: color_mod, make_input + omniloc_batch, one image at a time (what the batcher did with per-image colours);
  (b) color_mod of every image, then make_input_images + omniloc_batch_images with the list of per-image colours (colour sets);
  (c) the shared-colour batched path (no color_mod: one rgb for all images), the reference point.
Also checks that (a) and (b) return the same tensors (starting poses and refined poses), bit for bit."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from piccolo_amd import omniloc as po
from piccolo_amd import _lib, ops, utils

argv = [int(a) for a in sys.argv[1:]]
N, H, W, NUM_INPUT, NUM_MID, IPL, GROUPS = (argv + [166_667, 1024, 2048, 6, 50, 8, 3][len(argv):])[:7]


class Cfg:
    lr, num_iter, patience, factor, out_of_room_quantile = bench.LR, bench.NUM_ITER, bench.PATIENCE, bench.FACTOR, bench.QUANTILE
    num_input = NUM_INPUT


sc = bench.Scene(N, H, W, torch.device("cuda:0"))
init = bench.STANFORD_INIT


def path_a(imgs):
    out = []
    for img in imgs:
        img_eq, c = ops.color_mod(img, sc.C, 256)
        tr, ro = utils.make_input(img_eq, sc.X, c, NUM_INPUT, init, "loss_histogram", NUM_MID)
        st = (tr.clone(), ro.clone())
        out.append((st, po.omniloc_batch(img, sc.X, c, tr, ro, Cfg(), {})))
    return out


def path_b(imgs):
    eq = [ops.color_mod(img, sc.C, 256) for img in imgs]
    starts = utils.make_input_images([e[0] for e in eq], sc.X, [e[1] for e in eq], NUM_INPUT, init, "loss_histogram", NUM_MID)
    st = [(a.clone(), b.clone()) for a, b in starts]
    res = po.omniloc_batch_images(imgs, sc.X, [e[1] for e in eq], [s[0] for s in starts], [s[1] for s in starts], Cfg())
    return list(zip(st, res))


def path_c(imgs):
    starts = utils.make_input_images(imgs, sc.X, sc.C, NUM_INPUT, init, "loss_histogram", NUM_MID)
    return po.omniloc_batch_images(imgs, sc.X, sc.C, [s[0] for s in starts], [s[1] for s in starts], Cfg())


def timed(fn, imgs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(imgs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(imgs), out


ms = {"a": [], "b": [], "c": []}
same = True
for g in range(GROUPS + 1):
    imgs = [sc.image(5_000_000 + g * IPL + j, keep_img=True).pop("img") for j in range(IPL)]
    order = ("a", "b", "c") if g % 2 == 0 else ("b", "a", "c")
    outs = {}
    for k in order:
        t, outs[k] = timed({"a": path_a, "b": path_b, "c": path_c}[k], imgs)
        if g > 0:
            ms[k].append(t)
    for (sa, ra), (sb, rb) in zip(outs["a"], outs["b"]):
        same = same and all(torch.equal(x, y) for x, y in zip(sa, sb)) and all(torch.equal(x, y) for x, y in zip(ra, rb))
    for k in ms:
        del outs[k]

plan = {}
for B, sets in ((NUM_INPUT, 1), (NUM_INPUT * IPL, IPL), (NUM_INPUT * IPL, 1)):
    h = _lib.GdHyper(0.1, 0.8, 5, 1, 0, 0.0, 0, 0, 0, 0, IPL if sets > 1 else 0, sets)
    c, gp, f = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().pcl_gd_plan_hyper(N, B, ctypes.byref(h), ctypes.byref(c), ctypes.byref(gp), ctypes.byref(f))
    plan["%d candidates, %d colour set(s)" % (B, sets)] = {"chunks": c.value, "poses_per_block": gp.value, "fused": f.value,
                                                             "blocks": c.value * B // gp.value}
print(json.dumps({"what": "ms per query image, %d points, %dx%d, %d candidates (%d intermediate), %d images per group, medians over %d groups"
                          % (N, W, H, NUM_INPUT, NUM_MID, IPL, GROUPS),
                  "a_one_by_one_ms": float(np.median(ms["a"])), "b_color_sets_ms": float(np.median(ms["b"])),
                  "c_shared_colours_ms": float(np.median(ms["c"])), "b_over_a": float(np.median(ms["b"]) / np.median(ms["a"])),
                  "a_runs": ms["a"], "b_runs": ms["b"], "c_runs": ms["c"], "a_equals_b": bool(same), "refine_plans": plan}, indent=1))
