#!/usr/bin/env python3
"""The depth mask inside shared chains, timing.  With cfg.depth_mask the refinement of R rooms x I images runs
  (a) as it did before the depth chain existed, called explicitly — R x omniloc_batch (I = 1), R x omniloc_batch_images (shared colours,
      I > 1), R x I x omniloc_batch (per-image colours), I x omniloc_batch (colour sets of one room) — against
  (b) the shared depth chain: omniloc_batch_rooms / omniloc_batch_rooms_images / omniloc_batch_images with a list of colours.
Both forms are timed alternately (a b a b ...), medians of --reps in ms per (room, image), with form (a)'s spread between repeats.  Form (b)
must equal the R x I single calls bit for bit (asserted).  Form (a) is those very calls except with shared colours and I > 1, where
omniloc_batch_images cuts the cloud by the plan of all I images' candidates: equal bits are asserted there when that plan is the
single-image plan, else the largest difference of the returned losses is reported (`a_plan_differs`).

    python tools/depth_chain_bench.py [--reps 9] [--rooms 4,8] [--images 1,8] [--no-large] [--out file.json]

Shapes: rooms of 166,667 points x 6 candidates, 2048 x 1024, 100 iterations; colour sets alone at 166,667 x 6 x 8 images and at
1M x 32 x 5 images.  Prints one JSON object per line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from piccolo_amd import _lib, ops, synth  # noqa: E402
from piccolo_amd import omniloc as po  # noqa: E402


class Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed_ab(fa, fb, reps):
    a, b = [], []
    for _ in range(reps):
        a.append(once(fa))
        b.append(once(fb))
    return a, b


def summary(prefix, runs, units):
    per = [v / units for v in runs]
    med = statistics.median(per)
    return {prefix + "_ms": round(med, 3), prefix + "_min": round(min(per), 3), prefix + "_max": round(max(per), 3),
            prefix + "_spread": round((max(per) - min(per)) / med, 4)}


def scene(R, I, n, per_image, H, W, per_image_colours):
    rooms = [(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()) for x, c in synth.rooms_side_by_side([n] * R, seed=R)]
    imgs = []
    for i in range(I):
        r = i % R
        t_gt, ypr = synth.room_gt_pose(r, 1 + i)
        imgs.append(synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(rooms[r][0], torch.from_numpy(t_gt), torch.from_numpy(ypr)),
                                                                 rooms[r][1], (H, W))))
    starts = []
    for r in range(R):
        row = []
        for i in range(I):
            t, y = synth.room_gt_pose(r, 2 + r)
            tr, ro = synth.start_poses(t, y, per_image, seed=r + 37 * i, sigma_t=0.4, sigma_r=0.2)
            row.append((torch.from_numpy(tr).cuda(), torch.from_numpy(ro).cuda()))
        starts.append(row)
    if per_image_colours:                                 # image i's own colours of every room (a gain and an offset, as color_mod gives)
        rooms = [(x, [(c * (0.8 + 0.02 * i) + 0.01 * i).clamp(0, 1).contiguous() for i in range(I)]) for x, c in rooms]
    return rooms, imgs, starts


def rgb_of(room, i):
    return room[1][i] if isinstance(room[1], list) else room[1]


def same_plan(n, per_image, I):
    lib = _lib.load()
    out = []
    for B in (per_image, I * per_image):
        nch, G = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(lib.pcl_gd_plan(n, B, ctypes.byref(nch), ctypes.byref(G), None), "pcl_gd_plan")
        out.append((nch.value, G.value))
    return out[0] == out[1]


def line(R, I, n, per_image, H, W, iters, per_image_colours, reps):
    rooms, imgs, starts = scene(R, I, n, per_image, H, W, per_image_colours)
    cfg = Cfg(lr=0.1, num_iter=iters, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=per_image, depth_mask=True)
    clone = lambda k: [[s[k].clone() for s in row] for row in starts]      # noqa: E731

    def singles():                                        # R x I x omniloc_batch -> [r][i]
        return [[po.omniloc_batch(imgs[i], rooms[r][0], rgb_of(rooms[r], i), starts[r][i][0].clone(), starts[r][i][1].clone(), cfg, {})
                 for i in range(I)] for r in range(R)]

    def per_room():                                       # R x omniloc_batch_images, shared colours
        tr, ro = clone(0), clone(1)
        return [po.omniloc_batch_images(imgs, rooms[r][0], rooms[r][1], tr[r], ro[r], cfg) for r in range(R)]

    def chain():
        if R == 1:                                        # colour sets of one room (or one room, one image: the single chain itself)
            tr, ro = clone(0), clone(1)
            return [po.omniloc_batch_images(imgs, rooms[0][0], rooms[0][1], tr[0], ro[0], cfg)]
        return po.omniloc_batch_rooms_images(imgs, rooms, clone(0), clone(1), cfg)
    routed = R == 1 or I == 1 or per_image_colours or I * per_image <= SHARED_CUT_OFF              # does the product take form (b) here?
    plan_differs = I > 1 and not per_image_colours and not same_plan(n, per_image, I)
    form_a = per_room if (I > 1 and not per_image_colours) else singles
    want, got = singles(), chain()
    form_a()
    same = all(torch.equal(got[r][i][k], want[r][i][k]) for r in range(R) for i in range(I) for k in range(3))
    assert same, "the shared depth chain and the single depth-masked calls differ"
    rec = {"rooms": R, "images": I, "points": n, "per_image": per_image, "iters": iters, "per_image_colours": per_image_colours,
           "identical_to_single_calls": bool(same), "a_form": form_a.__name__, "a_plan_differs": bool(plan_differs), "product_routes_to_b": bool(routed)}
    if form_a is per_room:
        fa = form_a()
        if plan_differs:
            rec["a_max_loss_difference"] = max(abs(float(fa[r][i][2]) - float(got[r][i][2])) for r in range(R) for i in range(I))
        else:
            assert all(torch.equal(got[r][i][k], fa[r][i][k]) for r in range(R) for i in range(I) for k in range(3)), "forms (a) and (b) differ"
    a, b = timed_ab(form_a, chain, reps)
    rec.update(summary("a", a, R * I))
    rec.update(summary("b", b, R * I))
    rec["ratio"] = round(rec["b_ms"] / rec["a_ms"], 3)
    rec["b_us_per_iteration"] = round(statistics.median(b) * 1e3 / iters, 1)
    del rooms, imgs, starts
    po._cache.clear()
    torch.cuda.empty_cache()
    return rec


SHARED_CUT_OFF = po.DEPTH_SHARED_ROOM_CANDIDATES         # the product's rule (omniloc.depth_shared_chain_pays), reported per line


def main():
    po.DEPTH_SHARED_ROOM_CANDIDATES = 1 << 30            # time the shared chain everywhere, also where the product routes to form (a)
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rooms", default="4,8")
    ap.add_argument("--images", default="1,8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    for k in ("cloud", "order", "box"):                  # a room search of an area keeps its rooms' packings for every image
        po._CAPACITY[k] = 128
    H, W, iters = 1024, 2048, 100
    shapes = []
    for R in [int(v) for v in args.rooms.split(",")]:
        for I in [int(v) for v in args.images.split(",")]:
            shapes.append((R, I, 166_667, 6, False))
            if I > 1:
                shapes.append((R, I, 166_667, 6, True))
    shapes.append((1, 8, 166_667, 6, True))              # colour sets alone
    if not args.no_large:
        shapes.append((1, 5, 1_000_000, 32, True))
        shapes.append((4, 1, 1_000_000, 32, False))      # a rooms chain of large rooms
    lines = []
    for R, I, n, per, sets in shapes:
        rec = line(R, I, n, per, H, W, iters, sets, args.reps)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
