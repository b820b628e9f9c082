#!/usr/bin/env python3
"""Room search over several panoramas, timing: I query panoramas localised among R rooms
  (a) one at a time — I x localize_in_rooms, each with R make_input calls and a chain of its own — against
  (b) together — one localize_images_in_rooms: per room ONE make_input_images over the I images, then ONE chain of I x R x 6 candidates,
with the rooms' colours shared by the images and with sharpen_color (every image its own equalised colours of every room); and the chain
alone: omniloc_batch_rooms_images against I x omniloc_batch_rooms.  Both forms are timed alternately (a b a b ...), medians of --reps,
in ms per image; both must return equal tensors (asserted).

    python tools/room_images_bench.py [--reps 9] [--rooms 4,8] [--images 2,4,8] [--out file.json]

Shipped shape: rooms of 166,667 points, 6 candidates, 2048 x 1024 panorama, 100 iterations; plus two chain-only lines with I = 4: 8 rooms
of 333,333 points x 6 candidates (the size cut-off of omniloc.rooms_images_chain_pays) and 4 rooms of 1M points x 32 candidates.  Prints one JSON object per line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from piccolo_amd import localize, ops, synth  # noqa: E402
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
    """A and B timed alternately (A B A B ...): clock and cache drift over the run falls on both sides alike"""
    a, b = [], []
    for _ in range(reps):
        a.append(once(fa))
        b.append(once(fb))
    return a, b


def summary(prefix, runs, I):
    """median, extremes and spread ((max - min) / median) of one form's repeats, in ms per image"""
    per = [v / I for v in runs]
    med = statistics.median(per)
    return {prefix + "_ms_per_image": round(med, 3), prefix + "_min": round(min(per), 3), prefix + "_max": round(max(per), 3),
            prefix + "_spread": round((max(per) - min(per)) / med, 4)}


def same_results(xs, ys):
    return all(a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1:], b[1:])) for a, b in zip(xs, ys))


def scene(R, I, n, per_image, H, W):
    rooms = [(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()) for x, c in synth.rooms_side_by_side([n] * R, seed=R)]
    imgs = []
    for i in range(I):                                   # image i was taken in room i mod R
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
    return rooms, imgs, starts


def chain_lines(rooms, imgs, starts, cfg, reps):
    """omniloc_batch_rooms_images against I x omniloc_batch_rooms, the packed clouds cached on both sides"""
    R, I = len(rooms), len(imgs)

    def together():
        return po.omniloc_batch_rooms_images(imgs, rooms, [[s[0].clone() for s in row] for row in starts], [[s[1].clone() for s in row] for row in starts], cfg)

    def one_by_one():
        return [po.omniloc_batch_rooms(imgs[i], rooms, [starts[r][i][0].clone() for r in range(R)], [starts[r][i][1].clone() for r in range(R)], cfg)
                for i in range(I)]
    together()
    one_by_one()
    got, want = together(), one_by_one()
    same = all(torch.equal(got[r][i][k], want[i][r][k]) for r in range(R) for i in range(I) for k in range(3))
    assert same, "the chain of all images and the chains per image differ"
    a, b = timed_ab(one_by_one, together, reps)
    rec = {"identical": bool(same)}
    rec.update(summary("chain_a", a, I))
    rec.update(summary("chain_b", b, I))
    rec["chain_ratio"] = round(rec["chain_b_ms_per_image"] / rec["chain_a_ms_per_image"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rooms", default="4,8")
    ap.add_argument("--images", default="2,4,8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-large", action="store_true")
    args = ap.parse_args()
    for k in ("cloud", "order", "box"):                  # a room search of an area keeps its rooms' packings for every image
        po._CAPACITY[k] = 128
    H, W, iters = 1024, 2048, 100
    lines = []
    for R in [int(v) for v in args.rooms.split(",")]:
        for I in [int(v) for v in args.images.split(",")]:
            rooms, imgs, starts = scene(R, I, 166_667, 6, H, W)
            cfg = Cfg(lr=0.1, num_iter=iters, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=6)
            chain = chain_lines(rooms, imgs, starts, cfg, args.reps)
            for sharpen in (False, True):
                icfg = Cfg(dataset="Stanford2D-3D-S", num_trans=50, xy_only=False, yaw_only=False, num_yaw=4, num_pitch=4, num_roll=4,
                           criterion="loss_histogram", num_intermediate=50, num_input=6, num_split_h=4, num_split_w=4, lr=0.1, num_iter=iters,
                           patience=5, factor=0.8, out_of_room_quantile=0.05, parallel=True, sharpen_color=sharpen, num_bins=256)
                init = localize.get_init_dict(icfg)

                def form_a():
                    return [localize.localize_in_rooms(im, im, rooms, icfg, init) for im in imgs]

                def form_b():
                    return localize.localize_images_in_rooms(imgs, imgs, rooms, icfg, init)
                form_a()                                 # warm-up: packing, engines, graph capture
                form_b()
                same = same_results(form_a(), form_b())
                assert same, "localize_images_in_rooms and localize_in_rooms differ"
                a, b = timed_ab(form_a, form_b, args.reps)
                rec = {"rooms": R, "images": I, "points": 166_667, "per_image": 6, "iters": iters, "sharpen_color": sharpen, "identical": bool(same)}
                rec.update(summary("a", a, I))
                rec.update(summary("b", b, I))
                rec["ratio"] = round(rec["b_ms_per_image"] / rec["a_ms_per_image"], 3)
                if not sharpen:
                    rec.update({k: v for k, v in chain.items() if k != "identical"})
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del rooms, imgs, starts
            po._cache.clear()
            torch.cuda.empty_cache()
    # chain-only lines at larger chains: at the size cut-off (omniloc.rooms_images_chain_pays: 16M point-poses per image), and the
    # 1M-point x 32-candidate line (128M); `shared_chain`: did the images share one chain, or did the rule give every image its own
    for R, I, n, per in ([] if args.no_large else [(8, 4, 333_333, 6), (4, 4, 1_000_000, 32)]):
        rooms, imgs, starts = scene(R, I, n, per, H, W)
        cfg = Cfg(lr=0.1, num_iter=iters, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=per)
        rec = {"rooms": R, "images": I, "points": n, "per_image": per, "iters": iters, "chain_only": True,
               "shared_chain": bool(po.rooms_images_chain_pays(R * n, per))}
        rec.update(chain_lines(rooms, imgs, starts, cfg, max(3, args.reps // 3)))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del rooms, imgs, starts
        po._cache.clear()
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
