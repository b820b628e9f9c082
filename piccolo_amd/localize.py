"""Counterpart of the reference's dataset harness (localize.py): the per-image body — colour preprocessing ->
starting poses -> refinement -> pose error (localize.py:173-258) —, a synthetic-scene driver that needs no dataset, and
the two dataset loops `localize_stanford` / `localize_omniscenes` over the reference's directory layout and CSV format.
The reference's own localize.py also runs unchanged on top of piccolo_amd's modules; the loops here
exist so that `main.py` works without OpenCV / TensorBoard (images through PIL, an optional writer) and shards the query
images over the ranks of a process group.
Every dataset loop (Stanford known room, Stanford room search, OmniScenes) is a `_Dataset` — ground_truth / load / report per image,
localize_group per call — run by ONE driver, `_run_dataset`, under ONE grouping rule, `_groups`: consecutive non-skipped images of this
rank whose jobs have equal group keys go into one call, up to cfg.images_per_launch (known room) or cfg.room_search_images (room search)
of them.  A size of 1 is the same path with groups of one.
"""
import collections
import csv
import dataclasses
import glob
import os
import random
import time

import numpy as np
import torch

from . import data_utils
from . import dist as pdist
from . import cfg_rules, ops, synth
from .cfg_rules import (dataset_plan, group_size as _group_size, polish_rules as _check_polish_cfg,  # noqa: F401  (the rules' old names here)
                        robust_rules as _check_robust_cfg, room_polish_rules as _check_room_polish_cfg, score_rules as _check_score_cfg)
from .color_utils import color_match, color_mod
from .omniloc import (omniloc_all, omniloc_batch, omniloc_batch_images, omniloc_batch_images_polished, omniloc_batch_images_robust,
                      omniloc_batch_rooms_images, omniloc_batch_rooms_images_polished, density_weights_of, score_weights)
from .utils import align_cloud, make_input_images, make_input_scored, make_pano, out_of_room, resize_image, voxel_downsample, write_summaries


def preprocess_colors(img, rgb, cfg):
    """The colour modulation step of the per-image body (localize.py:173-179 for Stanford2D3DS, :395-409 for
    OmniScenes): cfg.match_color -> color_match(img, rgb); cfg.sharpen_color -> color_mod(img, rgb, cfg.num_bins).
    As in the reference, both start from the ORIGINAL image (when both are set, color_mod's result is the one kept) and
    the result is re-quantised to uint8 levels (`(255 * new_img).astype(np.uint8)`, :404, :410).  -> (img, rgb)."""
    new_img = img
    if getattr(cfg, "match_color", False):
        new_img = color_match(img, rgb)
    if getattr(cfg, "sharpen_color", False):
        new_img, rgb = color_mod(img, rgb, int(getattr(cfg, "num_bins", 256)))
    if new_img is not img:
        new_img = synth.quantise_like_image_file(new_img * 255.0)
    return new_img, rgb


def refine_image(img, xyz, rgb, input_trans, input_rot, cfg, scalar_summaries=None, weights=None):
    """localize.py:215-233: run the refinement the config asks for and pick the min-loss candidate.
    Returns (t (3,1), R (3,3), loss) as cpu tensors.  weights (not in the reference): (N,) per-point weights of the refinement's loss.
    The extension keys (cfg_rules' table): the parallel branch is omniloc_batch and takes what it takes — with cfg.pose_covariance the
    return is (t, R, loss, cov); the non-parallel branch returns every candidate and refuses them all (ValueError), as omniloc_all does."""
    summaries = scalar_summaries if scalar_summaries is not None else {}
    if cfg_rules.on(cfg, "parallel"):
        results = [omniloc_batch(img, xyz, rgb, input_trans, input_rot, cfg, summaries, weights=weights)]
    else:
        # the reference loops omniloc() over the starting points (localize.py:219-220); same results, one launch chain
        results = omniloc_all(img, xyz, rgb, input_trans, input_rot, cfg, summaries, weights=weights)
    best = min(range(len(results)), key=lambda i: float(results[i][2]))
    return tuple(results[best][:4]) if cfg_rules.on(cfg, "pose_covariance") else (results[best][0], results[best][1], results[best][2])


def _make_input_args(cfg, init_dict=None):
    """What make_input / make_input_images take after the cloud, from cfg: (num_input, init_dict, criterion, num_intermediate)."""
    return (getattr(cfg, "num_input", 6), init_dict if init_dict is not None else get_init_dict(cfg), getattr(cfg, "criterion", "histogram"),
            getattr(cfg, "num_intermediate", 20))


def _images_in_rooms(imgs_init, imgs_main, rooms, cfg, init_dict):
    """The body of localize_in_rooms (I = 1) and localize_images_in_rooms.  One image issues exactly make_input per room and one
    omniloc_batch_rooms, by the entry points' own forwarding: shared_rgb turns a one-entry colour list into its tensor; make_input_images
    returns [make_input(...)] for I == 1, after looking up the same cached grids; omniloc_batch_rooms_images returns
    omniloc_batch_rooms(imgs[0], ...) on the callers' pose tensors for I == 1 — its depth_tau_groups split is omniloc_batch_rooms' own,
    and its other fallbacks ask for I > 1."""
    trs, ros, prepped = [], [], []
    for xyz, rgb in rooms:
        pre = [preprocess_colors(im, rgb, cfg) for im in imgs_init]
        rgbs = [c for _, c in pre]
        rgb_r = rgb if all(c is rgb for c in rgbs) else rgbs
        starts = make_input_images([im for im, _ in pre], xyz, rgb_r, *_make_input_args(cfg, init_dict))
        trs.append([tr for tr, _ in starts])
        ros.append([ro for _, ro in starts])
        prepped.append((xyz, rgb_r))
    polished = cfg_rules.on(cfg, "room_search_polish")
    if polished:
        # the room is decided by the CHAIN's losses — the plain search's, bit for bit —; pose, loss and cov are the found room's polished entry
        res, chain_loss = omniloc_batch_rooms_images_polished(imgs_main, prepped, trs, ros, cfg)
    else:
        res = omniloc_batch_rooms_images(imgs_main, prepped, trs, ros, cfg, batch_mode=cfg_rules.on(cfg, "parallel"))
    out = []
    for i in range(len(imgs_init)):
        losses = chain_loss[:, i].clone() if polished else torch.stack([res[r][i][2].reshape(()) for r in range(len(rooms))])
        k = int(torch.argmin(losses))
        out.append((k,) + tuple(res[k][i][:3]) + (losses,) + tuple(res[k][i][3:4]))          # (room, t, R, loss, every room's loss[, cov])
    return out


def localize_in_rooms(img_init, img_main, rooms, cfg, init_dict):
    """Room search: which of `rooms` (a list of (xyz, rgb) clouds in one frame, e.g. the rooms of one Stanford area) was the panorama
    taken in, and where.  Per room the colour preprocessing (preprocess_colors: with sharpen_color every room gets its own equalised
    colours) and the starting poses (make_input) on the initialisation image, then ONE refinement of the main image against all rooms
    (omniloc_batch_rooms; cfg.parallel selects omniloc_batch's or omniloc_all's semantics).  The room with the smallest loss wins (ties
    to the lowest index, as torch.argmin).  -> (room index, t (3,1), R (3,3), loss, every room's loss (R,))
    With cfg.room_search_polish (and the gn keys and / or cfg.pose_covariance; parallel only) the refinement is
    omniloc_batch_rooms_images_polished: the room and every room's loss are still the chain's — those of the plain search, bit for bit —,
    t, R and loss are the found room's polished entry, and with cfg.pose_covariance the tuple ends with that entry's cov (6, 6).
    (preprocess_colors re-quantises the colour-modulated initialisation image to 8-bit levels and honours match_color, like the OmniScenes
    loop; the known-room Stanford loop keeps color_mod's image as it is.  So a room search restricted to the ground-truth room does not
    reproduce a known-room Stanford run bit for bit: its starting poses may differ.)"""
    return _images_in_rooms([img_init], [img_main], rooms, cfg, init_dict)[0]


def localize_images_in_rooms(imgs_init, imgs_main, rooms, cfg, init_dict):
    """localize_in_rooms for SEVERAL panoramas of one size that meet the same rooms: per room the colour preprocessing of every image
    (preprocess_colors), then ONE make_input_images over the I initialisation images (with a colour list when the colours differ per image:
    sharpen_color), then ONE refinement of all main images against all rooms (omniloc_batch_rooms_images).
    -> a list whose entry i equals localize_in_rooms(imgs_init[i], imgs_main[i], rooms, cfg, init_dict) bit for bit: (room index, t, R,
    loss, every room's loss)."""
    if len(imgs_init) == 0 or len(imgs_main) != len(imgs_init):
        raise ValueError("localize_images_in_rooms: %d initialisation images, %d main images" % (len(imgs_init), len(imgs_main)))
    return _images_in_rooms(imgs_init, imgs_main, rooms, cfg, init_dict)


def pose_errors(t, R, gt_trans, gt_rot):
    """t-error (m) / R-error (deg), localize.py:239-247."""
    return synth.pose_errors(np.asarray(t), np.asarray(R), np.asarray(gt_trans), np.asarray(gt_rot))


def localize_synthetic(cfg, writer=None, log_dir=None):
    """Localise `num_images` synthetic panoramas of the box room (SURVEY.md §8d recipe) and report per-image errors.

    Query images are sharded over the ranks of an initialised process group (one process per GPU); every rank
    returns the full (num_images, 16) result table [t(3), R(9), loss, t_err, r_err, seconds]."""
    cfg_rules._refuse(cfg, "localize_synthetic")
    dev = ops.device()
    n = int(getattr(cfg, "num_points", 100_000))
    H, W = int(getattr(cfg, "pano_height", 256)), int(getattr(cfg, "pano_width", 512))
    n_img = int(getattr(cfg, "num_images", 4))
    B = int(getattr(cfg, "num_input", 6))
    xyz_np, rgb_np = synth.box_room(n, seed=0)
    xyz, rgb = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(rgb_np).to(dev)

    def body(k):
        t_gt, ypr_gt = synth.gt_pose(k)
        cam = ops.transform_cloud(xyz, torch.from_numpy(t_gt), torch.from_numpy(ypr_gt))
        img = synth.quantise_like_image_file(ops.make_pano(cam, rgb, (H, W)))
        img, rgb_k = preprocess_colors(img, rgb, cfg)
        tr, ro = synth.start_poses(t_gt, ypr_gt, B, seed=k, sigma_t=float(getattr(cfg, "start_sigma_t", 0.3)),
                                   sigma_r=float(getattr(cfg, "start_sigma_r", 0.15)))
        torch.cuda.synchronize()
        t0 = time.time()
        t, R, loss = refine_image(img, xyz, rgb_k, torch.from_numpy(tr).to(dev), torch.from_numpy(ro).to(dev), cfg)
        dt = time.time() - t0
        t_err, r_err = pose_errors(t, R, t_gt, synth.rot_from_ypr_np(ypr_gt))
        return torch.cat([t.reshape(3), R.reshape(9), loss.reshape(1), torch.tensor([t_err, r_err, dt])])

    table = pdist.localize_sharded(n_img, body, dev)
    rank, _ = pdist.world()
    if rank == 0 and log_dir is not None:
        os.makedirs(log_dir, exist_ok=True)
        with open(os.path.join(log_dir, "synthetic_results.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["image", "t_error (m)", "r_error (degrees)", "loss", "time (s)"])
            for k, row in enumerate(table.cpu().numpy()):
                w.writerow([k, row[13], row[14], row[12], row[15]])
    return table


# ------------------------------------------------------------------------------------------ dataset harness
def get_init_dict(cfg):
    """localize.py:18-73: the initialisation settings make_input reads, with the reference's defaults."""
    g = lambda k, d: getattr(cfg, k, d)  # noqa: E731
    return {"xy_only": g("xy_only", True), "num_trans": g("num_trans", 50), "yaw_only": g("yaw_only", True),
            "num_yaw": g("num_yaw", 4), "num_pitch": g("num_pitch", 0), "num_roll": g("num_roll", 0),
            "max_yaw": g("max_yaw", 2 * np.pi), "min_yaw": g("min_yaw", 0), "max_pitch": g("max_pitch", 2 * np.pi),
            "min_pitch": g("min_pitch", 0), "max_roll": g("max_roll", 2 * np.pi), "min_roll": g("min_roll", 0),
            "z_prior": g("z_prior", None), "dataset": cfg.dataset, "sample_rate_for_init": g("sample_rate_for_init", None),
            "trans_init_mode": g("trans_init_mode", "quantile"), "x_max": g("x_max", None), "x_min": g("x_min", None),
            "y_max": g("y_max", None), "y_min": g("y_min", None), "z_max": g("z_max", None), "z_min": g("z_min", None),
            "num_split_h": g("num_split_h", 2), "num_split_w": g("num_split_w", 4)}


def read_image(filename):
    """RGB uint8 (H,W,3) array of an image file (the reference: cv2.imread + BGR2RGB, localize.py:167)."""
    from PIL import Image
    with Image.open(filename) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8).copy()


def _to_img(img8, dev):
    # host division, like the reference (localize.py:169); exactly k/255 by construction: tagged, so that packing it never waits
    # for the device-side exactness check
    if img8.dtype != np.uint8:                    # the tag below promises levels k/255: only a decoded 8-bit image keeps it
        raise TypeError("_to_img: expected a uint8 image, got %s" % img8.dtype)
    return synth.mark_levels((torch.from_numpy(img8).float() / 255.).to(dev))


def _downsample(cfg):
    """cfg's down-sample factors of the query image: (init_h, init_w, main_h, main_w)."""
    return tuple(getattr(cfg, k, 1) for k in ("init_downsample_h", "init_downsample_w", "main_downsample_h", "main_downsample_w"))


def _query_images(orig, factors, dev):
    """The decoded uint8 image at the initialisation and at the main resolution (localize.py:168-169, :211-213), on the device."""
    dh, dw, mh, mw = factors
    return (_to_img(resize_image(orig, orig.shape[1] // dw, orig.shape[0] // dh), dev),
            _to_img(resize_image(orig, orig.shape[1] // mw, orig.shape[0] // mh), dev))


def pose_to_cloud_frame(t, R, align_rot, align_trans):
    """A pose (t (3, 1), R (3, 3)) found on the ALIGNED cloud x' = align_rot (x - align_trans), as a pose of the cloud's own frame: from
    R (R_a (x - a) - t) = (R R_a) (x - (a + R_a^T t)), t0 = a + R_a^T t and R0 = R R_a.  Computed in float64 -> float32 numpy."""
    Ra, a = np.asarray(align_rot, np.float64).reshape(3, 3), np.asarray(align_trans, np.float64).reshape(3, 1)
    t, R = np.asarray(t, np.float64).reshape(3, 1), np.asarray(R, np.float64).reshape(3, 3)
    return (a + Ra.T @ t).astype(np.float32), (R @ Ra).astype(np.float32)


def pose_from_cloud_frame(t0, R0, align_rot, align_trans):
    """pose_to_cloud_frame's inverse (what the reference does to the ground truth, localize.py:185-186): t = R_a (t0 - a), R = R0 R_a^T."""
    Ra, a = np.asarray(align_rot, np.float64).reshape(3, 3), np.asarray(align_trans, np.float64).reshape(3, 1)
    t0, R0 = np.asarray(t0, np.float64).reshape(3, 1), np.asarray(R0, np.float64).reshape(3, 3)
    return (Ra @ (t0 - a)).astype(np.float32), (R0 @ Ra.T).astype(np.float32)


# A room's alignment (cfg.align_cloud): utils.align_cloud's rot, trans and info, and xyz — the points of the cloud the routes see, in the
# room's OWN frame (what the result images show under the mapped pose)
_Alignment = collections.namedtuple("_Alignment", "rot trans info xyz")


class _Cloud(tuple):
    """(xyz, rgb) of a room on the device; .align: its _Alignment under cfg.align_cloud, else None"""
    align = None


def _read_cloud(read, path, sample_rate, dev, voxel=None, align=None):
    """(xyz, rgb) of a room on the device, a _Cloud.  align: cfg_rules.align_rules' answer under cfg.align_cloud — the cloud is turned once,
    after sample_rate and before the voxel keys (cells depend on the frame), so that its up direction is +z (utils.align_cloud).  voxel:
    cfg_rules.voxel_rules' (size, how) under cfg.voxel_size — the cloud is then replaced, once, before everything else, by its voxel grid's
    points (utils.voxel_downsample).  Every route sees a plain cloud."""
    xyz_np, rgb_np = read(path, sample_rate)
    xyz, rgb = torch.from_numpy(xyz_np).float().to(dev), torch.from_numpy(rgb_np).float().to(dev)
    own = xyz
    if align is not None:
        xyz, rot, trans, info = align_cloud(own, *align)
    if voxel is not None:
        xyz, rgb = voxel_downsample(xyz, rgb, voxel[0], how=voxel[1])[:2]
    cloud = _Cloud((xyz, rgb))
    if align is not None:
        if voxel is not None:                          # (the down-sampled points, back in the room's frame: R_a^T x + a)
            own = ops.align_transform_cloud(xyz, torch.from_numpy(rot.T.copy()), torch.from_numpy(-(rot @ trans)))
        cloud.align = _Alignment(rot, trans, info, own)
    return cloud


def _cloud_cache(read, sample_rate, dev, voxel=None, align=None, log=None):
    """path -> (xyz, rgb) on the device through a one-entry cache: consecutive images of one room get the SAME tensors (what their group
    key compares), and one room's cloud is held at a time.  voxel, align: _read_cloud's; log: a dict that gets every aligned room's
    tilt, yaw (degrees) and status under the cloud file's stem."""
    cache = {}

    def cloud(path):
        if path not in cache:
            cache.clear()
            cache[path] = _read_cloud(read, path, sample_rate, dev, voxel, align)
            _log_alignment(log, path, cache[path].align)
        return cache[path]
    return cloud


def _log_alignment(log, path, align):
    if log is not None and align is not None:
        log[os.path.splitext(os.path.basename(path))[0]] = {"tilt": float(np.degrees(align.info["tilt"])), "yaw": float(np.degrees(align.info["yaw"])),
                                                            "status": int(align.info["status"])}


def _gt_for_skip(align, gt_trans, gt_rot):
    """the ground-truth translation the skip rule tests against the cloud the routes see: mapped into the aligned frame under an alignment"""
    return gt_trans if align is None else pose_from_cloud_frame(gt_trans, gt_rot, align.rot, align.trans)[0]


def _results_to_cloud_frame(aligns, results):
    """every (t, R, ...) found on an aligned cloud as a pose of the room's own frame (pose_to_cloud_frame); the rest of a result — loss,
    covariance (the aligned frame's), found room — stays"""
    out = []
    for align, result in zip(aligns, results):
        if align is not None:
            t0, R0 = pose_to_cloud_frame(result[0], result[1], align.rot, align.trans)
            result = (torch.from_numpy(t0), torch.from_numpy(R0)) + tuple(result[2:])
        out.append(result)
    return out


def _fmt(a):
    return str(np.asarray(a).flatten())[1:-1].replace("\n", "")


class _NullWriter:
    def add_text(self, *a, **k):
        pass

    def add_scalar(self, *a, **k):
        pass


def _save_result_image(path, gt_img8, xyz, rgb, t, R, resolution):
    """localize.py:264-279: ground-truth panorama stacked over the cloud rendered from the estimated pose."""
    from PIL import Image
    new_xyz = torch.matmul(R.to(xyz.device), (xyz - t.reshape(1, 3).to(xyz.device)).t()).t()
    render = make_pano(new_xyz, rgb, resolution=resolution)
    gt = resize_image(gt_img8, render.shape[1], render.shape[0])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.concatenate([gt, np.asarray(render, np.uint8)], axis=0)).save(path)


def _save_starting_points(dirname, stem, gt_img8, xyz, rgb, input_trans, input_rot, align=None):
    """cfg.save_starting_point (localize.py:457-471): for every starting pose of the refinement, the query panorama stacked over
    the cloud rendered from that pose at half the panorama's resolution, as <dirname>/<stem>_<idx>.png.  align: the room's _Alignment —
    the poses are then mapped to the room's own frame and rendered over its own points."""
    from .utils import rot_from_ypr
    for idx in range(int(input_trans.shape[0])):
        t, R = input_trans[idx].detach().cpu().float(), rot_from_ypr(input_rot[idx].detach().cpu()).float()
        if align is not None:
            t, R = (torch.from_numpy(v) for v in pose_to_cloud_frame(t, R, align.rot, align.trans))
            xyz = align.xyz
        _save_result_image(os.path.join(dirname, "{}_{}.png".format(stem, idx)), gt_img8, xyz, rgb, t, R,
                           (gt_img8.shape[0] // 2, gt_img8.shape[1] // 2))


def _require_gravity_aligned(cfg):
    """localize.py:141,155-157 / :355,370-372: with gravity_aligned = False the reference calls data_utils.obtain_align_matrix,
    which its data_utils.py does not define (AttributeError on the first room); refused here before anything is loaded."""
    if not getattr(cfg, "gravity_aligned", True) and not cfg_rules.on(cfg, "align_cloud"):       # (with the switch: cfg_rules.align_rules)
        raise NotImplementedError("gravity_aligned = False: the reference's own path stops at the undefined "
                                  "data_utils.obtain_align_matrix (localize.py:155); align the cloud beforehand")


def stanford_success(t_err, r_err):
    """localize.py:250: `(t_error < 0.2) and (r_error < np.rad2deg(0.2))` — 0.2 m and 0.2 rad (11.46 degrees)."""
    return bool(t_err < 0.2 and r_err < np.rad2deg(0.2))


def omniscenes_success(t_err, r_err):
    """localize.py:513: `(t_error < 0.1) and (r_error < 5)` — 0.1 m and 5 degrees."""
    return bool(t_err < 0.1 and r_err < 5)


LAST_RUN = {}          # rank 0's summary of the latest dataset loop: accuracy, failed / skipped file names (what the reference prints)


def write_results(table, gts, filenames, writer, log_dir, csv_name, header, row_prefix, success, row_suffix=None):
    """Rank 0's tail of the dataset loops (localize.py:250-297 / :513-530): the CSV in the reference's columns, the running
    accuracy under the DATASET's own success rule (`success(t_err, r_err)`), failed / skipped rooms.  Pure host code.
    -> {"accuracy", "well_posed", "total", "failed", "skipped"}."""
    import contextlib
    writer = writer if writer is not None else _NullWriter()
    accuracy, well_posed, total = 0.0, 0, 0
    failed, skipped_list = [], []
    scalar_summaries = {"current_accuracy": []}
    if log_dir is not None:
        os.makedirs(log_dir, exist_ok=True)
    with (open(os.path.join(log_dir, csv_name), "w", encoding="utf-8", newline="") if log_dir is not None
          else contextlib.nullcontext(open(os.devnull, "w"))) as f:
        w = csv.writer(f)
        w.writerow(header)
        for k, row in enumerate(np.asarray(table)):
            gt_t, gt_r, skipped = gts[k]
            if skipped:
                skipped_list.append(filenames[k])
                writer.add_text("skipped rooms", filenames[k])
                w.writerow(row_prefix(filenames[k]) + [_fmt(gt_t), _fmt(gt_r), 1])
                continue
            t_err, r_err = float(row[13]), float(row[14])
            if success(t_err, r_err):
                well_posed += 1
            else:
                failed.append(filenames[k])
                writer.add_text("failed rooms", filenames[k])
            total += 1
            accuracy = well_posed / total
            scalar_summaries["current_accuracy"] = [accuracy]
            write_summaries(writer, scalar_summaries, k)                     # localize.py:295
            w.writerow(row_prefix(filenames[k]) + [_fmt(gt_t), _fmt(gt_r), 0, _fmt(row[0:3]), _fmt(row[3:12]), t_err, r_err,
                                                   float(row[15])] + (row_suffix(k) if row_suffix is not None else []))
    writer.add_scalar("final accuracy", accuracy)
    print("Final Accuracy : {}".format(accuracy))
    print("failed {} rooms : {}\n".format(len(failed), failed))
    print("skipped {} rooms : {}".format(len(skipped_list), skipped_list))
    return {"accuracy": accuracy, "well_posed": well_posed, "total": total, "failed": failed, "skipped": skipped_list}


@dataclasses.dataclass(eq=False)
class _Job:
    """One loaded query image of a dataset loop: what localize_group and report need of it."""
    img_init: torch.Tensor             # the image at the initialisation and at the main resolution, on the device
    img_main: torch.Tensor
    orig: np.ndarray                   # the uint8 image the result images show
    xyz: torch.Tensor = None           # known room: its cloud with THIS image's colours (color_mod / preprocess_colors) ...
    rgb: torch.Tensor = None
    show_rgb: torch.Tensor = None      # ... and the colours its result image is rendered with
    area: int = None                   # room search: the area and its [(room name, xyz, rgb)]
    rooms: list = None
    on_start: object = None            # on_start(input_trans, input_rot), called once the starting poses exist (save_starting_point)
    align: object = None               # known room under cfg.align_cloud: the room's _Alignment (xyz is then the aligned cloud)

    @property
    def show_xyz(self):
        """the points a result image shows under the reported pose: the room's own frame"""
        return self.xyz if self.align is None else self.align.xyz

    @property
    def group_key(self):
        """Jobs go into one call only if these are equal: the cloud's POINTS (known room: the xyz tensor itself; room search: the area)
        and the two image sizes."""
        return (id(self.xyz) if self.rooms is None else self.area, self.img_init.shape, self.img_main.shape)


# A dataset loop in plain steps.  ground_truth(k) -> (gt_trans, gt_rot, skipped): host work plus the cloud the skip rule needs (rank 0
# calls it for the other ranks' images too).  load(k) -> the image's job (anything with a group_key).  localize_group(jobs) -> one
# (t, R, loss, ...) per job, from ONE call.  report(k, job, result, row): the prints and the result image of a localised image.
_Dataset = collections.namedtuple("_Dataset", "ground_truth load localize_group report")


def _groups(indices, skipped, key, size):
    """THE grouping rule of the dataset loops, pure host code: walk `indices` in order; a skipped index neither joins nor ends a group;
    any other index joins the open group if its key equals the group's, else the open group ends and the index opens the next; a group
    of `size` ends at once.  Yields each group (a list of indices) when it ends — a full one before the next index is looked at — and
    calls skipped(k), then key(k), once per index."""
    group, group_key = [], None
    for k in indices:
        if skipped(k):
            continue
        k_key = key(k)
        if group and k_key != group_key:
            yield group
            group = []
        group, group_key = group + [k], k_key
        if len(group) >= size:
            yield group
            group = []
    if group:
        yield group


def _result_row(t, R, loss, gt_trans, gt_rot, seconds):
    t_err, r_err = pose_errors(t, R, gt_trans, gt_rot)
    return torch.cat([t.reshape(3), R.reshape(9), loss.reshape(1), torch.tensor([t_err, r_err, seconds], dtype=torch.float32)])


def _run_dataset(writer, log_dir, filenames, dataset, group_size, csv_name, header, row_prefix, success, row_suffix=None, on_gathered=None):
    """The one loop of the dataset harnesses: this rank's images (pdist.shard) in groups (_groups; every image is loaded once), one
    clock around a group's localize_group with the wall time shared equally (localize.py:208,222-223 per image), then a RESULT_WIDTH
    row and a report per image; a skipped image keeps its NaN row.  The rows are gathered, and rank 0 writes the reference's CSV and the
    accuracy under the dataset's own success rule (`success`: stanford_success / omniscenes_success)."""
    rank, world = pdist.world()
    mine = pdist.shard(len(filenames), rank, world)
    rows = torch.full((len(mine), pdist.RESULT_WIDTH), float("nan"), dtype=torch.float32)
    cuda = torch.cuda.is_available()                # (the loop itself is host code: the CPU tests drive it with a canned dataset)
    gts, jobs = {}, {}

    def ground_truth(k):
        if k not in gts:
            gts[k] = dataset.ground_truth(k)
        return gts[k]

    def skipped(k):
        skip = ground_truth(k)[2]
        if skip:
            print("corrupted file : {}, gt_trans is out of the room\n".format(filenames[k]))
        return skip

    def key(k):
        jobs[k] = dataset.load(k)
        return jobs[k].group_key

    for group in _groups(mine, skipped, key, group_size):
        batch = [jobs.pop(k) for k in group]
        if cuda:
            torch.cuda.synchronize()
        t0 = time.time()
        results = dataset.localize_group(batch)
        share = (time.time() - t0) / len(group)     # the group's wall time, shared equally
        for k, job, result in zip(group, batch, results):
            row = rows[(k - rank) // world] = _result_row(*result[:3], *ground_truth(k)[:2], share)
            dataset.report(k, job, result, row)
    table = pdist.gather_rows(rows.to(ops.device()) if cuda else rows, len(filenames), rank, world)
    if on_gathered is not None:                     # (every rank, after the rows: a collective of the caller's own, e.g. room search's)
        on_gathered()
    if world > 1 and rank == 0:                     # ground truths of the other ranks' images, for the CSV
        for k in range(len(filenames)):
            ground_truth(k)
    LAST_RUN.clear()
    if rank == 0:
        LAST_RUN.update(write_results(table.cpu().numpy(), gts, filenames, writer, log_dir, csv_name, header, row_prefix, success, row_suffix))
    return table


def _localize_known_room(cfg, plan, jobs):
    """localize_group of the known-room loops (localize.py:199-233): images that share the cloud's POINTS and the image sizes are
    initialised in one set of launches (make_input_images) and refined in one launch chain (omniloc_batch_images) — at the shipped 6
    candidates per image a launch is latency-bound, eight images cost little more than one.  Images whose cloud colours were changed per
    image (sharpen_color: color_mod gives every image its own equalised colours, localize.py:173-179) share the launches too: the
    group's cloud then holds one colour set per image, and every image's results are those of its own one-image calls, bit for bit.  When
    every job shares one rgb tensor it is passed as that tensor (the shared-colour path).  Grouping by colour sets was measured to beat
    one image at a time at the shipped and at the cfg-2 shape (tools/color_sets_bench.py).  One job: make_input_images is
    make_input, and the refinement is refine_image.  plan.route names a larger group's entry point: "polished" omniloc_batch_images_polished
    (the plain, robust or pruned chain, then the polish and / or covariance of all winners at once), "robust" omniloc_batch_images_robust;
    "scored" has groups of one, initialised with make_input_scored and refined under the score weights of their maps.  Under the density
    keys (cfg_rules.density_rules; route "plain", groups of one) the refinement runs under omniloc.density_weights_of the room's points: one
    weights tensor per room, hence one weighted pack for all of its images."""
    xyz = jobs[0].xyz
    rgb = jobs[0].rgb if all(j.rgb is jobs[0].rgb for j in jobs) else [j.rgb for j in jobs]
    if plan.route == "scored":                               # (one image per group: the rules refused every other group size)
        (job,), (split, floor, min_count) = jobs, plan.score
        tr, ro, maps = make_input_scored(job.img_init, xyz, rgb, *_make_input_args(cfg), score_split=split)
        if job.on_start is not None:
            job.on_start(tr, ro)
        return [refine_image(job.img_main, xyz, rgb, tr, ro, cfg, weights=score_weights(maps, floor, min_count))]
    starts = make_input_images([j.img_init for j in jobs], xyz, rgb, *_make_input_args(cfg))
    for j, (tr, ro) in zip(jobs, starts):
        if j.on_start is not None:
            j.on_start(tr, ro)
    if len(jobs) == 1:
        density = cfg_rules.density_rules(cfg)               # (one image per group under the density keys: the rules refused every other size)
        weights = density_weights_of(xyz, *density) if density is not None else None
        return [refine_image(jobs[0].img_main, xyz, rgb, *starts[0], cfg, weights=weights)]
    chain = ([j.img_main for j in jobs], xyz, rgb, [tr for tr, _ in starts], [ro for _, ro in starts], cfg)
    if plan.route == "polished":                             # (the gn keys and / or pose_covariance: the chain, then all winners at once)
        return [tuple(r) for r in omniloc_batch_images_polished(*chain)]
    if plan.route == "robust":                               # (groups of cfg.robust_images_per_launch, parallel only)
        return omniloc_batch_images_robust(*chain)
    return omniloc_batch_images(*chain, batch_mode=plan.parallel)


def _localize_aligned(cfg, plan, jobs):
    """_localize_known_room, its poses mapped back to the room's own frame where the jobs' cloud was aligned (cfg.align_cloud): errors, CSV
    rows, LAST_RUN and the result images are all made from the mapped poses.  A covariance stays the aligned frame's."""
    return _results_to_cloud_frame([j.align for j in jobs], _localize_known_room(cfg, plan, jobs))


def _note_alignments(plan, aligned):
    """LAST_RUN["align"] (rank 0, which reads every room for the ground truths): per room the tilt and yaw found, in degrees, and the vote's
    status — 1 (no voxel inside the tilt cone: the cloud was left as it is) is reported here, not raised"""
    if LAST_RUN and plan.align is not None:
        LAST_RUN["align"] = dict(aligned)


SIGMA_HEADER = ["sigma_t (m)", "sigma_r (degrees)"]


def pose_sigmas(cov):
    """(sigma_t in metres, sigma_r in degrees) of a (6, 6) pose covariance of (t, yaw, pitch, roll): sqrt(trace(cov[:3, :3])) and
    degrees(sqrt(trace(cov[3:, 3:]))); NaN where cov is"""
    cov = np.asarray(cov, dtype=np.float64).reshape(6, 6)
    return float(np.sqrt(np.trace(cov[:3, :3]))), float(np.degrees(np.sqrt(np.trace(cov[3:, 3:]))))


class _Columns:
    """`width` extra float columns per image of a dataset loop, next to its result row: a rank notes an image's values when it reports it,
    on_gathered sends them through the ranks' all_gather the way the result rows went, and every[k] / cells(k) read image k's out on every
    rank — NaN (an empty CSV cell) where nothing was noted: a skipped image, or a value that is NaN itself."""

    def __init__(self, width, count):
        self.width, self.count, self.local = width, count, {}
        self.every = np.full((count, width), np.nan, dtype=np.float32)

    def note(self, k, values):
        self.local[k] = values

    def on_gathered(self):
        rank, world = pdist.world()
        mine = pdist.shard(self.count, rank, world)
        rows = torch.full((len(mine), self.width), float("nan"), dtype=torch.float32)
        for j, k in enumerate(mine):
            if k in self.local:
                rows[j] = torch.tensor(self.local[k], dtype=torch.float32)
        self.every = pdist.gather_rows(rows.to(ops.device()) if torch.cuda.is_available() else rows, self.count, rank, world).cpu().numpy()

    def cells(self, k, first=0):
        return ["" if np.isnan(v) else float(v) for v in self.every[k][first:]]


def _run_known_room(plan, writer, log_dir, filenames, dataset, csv_name, header, row_prefix, success):
    """_run_dataset of a known-room loop.  With plan.sigmas (cfg.pose_covariance in a polished run: every result carries cov as its fourth
    entry) the CSV gains two last columns, sigma_t (m) and sigma_r (degrees) (pose_sigmas; empty where cov is NaN), through _Columns."""
    if not plan.sigmas:
        return _run_dataset(writer, log_dir, filenames, dataset, plan.group_size, csv_name, header, row_prefix, success)
    sigmas = _Columns(2, len(filenames))

    def report(k, job, result, row):
        sigmas.note(k, pose_sigmas(result[3]))
        dataset.report(k, job, result, row)

    return _run_dataset(writer, log_dir, filenames, dataset._replace(report=report), plan.group_size, csv_name, header + SIGMA_HEADER, row_prefix,
                        success, row_suffix=sigmas.cells, on_gathered=sigmas.on_gathered)


def _seed_all():
    torch.manual_seed(2)                            # localize.py:95-98
    if torch.cuda.is_available():
        torch.cuda.manual_seed(2)
    np.random.seed(2)
    random.seed(2)


def _f32(gt_trans, gt_rot):
    return gt_trans.astype(np.float32), gt_rot.astype(np.float32)


STANFORD_HEADER = ["area_num", "pano_name", "gt_trans", "gt_rot", "skipped?", "OmniLoc_trans", "OmniLoc_rot", "t_error (m)", "r_error (degrees)",
                   "time (s)"]
OMNISCENES_HEADER = STANFORD_HEADER[1:]             # (the same columns without the area)


def _stanford_parts(filename):
    """.../area_<area>/camera_<id>_<room type>_<room number>_... -> (area, image name, "<room type>_<room number>")"""
    img_name = filename.split("/")[-1]
    return int(filename.split("/")[-2].split("_")[-1]), img_name, "{}_{}".format(img_name.split("_")[2], img_name.split("_")[3])


def _stanford_row_prefix(filename):
    return list(_stanford_parts(filename)[:2])


def _stanford_report(filename, log_dir, job, xyz, rgb, result, row, found=""):
    area, img_name, _ = _stanford_parts(filename)
    print("\n{}\n{}translation error : {}\nrotation error : {}\n".format(img_name, found, float(row[13]), float(row[14])))
    if log_dir is not None:
        _save_result_image(os.path.join(log_dir, "results", "area_{}".format(area), img_name), job.orig, xyz, rgb, result[0], result[1],
                           (job.img_main.shape[0] // 2, job.img_main.shape[1] // 2))


def stanford_area_rooms(root, area, room_search=True):
    """The rooms a room search of Stanford area `area` considers: the stems of pcd_not_aligned/area_<area>/*.txt, sorted; a list
    `room_search` keeps those of its names (e.g. ["office_1", "hallway_2"]) in that sorted order."""
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(root, "pcd_not_aligned/area_{}/*.txt".format(area))))
    if isinstance(room_search, (list, tuple)):
        keep = {str(r) for r in room_search}
        names = [n for n in names if n in keep]
    return names


def localize_stanford(cfg, writer=None, log_dir="./log", root="./data/stanford"):
    """Stanford2D-3D-S loop (localize.py:76-297) over `root`/pano/area_*/ *.png, pcd_not_aligned/area_*/<room>.txt and
    pose/area_*/ *.json; writes `stanford_results.csv` with the reference's columns and result images under results/.
    The extension keys — cfg.images_per_launch and its robust_ / polish_ forms, the robust, gn, pose_covariance and score keys, room_search
    with room_search_images and room_search_polish — are resolved once, before any file is read, into cfg_rules.dataset_plan's route,
    group size and CSV columns (the rules: cfg_rules' table): a known-room route goes through _run_known_room and _localize_known_room,
    a room search (cfg.room_search True, or a list of room names) through _localize_stanford_rooms."""
    _require_gravity_aligned(cfg)
    plan = dataset_plan(cfg, "localize_stanford")
    _seed_all()
    dev = ops.device()
    area_num = getattr(cfg, "area", None)
    # the reference's sort key (room type, room number) leaves the cameras of one room in glob order; names break the tie here
    key = lambda x: (x.split("/")[-1].split("_")[2], int(x.split("/")[-1].split("_")[3]))  # noqa: E731
    if area_num is not None:
        areas = area_num if isinstance(area_num, list) else [area_num]
        filenames = []
        for a in areas:
            filenames += sorted(sorted(glob.glob(os.path.join(root, "pano/area_{}/*.png".format(a)))), key=key)
    else:
        filenames = sorted(sorted(glob.glob(os.path.join(root, "pano/area_*/*.png"))),
                           key=lambda x: (int(x.split("/")[-2].replace("area_", "")),) + key(x))
    room_name = getattr(cfg, "room_name", None)
    if room_name is not None:
        filenames = [f for f in filenames if room_name in f]
    if plan.room_search:
        return _localize_stanford_rooms(cfg, plan, writer, log_dir, root, filenames)
    quant = getattr(cfg, "out_of_room_quantile", 0.05)
    aligned = {}
    read_cloud = _cloud_cache(data_utils.read_stanford, getattr(cfg, "sample_rate", 1), dev, cfg_rules.voxel_rules(cfg), plan.align, aligned)

    def cloud(k):
        area, _, room = _stanford_parts(filenames[k])
        return read_cloud(os.path.join(root, "pcd_not_aligned/area_{}/{}.txt".format(area, room)))

    def ground_truth(k):
        area, img_name, _ = _stanford_parts(filenames[k])
        gt_trans, gt_rot = _f32(*data_utils.obtain_gt_stanford(area, img_name, root=os.path.join(root, "pose")))
        room = cloud(k)
        skipped = (bool(out_of_room(room[0], torch.from_numpy(_gt_for_skip(room.align, gt_trans, gt_rot)), quant))
                   and not getattr(cfg, "eval_full", False))
        return gt_trans, gt_rot, skipped

    def load(k):
        room = cloud(k)
        xyz, rgb = room
        orig = read_image(filenames[k])
        img, img_main = _query_images(orig, _downsample(cfg), dev)
        rgb_k = rgb
        if getattr(cfg, "sharpen_color", False):        # localize.py:175-179: only the INITIALISATION image is equalised
            img, rgb_k = color_mod(img, rgb, int(getattr(cfg, "num_bins", 256)))
        return _Job(img, img_main, orig, xyz, rgb_k, show_rgb=rgb, align=room.align)

    def report(k, job, result, row):
        _stanford_report(filenames[k], log_dir, job, job.show_xyz, job.show_rgb, result, row)

    table = _run_known_room(plan, writer, log_dir, filenames, _Dataset(ground_truth, load, lambda jobs: _localize_aligned(cfg, plan, jobs), report),
                            "stanford_results.csv", STANFORD_HEADER, _stanford_row_prefix, stanford_success)
    _note_alignments(plan, aligned)
    return table


def _localize_stanford_rooms(cfg, plan, writer, log_dir, root, filenames):
    """localize_stanford on the routes "rooms" / "rooms-polished" (cfg.room_search): every image is localised among the rooms of its area
    (stanford_area_rooms) by localize_in_rooms instead of in the room its file name names.  The skip rule stays on the ground-truth room's
    cloud (the same images are evaluated as in a known-room run); the CSV gets a last column found_room, LAST_RUN a room_accuracy, and
    the result image is rendered from the found room's cloud.  Each area's clouds are read once.  plan.group_size (cfg.room_search_images)
    = N: up to N consecutive non-skipped images of this rank that share area and image sizes are localised by ONE localize_images_in_rooms
    call (the same results, bit for bit); a group of one goes through localize_in_rooms.  Every rank localises its share of the images; the
    found rooms (as indices into the area's sorted listing) and, with plan.sigmas, sigma_t (m) and sigma_r (degrees) — the CSV's last
    columns after found_room — are gathered with the result rows (_Columns), so that rank 0 writes them and room_accuracy for every image.
    On "rooms-polished" (cfg.room_search_polish) localize_in_rooms goes through omniloc_batch_rooms_images_polished; found_room and
    room_accuracy stay those of the plain search."""
    dev = ops.device()
    sample_rate = getattr(cfg, "sample_rate", 1)
    quant = getattr(cfg, "out_of_room_quantile", 0.05)
    init_dict = get_init_dict(cfg)
    room_search, areas, found, voxel = plan.room_search, {}, {}, cfg_rules.voxel_rules(cfg)
    extra = _Columns(3 if plan.sigmas else 1, len(filenames))      # (the found room's index in the area's sorted listing[, sigma_t, sigma_r])
    frames, aligned = {}, {}                                       # cfg.align_cloud: (area, room) -> its _Alignment; LAST_RUN's log

    def read_cloud(area, room):
        path = os.path.join(root, "pcd_not_aligned/area_{}/{}.txt".format(area, room))
        cloud = _read_cloud(data_utils.read_stanford, path, sample_rate, dev, voxel, plan.align)
        frames[(area, room)] = cloud.align                         # (every room its own alignment)
        _log_alignment(aligned, path, cloud.align)
        return tuple(cloud)

    def area_rooms(area):
        if area not in areas:
            rooms = [(name,) + read_cloud(area, name) for name in stanford_area_rooms(root, area, room_search)]
            areas.clear()                              # (one area's clouds at a time: the images are sorted by area)
            areas[area] = rooms
        return areas[area]

    def ground_truth(k):
        area, img_name, gt_room = _stanford_parts(filenames[k])
        gt_trans, gt_rot = _f32(*data_utils.obtain_gt_stanford(area, img_name, root=os.path.join(root, "pose")))
        gt_cloud = next((xyz for name, xyz, _ in area_rooms(area) if name == gt_room), None)
        if gt_cloud is None:                           # (a list that leaves the ground-truth room out: its cloud still decides the skip)
            gt_cloud = read_cloud(area, gt_room)[0]
        skipped = (bool(out_of_room(gt_cloud, torch.from_numpy(_gt_for_skip(frames.get((area, gt_room)), gt_trans, gt_rot)), quant))
                   and not getattr(cfg, "eval_full", False))
        return gt_trans, gt_rot, skipped

    def load(k):
        area = _stanford_parts(filenames[k])[0]
        if not area_rooms(area):
            raise FileNotFoundError("room_search: no room clouds under pcd_not_aligned/area_{}".format(area))
        orig = read_image(filenames[k])
        return _Job(*_query_images(orig, _downsample(cfg), dev), orig, area=area, rooms=area_rooms(area))

    def localize_group(jobs):
        rooms = [(xyz, rgb) for _, xyz, rgb in jobs[0].rooms]
        if len(jobs) == 1:
            res = [localize_in_rooms(jobs[0].img_init, jobs[0].img_main, rooms, cfg, init_dict)]
        else:
            res = localize_images_in_rooms([j.img_init for j in jobs], [j.img_main for j in jobs], rooms, cfg, init_dict)
        res = [(one[1], one[2], one[3], one[0]) + tuple(one[5:6]) for one in res]       # (t, R, loss, room[, cov])
        return _results_to_cloud_frame([frames.get((j.area, j.rooms[one[3]][0])) for j, one in zip(jobs, res)], res)

    def report(k, job, result, row):
        name, xyz, rgb = job.rooms[result[3]]
        if frames.get((job.area, name)) is not None:
            xyz = frames[(job.area, name)].xyz
        extra.note(k, (float(result[3]),) + (pose_sigmas(result[4]) if plan.sigmas else ()))
        _stanford_report(filenames[k], log_dir, job, xyz, rgb, result, row, "found room : {}\n".format(name))

    def gather_found():
        extra.on_gathered()
        found.clear()
        listings = {}
        for k, v in enumerate(extra.every[:, 0]):
            if not np.isnan(v):
                area, _, gt_room = _stanford_parts(filenames[k])
                if area not in listings:
                    listings[area] = stanford_area_rooms(root, area, room_search)
                found[k] = (listings[area][int(v)], gt_room)

    def suffix(k):
        return [found[k][0] if k in found else ""] + extra.cells(k, 1)

    table = _run_dataset(writer, log_dir, filenames, _Dataset(ground_truth, load, localize_group, report),
                         plan.group_size, "stanford_results.csv",
                         STANFORD_HEADER + ["found_room"] + (SIGMA_HEADER if plan.sigmas else []), _stanford_row_prefix, stanford_success,
                         row_suffix=suffix, on_gathered=gather_found)
    if LAST_RUN:
        hits = [name == gt for name, gt in found.values()]
        LAST_RUN["room_accuracy"] = sum(hits) / len(hits) if hits else 0.0
        LAST_RUN["found_rooms"] = {filenames[k]: v[0] for k, v in found.items()}
        print("Room accuracy : {}".format(LAST_RUN["room_accuracy"]))
    _note_alignments(plan, aligned)
    return table


def localize_omniscenes(cfg, writer=None, log_dir="./log", root="./data/omniscenes"):
    """OmniScenes loop (localize.py:300-530) over `root`/<split>_pano/<video>/<frame>, pcd/<room>.txt and <split>_pose;
    writes `omniscenes_results.csv`.  Includes the synthetic illumination changes (synth_const / synth_gamma / synth_wb)
    and the colour preprocessing of the whole image (match_color / sharpen_color).  The extension keys as in localize_stanford's
    known-room routes (cfg_rules.dataset_plan; the room-search keys are ignored here)."""
    _require_gravity_aligned(cfg)
    plan = dataset_plan(cfg, "localize_omniscenes")
    _seed_all()
    dev = ops.device()
    split = getattr(cfg, "split_name", "extreme")
    filenames = sorted(glob.glob(os.path.join(root, "{}_pano/*/*".format(split))))
    room_name, scene = getattr(cfg, "room_name", None), getattr(cfg, "scene_number", None)
    if isinstance(room_name, str):
        filenames = [f for f in filenames if room_name in f]
    elif isinstance(room_name, list):
        filenames = [f for f in filenames if any(rm in f for rm in room_name)]
    if scene is not None:
        filenames = [f for f in filenames if "scene_{}".format(scene) in f]
    quant = getattr(cfg, "out_of_room_quantile", 0.05)
    dh, dw, mh, mw = _downsample(cfg)
    factors = (max(dh // 2, 1), max(dw // 2, 1), mh, mw)           # "match resolution with stanford" (localize.py:349-350)
    aligned = {}
    read_cloud = _cloud_cache(data_utils.read_omniscenes, getattr(cfg, "sample_rate", 1), dev, cfg_rules.voxel_rules(cfg), plan.align, aligned)

    def names(k):
        video, frame = filenames[k].split("/")[-2:]
        return video, frame, os.path.splitext(frame)[0]

    def cloud(k):
        video = names(k)[0]
        return read_cloud(os.path.join(root, "pcd/{}_{}.txt".format(video.split("_")[1], video.split("_")[2])))

    def ground_truth(k):
        gt_trans, gt_rot = _f32(*data_utils.obtain_gt_omniscenes(filenames[k]))
        room = cloud(k)
        return gt_trans, gt_rot, bool(out_of_room(room[0], torch.from_numpy(_gt_for_skip(room.align, gt_trans, gt_rot)), quant))

    def load(k):
        room = cloud(k)
        xyz, rgb = room
        video, _, stem = names(k)
        orig = resize_image(read_image(filenames[k]), 2048, 1024)   # localize.py:372
        if getattr(cfg, "synth_const", None) is not None:           # synthetic illumination changes, localize.py:375-385
            orig = orig // cfg.synth_const
        if getattr(cfg, "synth_gamma", None) is not None:
            orig = (((orig / 255.) ** cfg.synth_gamma) * 255).astype(np.uint8)
        if getattr(cfg, "synth_wb", None):
            for c, gain in enumerate((cfg.synth_r, cfg.synth_g, cfg.synth_b)):
                orig[..., c] = (((orig[..., c] / 255.) * gain) * 255).astype(np.uint8)
        new_img, rgb_k = preprocess_colors(_to_img(orig, dev), rgb, cfg)
        orig = (255 * new_img.cpu().numpy()).astype(np.uint8)
        on_start = None
        if getattr(cfg, "save_starting_point", False) and log_dir is not None:
            def on_start(input_trans, input_rot):
                _save_starting_points(os.path.join(log_dir, "starting_points", video), stem, orig, xyz, rgb_k, input_trans, input_rot, room.align)
        return _Job(*_query_images(orig, factors, dev), orig, xyz, rgb_k, show_rgb=rgb_k, on_start=on_start, align=room.align)

    def report(k, job, result, row):
        video, frame, stem = names(k)
        print("\n{}/{}\ntranslation error : {}\nrotation error : {}\n".format(video, frame, float(row[13]), float(row[14])))
        if log_dir is not None:
            _save_result_image(os.path.join(log_dir, "results", video, stem + ".png"), job.orig, job.show_xyz, job.show_rgb, result[0], result[1],
                               (job.img_main.shape[0] // 2, job.img_main.shape[1] // 2))

    table = _run_known_room(plan, writer, log_dir, filenames, _Dataset(ground_truth, load, lambda jobs: _localize_aligned(cfg, plan, jobs), report),
                            "omniscenes_results.csv", OMNISCENES_HEADER, lambda f: ["{}/{}".format(*f.split("/")[-2:])], omniscenes_success)
    _note_alignments(plan, aligned)
    return table
