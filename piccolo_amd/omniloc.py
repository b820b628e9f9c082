"""MI355X counterpart of the reference's omniloc.py — same names, arguments, return values and error behaviour.

    omniloc(img, xyz, rgb, input_trans, input_rot, starting_point, cfg, scalar_summaries)   omniloc.py:11-102
    omniloc_batch(img, xyz, rgb, input_trans, input_rot, cfg, scalar_summaries)             omniloc.py:205-296
    sampling_loss(img, xyz, rgb, input_trans, input_rot, starting_point, cfg, return_list)  omniloc.py:105-157
    SamplingLoss / BatchSamplingLoss (nn.Module, differentiable w.r.t. the pose)            omniloc.py:160-202, :299-356

The reference builds the loss from ~40 ATen ops and lets autograd differentiate it; here one HIP kernel computes
loss and gradient together (csrc/pcl_loss.hip) and the whole Adam / ReduceLROnPlateau / clamp loop runs on the
device (csrc/pcl_gd.hip) without a host round trip per iteration.  Differences a caller can observe:
  * results come back as DETACHED cpu float32 tensors (the reference's still require grad, which breaks its own
    localize.py:227 on numpy >= 2);
  * omniloc_batch also accepts a single candidate (the reference asserts num_input > 1, omniloc.py:208; the assert
    is kept because callers may rely on it, see `strict_reference_asserts`);
  * extra, optional cfg keys: depth_mask (default False = reference behaviour) multiplies the north star's
    scatter-min visibility (csrc/pcl_depth.hip) of the CURRENT poses into the loss mask at every iteration; depth_res =
    (depth_h, depth_w) is the z-buffer's grid (default: by point density, pcl_depth_default — not the panorama's size),
    depth_tau its tolerance (default: the rule's value for the grid), depth_stride = s builds the z-buffer from every s-th
    point of the Morton-ordered cloud (default: pcl_depth_default's choice; every point is still tested against it);
  * extra, optional cfg keys, all absent by default = reference behaviour, ruled by cfg_rules (its table: what goes with what, which entry
    point takes which family) and described at their sections below: prune_iters / prune_keep, robust_iters / robust_kind / robust_k,
    pose_covariance, gn_iters / gn_step_cap / gn_lambda / gn_objective / gn_delta, pyramid_iters / pyramid_reset; the score keys belong to the known-room dataset loops —
    here score_maps / score_weights give a caller the weights for weights=;
  * cfg.visualize: the reference's frame capture is broken (`new_xyz` undefined, omniloc.py:61 -> NameError); here
    omniloc returns the frame list that code means to build (query image over the cloud rendered at the current pose,
    per iteration) as 4th element.
"""
import weakref
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops
from .cfg_rules import (GN_KEYS, ROBUST_KEYS, SCORE_KEYS, _EXTENSIONS, _cfg, _refuse, _refuse_l1,  # noqa: F401  (re-exported)
                        depth_polish_flag, gn_schedule, pose_covariance_flag, prune_schedule, pyramid_schedule, robust_schedule)

strict_reference_asserts = True

# ------------------------------------------------------------------------------------------------ pack caches
# The harness calls omniloc() once per starting point with the same img/xyz/rgb (localize.py:219-220): pack once.
# One small LRU per KIND of packed object, so a stream of query images can never evict the room's Morton order, packed
# cloud, quantile box or translation grid (a dataset loop touches 4 cloud-side entries per room and 2 per image).
# An entry is keyed by the identity of the tensors it was made from (address, shape, in-place version) and holds weak
# references to them: a hit needs the very same live tensor, and entries whose tensors died are purged.
_CAPACITY = {"cloud": 2, "cloud_w": 2, "density": 4, "order": 2, "box": 8, "grid": 4, "pano": 16, "pano_u8": 16, "pano_u8p": 16, "pano_u8v": 16, "gd": 6, "gd_rooms": 4, "gd_rooms_images": 4, "trimgroups": 4, "pyramid": 16}


class _PackCache:
    def __init__(self):
        self.kinds = {}                     # kind -> OrderedDict(key -> ([weakrefs], object)), least recent first

    def _lru(self, kind):
        lru = self.kinds.get(kind)
        if lru is None:
            lru = self.kinds[kind] = OrderedDict()
        return lru

    def get(self, kind, key, tensors):
        lru = self._lru(kind)
        hit = lru.get(key)
        if hit is not None and all(r() is t for r, t in zip(hit[0], tensors)):
            lru.move_to_end(key)
            return hit[1]
        return None

    def put(self, kind, key, tensors, obj):
        lru = self._lru(kind)
        for k in [k for k, (refs, _) in lru.items() if any(r() is None for r in refs)]:
            del lru[k]                      # the tensors are gone: the address may be reused by another tensor
        lru[key] = ([weakref.ref(t) for t in tensors], obj)
        lru.move_to_end(key)
        while len(lru) > _CAPACITY.get(kind, 4):
            lru.popitem(last=False)

    def clear(self):
        self.kinds.clear()

    def __len__(self):
        return sum(len(v) for v in self.kinds.values())


_cache = _PackCache()


def _key(*tensors):
    return tuple((t.data_ptr(), tuple(t.shape), t._version, str(t.device), t.dtype) for t in tensors)


def _cached(kind, tensors, make, sub=None):
    """`kind` selects the LRU (and its capacity), `sub` distinguishes entries of one kind made from the same tensors
    (the quantile of a box, the config of a candidate grid)."""
    k = (sub,) + _key(*tensors)
    obj = _cache.get(kind, k, tensors)
    if obj is None:
        obj = make()
        _cache.put(kind, k, tensors, obj)
    return obj


def quantile_box_of(xyz, out_quantile):
    """The clamp box of omniloc.py:53-55 / :245-247, computed once per (cloud, quantile)."""
    return _cached("box", (xyz,), lambda: ops.quantile_box(xyz, out_quantile), sub=float(out_quantile))


def packed_cloud(xyz, rgb, weights=None):
    """Packed cloud cached per (xyz, rgb); the Morton order is cached per xyz alone, so a cloud whose colours change with
    every query image (color_mod, localize.py:175-179) is re-packed without being re-sorted.  `weights`: (N,) per-point weights in the
    order of xyz's rows, part of the cache key and kept in an LRU of their own ('cloud_w'): a weighted and an unweighted pack of the same
    (xyz, rgb) never alias, and neither takes the other's place."""
    def make():
        order = _cache.get("order", (None,) + _key(xyz), (xyz,))
        if order is not None:
            return ops.Cloud(xyz, rgb, order=order, weights=weights)
        c = ops.Cloud(xyz, rgb, weights=weights)
        if c.order is not None:
            _cache.put("order", (None,) + _key(xyz), (xyz,), c.order)
        return c
    if weights is None:
        return _cached("cloud", (xyz, rgb), make)
    if not torch.is_tensor(weights):
        raise ValueError("weights must be an (N,) tensor")
    # (an LRU of their own: make_input packs the room unweighted and the refinement weighted, and the two must not evict each other)
    return _cached("cloud_w", (xyz, rgb, weights), make)


def packed_cloud_sets(xyz, rgbs):
    """ONE packed cloud holding a colour set per entry of `rgbs` (ops.Cloud.with_color_sets): set i is packed_cloud(xyz, rgbs[i])'s colours,
    in the room's one Morton order (cached per xyz, as for packed_cloud)."""
    def make():
        order = _cache.get("order", (None,) + _key(xyz), (xyz,))
        if order is not None:
            return ops.Cloud.with_color_sets(xyz, rgbs, order=order)
        c = ops.Cloud.with_color_sets(xyz, rgbs)
        if c.order is not None:
            _cache.put("order", (None,) + _key(xyz), (xyz,), c.order)
        return c
    return _cached("cloud", (xyz,) + tuple(rgbs), make)


def color_set_groups(n, I, cap=None):
    """How per-image colour sets split I images of an n-point cloud: group sizes of at most the addressing limit (ops.max_color_sets), the
    32 images a trim / histogram launch takes and `cap`."""
    cap = max(1, min(ops.max_color_sets(n), ops.TRIM_MAX_IMAGES, ops.HIST_MAX_IMAGES, cap if cap is not None else I))
    return [min(cap, I - i0) for i0 in range(0, I, cap)]


def shared_rgb(rgb):
    """`rgb` of the multi-image entry points: one (N, 3) tensor, or a list of one per image.  A list whose entries are all the same tensor
    is that tensor (the shared-colour path, bit for bit).  -> the tensor, or the list"""
    if isinstance(rgb, (list, tuple)):
        if len(rgb) == 0:
            raise ValueError("rgb: an empty list of colour sets")
        if all(r is rgb[0] for r in rgb):
            return rgb[0]
        return list(rgb)
    return rgb


def packed_pano(img, many_poses=False, n_points=None):
    """Packed panorama of `img`, cached per tensor.  RGBA8 texels (half the footprint of the fp16-level default) when the launch
    evaluates hundreds of candidate poses all over the room (`many_poses`, trim_input_loss: with 1800 poses the fp16 texture
    thrashes L2, 8.7 vs 5.3 ms per launch at cfg-2 size) or when the cloud to be refined is sparse against the panorama
    (`n_points`: ops.refine_texels); fp16-level texels otherwise (the refinement's nearby poses on a dense cloud run 5 % faster on
    them).  The trim launch of a SPARSE cloud takes its own layout ('u8p', rows interleaved in pairs, cache 'pano_u8p'; a DENSE one
    'u8v', vertical pairs), so at the
    shipped 167k-point shape an image whose initialisation and refinement use the same tensor is packed twice (8 MB each, two
    caches): the two stages share a packing only for dense clouds' trim ('u8') and a sparse cloud's refinement ('u8').  Images that
    are not k/255 get float4 texels either way."""
    rgba8 = many_poses or (n_points is not None and ops.refine_texels(n_points, img.shape[0], img.shape[1]) == "u8")
    if ops.EXPERIMENT.pano_fmt in ("f16", "f32") and not many_poses:             # experiments: force the refinement's format
        rgba8 = False
    if not rgba8:
        return _cached("pano", (img,), lambda: ops.Pano(img))
    # the trim launch picks its own layout by point density (ops.trim_texels: rows interleaved in pairs / plain rows / vertical pairs);
    # nothing else reads the paired layouts
    fmt = ops.trim_texels(n_points, img.shape[0], img.shape[1]) if many_poses and n_points is not None else "u8"
    if ops.EXPERIMENT.trim_fmt in ("u8", "u8p", "u8v") and many_poses:            # experiments
        fmt = ops.EXPERIMENT.trim_fmt

    def make():
        try:
            return ops.Pano(img, fmt=fmt)
        except ValueError:
            return ops.Pano(img, fmt="f32")
    return _cached("pano_" + fmt, (img,), make)


def _chain_panos(imgs, n_points, direct=False):
    """The packed panoramas of the images of ONE chain, in one texel format: the one packed_pano gives a refinement of n_points points, float4
    for all when the images do not agree (a launch needs ONE format, and float4 holds any image).  direct: packed past the cache, at
    refine_texels' format for images tagged as k/255 levels (omniloc_batch_images beyond eight images: more than the cache is meant to hold)."""
    if direct:
        fmt = ops.refine_texels(n_points, imgs[0].shape[0], imgs[0].shape[1])
        panos = [ops.Pano(im, fmt=fmt if ops._known_levels(im) else "auto") for im in imgs]
    else:
        panos = [packed_pano(im, n_points=n_points) for im in imgs]
    if len({p.fmt for p in panos}) > 1:
        panos = [ops.Pano(im, fmt="f32") for im in imgs]
    return panos


def _over_color_sets(n, I, part, rooms=None):
    """I images with per-image colour sets of an n-point cloud (the largest room's) in color_set_groups' groups: None when one group holds them
    all, else _side_by_side of the groups"""
    sizes = color_set_groups(n, I)
    return None if len(sizes) == 1 else _side_by_side(sizes, part, rooms)


def _side_by_side(sizes, part, rooms=None):
    """part(i0, i1) of every run [i0, i1) of `sizes` images concatenated, image after image — per room when part returns `rooms` lists"""
    out, i0 = [] if rooms is None else [[] for _ in range(rooms)], 0
    for m in sizes:
        some = part(i0, i0 + m)
        if rooms is None:
            out += some
        else:
            for r in range(rooms):
                out[r] += some[r]
        i0 += m
    return out


def _rot_matrix(ypr):
    return ops.rot_from_ypr(ypr.reshape(1, 3))[0]


# ------------------------------------------------------------------------------------------------ GD drivers
# A refinement of a SMALL problem is launch-latency bound: 2 x num_iter dependent launches of a few microseconds each
# (the reference's shipped configs: 167k points x 6 candidates, 15 us per iteration on the GPU).  For those the whole
# launch chain is captured once into a hipGraph and replayed for every later refinement of the same cloud and shape —
# pcl_gd_run neither allocates nor synchronises, every candidate reads its panorama through its pose record
# (pcl_gd_set_panos), so a new image only needs pcl_gd_init + pcl_gd_set_panos + one graph launch.  Replay is
# bit-identical to the eager launches (tests).  Measured at cfg 1: 0.65 vs 0.73 ms per refinement; nothing at cfg 2
# (110 us kernels), hence the size limit.  Round 5: between 4M and 16M point-poses (1M points x 6 candidates, 400k x 32: 15-30 us
# launches) the medians are the same, but an eager chain now and then loses a millisecond to the host thread (3.3 -> 4.4 ms, 5.2 -> 6.2 ms
# seen at 1M / 2M points x 6 candidates; never with replay): the limit went from 4M to 16M.
GRAPH_POINT_POSES = 16_000_000         # use graph replay when points x candidates is at most this (cfg key gd_graph overrides)


def _engine_args(cfg, batch_mode=True):
    """The keyword arguments every GD engine of ops takes, from cfg: the hyper-parameters, one or two launches per iteration (cfg gd_fuse =
    False: two, bit-identical) and the depth mask's optional tolerance, grid and occluder stride."""
    d_tau, d_res, d_st = _cfg(cfg, "depth_tau", None), _cfg(cfg, "depth_res", None), _cfg(cfg, "depth_stride", None)
    return {"lr": float(_cfg(cfg, "lr", 0.1)), "patience": int(_cfg(cfg, "patience", 5)), "factor": float(_cfg(cfg, "factor", 0.9)),
            "batch_mode": bool(batch_mode), "fuse": None if _cfg(cfg, "gd_fuse", True) else False,
            "depth_mask": bool(_cfg(cfg, "depth_mask", False)), "depth_tau": None if d_tau is None else float(d_tau),
            "depth_res": None if d_res is None else (int(d_res[0]), int(d_res[1])), "depth_stride": None if d_st is None else int(d_st)}


def _replays_graph(cfg, point_poses, depth_mask):
    """Does a chain of `point_poses` points x candidates replay a captured graph?  cfg gd_graph decides, else the size; a depth-masked chain
    always runs eager."""
    use_graph = _cfg(cfg, "gd_graph", None)
    if use_graph is None and ops.EXPERIMENT.gd_graph is not None:                   # experiments
        use_graph = bool(ops.EXPERIMENT.gd_graph)
    if use_graph is None:
        use_graph = point_poses <= GRAPH_POINT_POSES
    return bool(use_graph) and not depth_mask


def _cached_engine(kind, xyzs, sub, make, clouds, boxes):
    """One engine (state, workspace, captured graph) per POINT SETS `xyzs` and launch shape `sub` -> (engine, fresh: it was made just now, with
    the caller's poses).  The colours may change with every query image (color_mod / match_color give each image its own rgb, or its own
    colour sets): the engine make(clouds, boxes) builds owns private copies of the packed clouds and boxes, whose addresses its captured graph
    holds, and clouds with other colours are copied into them (24 bytes per point on the device) instead of capturing a new graph per image."""
    def make_private():
        private = [ops.Cloud.private_copy(c) for c in clouds], [ops._dev(b).reshape(6).clone() for b in boxes]
        g = make(*private)
        g._private = private
        g._cloud_src = [weakref.ref(c) for c in clouds]      # the copies just made ARE these clouds: nothing to copy on first use
        g._box_src, g._fresh = list(boxes), True             # (weak above: the engine must not keep packed clouds of past images alive)
        return g
    gd = _cached(kind, xyzs, make_private, sub=sub)
    fresh, gd._fresh = gd._fresh, False
    for r, (c, b) in enumerate(zip(clouds, boxes)):
        if gd._cloud_src[r]() is not c:
            gd._private[0][r].data.copy_(c.data)
            if c.weights is not None:                        # (the engine key tells weighted from unweighted: the private cloud has a plane)
                gd._private[0][r].weights.copy_(c.weights)
            gd._cloud_src[r] = weakref.ref(c)
        if gd._box_src[r] is not b:                          # (the cached box tensor of this cloud: identity is enough)
            gd._private[1][r].copy_(ops._dev(b).reshape(6))
            gd._box_src[r] = b
    return gd, fresh


# ------------------------------------------------------------------------------------------------ robust chains
# cfg robust_iters / robust_kind / robust_k (not in the reference; absent by default): a built-in source of per-point weights for a scene
# that changed since the cloud was scanned.  After robust_iters[j] iterations in all the chain takes the candidate pcl_gd_winner names, the
# per-point residuals at its pose (pcl_point_residuals), their lower median s, and weighs every point l <= k s ? 1 : 0 ("trunc") or
# l <= k s ? 1 : k s / l ("huber"); the SAME optimiser state goes on under pcl_gd_run_weighted.  Nothing waits for the host.  The returned
# loss is the WEIGHTED loss of the last forward; Adam's moments and the plateau scheduler carry on across the switch, so the scheduler's
# `best` then compares weighted with unweighted losses — it is not reset.  Several images of one cloud: omniloc_batch_images_robust.
def point_residuals(img, xyz, rgb, trans, rot, depth=None, return_visible=False):
    """(B, N) GPU tensor, in the order of xyz's rows: per point the ||c - rgb|| the sampling loss sums at the poses trans / rot ((B, 3)
    tensors: translation; yaw, pitch, roll) where its mask keeps the point, exactly -1 where the point samples exact black
    (ops.point_residuals over the cached packed cloud and panorama).  depth / return_visible: ops.point_residuals' (the depth mask of the
    same poses; -1 where hidden; with return_visible (rows, visible))."""
    return ops.point_residuals(packed_cloud(xyz, rgb), packed_pano(img, n_points=xyz.shape[0]), trans, rot, depth=depth,
                               return_visible=return_visible)


def robust_weights(residuals_row, kind="trunc", k=2.5):
    """(N,) GPU weights in the caller's point order from ONE row of point_residuals, usable as `weights=` wherever weights are taken: with s
    the lower median of the entries that are not -1, "trunc": l <= k s ? 1 : 0, "huber": l <= k s ? 1 : k s / l; masked points (-1) weigh 1,
    NaN or infinite residuals 0 (pcl_robust_weights — the weights do not depend on the order of the points)."""
    row = ops._dev(residuals_row).reshape(-1)
    n = int(row.numel())
    return ops.robust_plane(n, row, kind, k)[0][:n].clone()


# ------------------------------------------------------------------------------------------------ score maps
# (not in the reference; build-defined, include/piccolo_hip.h) a source of per-point weights that needs no current pose: the histogram
# stage's table of patch intersections, averaged over the candidate poses per image patch (2D map) and per point (3D map: the patch each
# point projects into).  A region of the cloud that no longer looks like the query image collects low intersections from every pose that
# sees it.  No occlusion test: a hidden point votes with the patch in front of it.  One cloud, one colour set, one image.
def score_maps(img, xyz, rgb, trans, rot, num_split_h, num_split_w, parts=None):
    """Namespace(score3d (N,), count3d (N,) int32 — in the order of xyz's rows; score2d, count2d (num_split_h - 2, num_split_w); inter, nproj
    (K, nblk), nimg (nblk,), scores (K,): the histogram stage's parts; num_split_h, num_split_w) of the K poses trans / rot against img:
    ops.hist_trim_scores(..., return_parts=True), then ops.score_maps.  parts: (scores, inter, nproj, nimg) of that very call made before
    (utils.make_input_scored keeps its histogram stage's)."""
    cloud = packed_cloud(xyz, rgb)
    trans, rot = ops._dev(trans).reshape(-1, 3), ops._dev(rot).reshape(-1, 3)
    H, W = int(img.shape[0]), int(img.shape[1])
    if parts is None:
        parts = ops.hist_trim_scores(img, cloud, trans, rot, num_split_h, num_split_w, return_parts=True)
    scores, inter, nproj, nimg = parts
    s3, c3, s2, c2 = ops.score_maps(cloud, trans, rot, H, W, num_split_h, num_split_w, inter, nproj, nimg)
    shape = (num_split_h - 2, num_split_w)
    return SimpleNamespace(score3d=s3, count3d=c3, score2d=s2.view(shape), count2d=c2.view(shape), inter=inter, nproj=nproj, nimg=nimg,
                                 scores=scores, num_split_h=num_split_h, num_split_w=num_split_w)


def score_weights(maps, floor=0.0, min_count=1):
    """(N,) GPU weights in the caller's point order from score_maps' 3D map, usable as `weights=` wherever weights are taken: the scores of
    the points with at least min_count votes stretched from [lowest, highest] to [floor, 1]; a point with fewer votes weighs 1, and so does
    every point when nothing voted or all voted scores are equal (pcl_score_weights — the weights do not depend on the order of the
    points)."""
    n = int(maps.score3d.numel())
    return ops.score_weight_plane(n, maps.score3d, maps.count3d, floor, min_count)[0][:n].clone()


# ------------------------------------------------------------------------------------------------ density weights
# (not in the reference; build-defined, include/piccolo_hip.h) a source of per-point weights that needs neither a pose
# nor the query image: a surface the scanner sampled fifty times as densely as another one otherwise gets fifty times the vote.
def density_weights_of(xyz, voxel, cap=1):
    """ops.VoxelGrid(xyz, voxel).weights(cap), cached per live xyz tensor and (voxel, cap): the SAME (N,) tensor object for every query image
    of a room — packed_cloud keys its weighted pack on the identity of the weights tensor, so one tensor means one pack.  Eager (the grid
    reads its voxel count back): the first image of a room pays for it."""
    voxel, cap = ops.voxel_size(voxel), ops.density_cap(cap)
    return _cached("density", (xyz,), lambda: ops.VoxelGrid(xyz, voxel).weights(cap), sub=(voxel, cap))


# ------------------------------------------------------------------------------------------------ pose information / covariance
# (not in the reference; build-defined, include/piccolo_hip.h): how well the panorama constrains a pose — the Gauss-Newton information
# matrix H = sum w m j j^T of theta = (t, yaw, pitch, roll) and cov = sigma^2 H^-1 with sigma^2 = sum w m l^2 / sum w m.  cfg
# pose_covariance (a bool, absent by default): omniloc_batch returns [t, R, loss, cov] under the weights its last forward ran with.  One
# cloud, one colour set, one image, no depth mask; nothing is claimed about its calibration on real data.

# ------------------------------------------------------------------------------------------------ Levenberg-Marquardt polish
# (not in the reference; build-defined, include/piccolo_hip.h): a damped Gauss-Newton chain on H and b, wholly on
# the device.  It minimises the MEAN SQUARED residual sigma^2 = sum w m l^2 / sum w m — not the sampling loss sum w m l / sum w m the GD
# chains minimise: same per-point terms, mask and weights, another objective.  cfg gn_iters (an int >= 1, absent by default), gn_step_cap
# and gn_lambda (optional: the step cap in metres / radians and the starting damping): omniloc_batch polishes its winner.  One cloud, one
# colour set, one image, no depth mask; nothing is claimed about real data.  cfg gn_objective = "l1" (gn_delta: ops.GN_L1_DELTA = 1 / 64 when
# absent) polishes on the Huber-L1 objective sum w m rho(l) / sum w m instead, which tends to the sampling loss itself as delta -> 0
# (DESIGN.md section 4.1i), re-weighting inside the chain.  The rooms forms refuse it.
# Under the depth mask: depth= of the functions below evaluates residuals, information and polish under the mask of
# the poses they evaluate, rebuilt at every trial pose; cfg depth_polish = True next to depth_mask lets omniloc_batch take the gn keys and
# pose_covariance (cfg_rules.depth_polish_flag).  Unweighted, one colour set, one image.
def gauss_newton_refine(img, xyz, rgb, trans, rot, iters=10, weights=None, trace=False, objective="l2", delta=None, depth=None, **hyper):
    """ops.gauss_newton_refine from the poses trans / rot ((B, 3) tensors: translation; yaw, pitch, roll) over the cached packed cloud and
    panorama: a dict of GPU tensors (trans, rot, sigma2_start, sigma2, lam, accepted, rejected, evaluations, status, H, b, stats, cov, and
    trace when asked).  weights: (N,) per-point weights in the order of xyz's rows.  objective="l1" / delta: the Huber-L1 objective
    (ops.gauss_newton_refine: sigma2* hold F_rho, stats = (M, S1, sum w m rho, F_rho, status), cov None).  depth: the chain under the depth
    mask, rebuilt at every trial pose (ops.gauss_newton_refine; not with weights)."""
    return ops.gauss_newton_refine(packed_cloud(xyz, rgb, weights), packed_pano(img, n_points=xyz.shape[0]), trans, rot, iters=iters, trace=trace,
                                   objective=objective, delta=delta, depth=depth, **hyper)


def pose_information(img, xyz, rgb, trans, rot, weights=None, objective="l2", delta=None, depth=None):
    """(H (B,6,6), b (B,6), stats (B,5) = M, S1, S2, sigma^2, status, cov (B,6,6)) on the GPU at the poses trans / rot ((B, 3) tensors:
    translation; yaw, pitch, roll), over the cached packed cloud and panorama (ops.pose_information).  weights: (N,) per-point weights in
    the order of xyz's rows.  objective="l1" / delta: the Huber-L1 record (ops.pose_information: H_rho, b_rho, stats = (M, S1, sum w m rho,
    F_rho, status), cov None).  depth: the sums under the depth mask of the same poses (ops.pose_information; not with weights)."""
    return ops.pose_information(packed_cloud(xyz, rgb, weights), packed_pano(img, n_points=xyz.shape[0]), trans, rot, objective=objective, delta=delta,
                                depth=depth)


def pose_covariance(img, xyz, rgb, trans, rot, weights=None, depth=None):
    """(cov (B,6,6), sigma^2 (B,), status (B,)) of pose_information: cov = sigma^2 H^-1 in theta's units (metres, radians), all NaN where
    status is not 0 (1: nothing kept or something not finite; 2: H not positive definite).  depth: under the depth mask of the poses."""
    _, _, stats, cov = pose_information(img, xyz, rgb, trans, rot, weights, depth=depth)
    return cov, stats[:, 3], stats[:, 4]


def _images_cloud(who, imgs, xyz, rgb, weights):
    """The packed cloud and panoramas of the several-image forms below: rgb one (N, 3) tensor (with optional (N,) weights) or a list of one
    per image (one colour set per image; no weights)"""
    rgb = shared_rgb(rgb)
    if isinstance(rgb, list):
        if len(rgb) != len(imgs):
            raise ValueError("%s: %d colour sets for %d images" % (who, len(rgb), len(imgs)))
        if weights is not None:
            raise ValueError("%s: per-point weights do not combine with per-image colour sets" % who)
        if len(rgb) == 1:
            rgb = rgb[0]
    cloud = packed_cloud_sets(xyz, rgb) if isinstance(rgb, list) else packed_cloud(xyz, rgb, weights)
    return cloud, _chain_panos(list(imgs), xyz.shape[0])


def pose_information_images(imgs, xyz, rgb, trans, rot, weights=None, objective="l2", delta=None):
    """pose_information for several query images of one cloud in one set of launches (ops.pose_information_images): row i of (H, b, stats,
    cov) is pose (trans[i], rot[i]) against imgs[i] — and rgb[i], when rgb is a list of one colour tensor per image.  weights: (N,) per-point
    weights in the order of xyz's rows, shared by the images (one colour tensor only).  objective / delta: as pose_information."""
    cloud, panos = _images_cloud("pose_information_images", imgs, xyz, rgb, weights)
    return ops.pose_information_images(cloud, panos, trans, rot, objective=objective, delta=delta)


def gauss_newton_refine_images(imgs, xyz, rgb, trans, rot, iters=10, weights=None, trace=False, objective="l2", delta=None, **hyper):
    """gauss_newton_refine for several query images of one cloud in ONE chain (ops.gauss_newton_refine_images): pose i is polished against
    imgs[i] — and rgb[i], when rgb is a list of one colour tensor per image.  Row i of every entry equals the single-image call's.
    objective / delta: as gauss_newton_refine."""
    cloud, panos = _images_cloud("gauss_newton_refine_images", imgs, xyz, rgb, weights)
    return ops.gauss_newton_refine_images(cloud, panos, trans, rot, iters=iters, trace=trace, objective=objective, delta=delta, **hyper)


POLISHED_ROW = 52      # floats per image a polished chain copies to the host: t (3), R (9), loss, took, S1, M, cov (36)


def _entry(row, want_cov=False, loss=None):
    """A host row -> [t (3,1), R (3,3), loss ()] from its columns 0:3, 3:12 and 12 (or the `loss` given), and cov (6,6) from a POLISHED_ROW's
    last 36 when wanted: with _polished_entry the only places where what an entry point returns is cut from what the D2H copy brought"""
    out = [row[0:3].reshape(3, 1).clone(), row[3:12].reshape(3, 3).clone(), row[12].clone() if loss is None else loss]
    if want_cov:
        out.append(row[16:POLISHED_ROW].reshape(6, 6).clone())
    return out


def _polished_entry(row, want_cov):
    """_entry of a _polished_rows row: where the polish took a step (column 13) the loss is S1 / M of its info record (columns 14, 15)"""
    # (float32 on the host: one correctly rounded division)
    return _entry(row, want_cov, row[14] / row[15] if float(row[13]) != 0.0 else None)


def _last_engine(gd):
    """the engine whose forward ran last in the chain `gd` (an engine or a _PrunedChain)"""
    return gd.last if isinstance(gd, _PrunedChain) else gd


def _winners_polished(gd, cloud, panos, wins, gn, want_cov):
    """What omniloc_batch does for its one winner, for the (I, 16) winners rows `wins` of the chain `gd` (an engine or a _PrunedChain) at
    once -> (I, POLISHED_ROW) on the GPU.  With gn: one gauss_newton_refine_images_at_winners under the weight planes the chain's last
    forward ran with; where the polish took a step (accepted > 1, status 0 or 3) t and R are the polished pose's, `took` is 1 and S1, M are
    those of the polish's info record at that pose (the caller forms the loss S1 / M), else the chain's own t, R, loss.  cov: the polish's
    own, or pose_information_images_at_winners' when there is no polish (zeros when not wanted)."""
    I = int(wins.shape[0])
    engine = _last_engine(gd)
    planes = engine._run_weights()
    if planes is not None:
        planes = planes.view(I, -1) if engine.weight_sets else None          # (a plain chain's cloud plane is the cloud's own)
    return _polished_rows(wins, gn, want_cov, lambda: ops.pose_information_images_at_winners(cloud, panos, wins, planes=planes),
                          lambda: ops.gauss_newton_refine_images_at_winners(cloud, panos, wins, iters=gn[0], planes=planes, **gn[1]),
                          lambda trans, rot: ops.pose_information_images(cloud, panos, trans, rot, planes=planes))


def _polished_rows(wins, gn, want_cov, information, polish, information_at=None):
    """The (I, POLISHED_ROW) rows of _winners_polished from information() (gn None) or polish(): the images or the rooms form at `wins`.
    An L1 polish has no cov of its own: information_at(trans, rot), one plain pass at the RETURNED poses, gives it."""
    I = int(wins.shape[0])
    zero = torch.zeros(I, 3, dtype=torch.float32, device=wins.device)
    if gn is None:
        cov = information()[3]
        return torch.cat([wins[:, 0:13], zero, cov.reshape(I, 36)], dim=1)
    res = polish()
    R = ops.rot_from_ypr(res["rot"]).reshape(I, 9)
    took = ((res["accepted"] > 1) & ((res["status"] == 0) | (res["status"] == 3))).reshape(I, 1)
    rows = torch.where(took, torch.cat([res["trans"], R, zero[:, 0:1]], dim=1), wins[:, 0:13])
    if want_cov and res["cov"] is None:
        cov = information_at(torch.where(took, res["trans"], wins[:, 0:3]), torch.where(took, res["rot"], wins[:, 13:16]))[3].reshape(I, 36)
    else:
        cov = res["cov"].reshape(I, 36) if want_cov else torch.zeros(I, 36, dtype=torch.float32, device=wins.device)
    return torch.cat([rows, took.to(torch.float32), res["stats"][:, 1:2], res["stats"][:, 0:1], cov], dim=1)


def _winner_cloud(gd, cloud):
    """`cloud` under the weight plane the last forward of the chain `gd` (an engine or a _PrunedChain) ran with"""
    plane = _last_engine(gd)._run_weights()
    if plane is not None and plane is not cloud.weights:
        cloud = cloud.weighted_view(plane)
    return cloud


def _winner_covariance(gd, cloud, pano, win, depth=None):
    """cov (1,6,6) on the GPU at the pose of the (1, 16) winners row `win` of the chain `gd` (an engine or a _PrunedChain), under the weight
    plane its last forward ran with (depth: under the chain's depth mask at that pose — cfg.depth_polish; such a chain has no weights)"""
    return ops.pose_information_at_winners(_winner_cloud(gd, cloud), pano, win, depth=depth)[3]


def _winner_polish(gd, cloud, pano, win, gn, want_cov=False, depth=None):
    """The (1, 16) winners row `win` polished on the device under the chain's weights -> (row (13,) GPU: t, R, loss where the polish took a
    step — accepted > 1 and status 0 or 3; R is rot_from_ypr of the polished angles, loss the sampling loss re-evaluated there by one
    forward-only launch — else the chain's own three entries bit for bit; cov (1,6,6) GPU: the polish's own, at the returned pose — an
    L1 polish has none: with want_cov one plain pose_information pass at the returned pose gives it, else None).  depth (cfg.depth_polish):
    the polish, the re-evaluated loss and that pass all run under the chain's depth mask, rebuilt at the pose each of them evaluates."""
    cloud = _winner_cloud(gd, cloud)
    res = ops.gauss_newton_refine_at_winners(cloud, pano, win, iters=gn[0], depth=depth, **gn[1])
    R = ops.rot_from_ypr(res["rot"]).reshape(1, 9)
    loss = ops.sampling_loss(cloud, pano, res["trans"], res["rot"], with_grad=False, depth=depth)[:, 0:1]
    took = ((res["accepted"] > 1) & ((res["status"] == 0) | (res["status"] == 3))).reshape(1, 1)
    cov = res["cov"]
    if cov is None and want_cov:
        cov = ops.pose_information(cloud, pano, torch.where(took, res["trans"], win[:, 0:3]), torch.where(took, res["rot"], win[:, 13:16]),
                                   depth=depth)[3]
    return torch.where(took, torch.cat([res["trans"], R, loss], dim=1), win[:, 0:13])[0], cov


# ------------------------------------------------------------------------------------------------ pruned chains
# cfg prune_iters / prune_keep (not in the reference; absent by default): after prune_iters[j] iterations in all, every image — every
# (room, image) of a rooms chain — keeps its prune_keep[j] best candidates by the loss of that iteration's forward (history row
# prune_iters[j] - 1) and the chain goes on with them alone: pcl_gd_prune hands their complete optimiser state to a smaller engine on the
# device, so nothing is re-initialised and nothing waits for the host.  The reference refines every one of its num_input candidates to
# the end; which schedule still finds its winner is the user's choice (DESIGN.md §4.6f has the CPU evidence for 16 -> 8 -> 4).
class _PrunedChain:
    """What a pruned refinement hands back in place of its engine: winners() of the LAST segment's engine, and every candidate's leaf row
    written back to the caller's buffers — a dropped candidate's from the prune call that dropped it (its pose at that time), a
    survivor's from the last engine, through the survivors' indices composed on the device."""

    def __init__(self, first, groups):
        self.B, self.groups, self.last = first.B, groups, first
        self.rows = None                  # row of the caller's tensors each candidate of the current engine came from (None: its own)
        self.steps = []                   # (rows, leaf_t, leaf_r) of every prune call, in order

    def prune(self, child):
        gd, dev = self.last, self.last.state.device
        leaf_t, leaf_r = torch.empty(gd.B, 3, dtype=torch.float32, device=dev), torch.empty(gd.B, 3, dtype=torch.float32, device=dev)
        survivors = gd.prune_into(child, leaf_t, leaf_r)
        per, keep = gd.B // self.groups, child.B // self.groups
        local = survivors.long() + torch.arange(self.groups, device=dev).repeat_interleave(keep) * per
        self.steps.append((self.rows, leaf_t, leaf_r))
        self.rows = local if self.rows is None else self.rows[local]
        self.last = child

    def winners(self, groups, leaf_trans=None, leaf_rot=None):
        if groups != self.groups:
            raise ValueError("winners: a chain pruned per %d groups asked for %d" % (self.groups, groups))
        dev = self.last.state.device
        leaf_t, leaf_r = torch.empty(self.last.B, 3, dtype=torch.float32, device=dev), torch.empty(self.last.B, 3, dtype=torch.float32, device=dev)
        out = self.last.winners(groups, leaf_t, leaf_r)
        for dst, col in ((leaf_trans, 1), (leaf_rot, 2)):
            if dst is None:
                continue
            dst = dst.view(self.B, 3)
            for step in self.steps + [(self.rows, leaf_t, leaf_r)]:
                if step[0] is None:
                    dst.copy_(step[col])
                else:
                    dst.index_copy_(0, step[0], step[col])
        return out

    def winner(self, nimages=1, leaf_trans=None, leaf_rot=None):
        return self.winners(nimages, leaf_trans, leaf_rot)


def _run_segments(sched, groups, gd, point_poses, cfg, depth_mask, cached_child):
    """Run the segments of prune_schedule one after another, starting with the engine `gd` (initialised, its pose records naming their
    panoramas): k iterations, prune into the next segment's engine, and so on.  Every segment is a replayed graph or eager by _replays_graph
    on ITS points x candidates, point_poses(per); a replaying segment's engine comes from cached_child(per) (_cached_engine), an eager one is
    made for the occasion (`per`: candidates per group).  -> _PrunedChain"""
    if _cfg(cfg, "visualize", False):
        raise ValueError("cfg.visualize does not combine with cfg.prune_iters / cfg.prune_keep")
    chain = _PrunedChain(gd, groups)
    for s, (iters, per) in enumerate(sched):
        graph = _replays_graph(cfg, point_poses(per), depth_mask)
        if s > 0 and groups * per != chain.last.B:           # (keeping every candidate would be a plain copy: the engine goes on as it is)
            chain.prune(cached_child(per) if graph else chain.last._smaller(per))
        if graph:
            chain.last.run_graph(iters)
        else:
            chain.last.run(iters)
    return chain


# What _drive needs to know of a chain.  kind, key(per), xyzs: the engine cache's LRU, the launch shape of `per` candidates per group, the point
# sets (_cached_engine); clouds, boxes: the caller's packs; make(clouds, boxes, trans, rot) -> a new engine; name(gd, graph, fresh): name the
# panoramas where this kind of chain does; groups: the candidate groups (images; rooms x images); point_poses(per): the size _replays_graph
# judges; run(gd, graph): the iterations of a chain without a schedule; sched: prune_schedule's segments or None; replay False: never a graph.
# (A plain namespace filled by keyword: a namedtuple built by keyword costs the host three times as much per refinement.)
_Chain = SimpleNamespace


def _drive(c, tr, ro, cfg):
    """THE chain driver: decide graph replay; eager: a new engine on the caller's packs, replay: the cached engine, reset unless it was made
    just now with these poses; name the panoramas; run the prune segments, or the chain's own run form.  -> the engine, or the _PrunedChain"""
    B = int(tr.shape[0])
    per = B // c.groups
    if per * c.groups != B:
        raise ValueError("%d candidates do not split into %d groups" % (B, c.groups))
    graph = c.replay and _replays_graph(cfg, c.point_poses(per), c.depth_mask)

    def cached(per):
        """-> (the cached engine of `per` candidates per group, fresh): made with the first rows of the caller's poses"""
        rows = c.groups * per
        return _cached_engine(c.kind, c.xyzs, c.key(per), lambda cs, bs: c.make(cs, bs, tr[:rows], ro[:rows]), c.clouds, c.boxes)
    if not graph:
        gd, fresh = c.make(c.clouds, c.boxes, tr, ro), True      # (fresh buffers: nothing worth keeping for a long eager chain)
    else:
        gd, fresh = cached(per)
        if not fresh:
            gd.reset(tr, ro)
    c.name(gd, graph, fresh)
    if c.sched is not None:
        return _run_segments(c.sched, c.groups, gd, c.point_poses, cfg, c.depth_mask, lambda per: cached(per)[0])
    c.run(gd, graph)
    return gd


def packed_pyramid(img, levels, pano0, n_points):
    """The PanoPyramid of `img` with `levels` coarse levels over the packed level-0 panorama `pano0`, cached per tensor; the coarse levels'
    texel formats are ops.refine_texels' for n_points points at each level's size."""
    return _cached("pyramid", (img,), lambda: ops.PanoPyramid(img, levels, n=n_points, pano0=pano0), sub=(levels, int(n_points), pano0.fmt))


def _refine(xyz, rgb, panos, trans, rot, box, cfg, batch_mode, vis_hook=None, weights=None, weight_sets=0, imgs=None):
    """Run the on-device GD for the rows of trans / rot and return the GradientDescent object (read gd.result() / gd.winner()); under
    cfg.prune_iters / cfg.prune_keep the _PrunedChain of its segments (read winner() / winners()).
    `panos`: one packed panorama per query image; the B rows split evenly over them, image by image.  `rgb`: one (N, 3) tensor, or a list
    of one per query image (per-image colour sets: image i's candidates read set i, and the chain runs the single-image plan).
    The GradientDescent object (state, workspace, captured graph) is cached per cloud and launch shape (_cached_engine).  `weights`: (N,)
    per-point weights (one colour set, no depth mask).  weight_sets = len(panos): the robust chain over several images (a weight-set engine,
    ops.GradientDescent(weight_sets=I): the single-image plan, one weight plane per image; omniloc_batch_images_robust).
    `imgs`: the query images `panos` were packed from, where the caller takes cfg.pyramid_iters / cfg.pyramid_reset (pyramid_schedule): the
    chain then runs coarse-to-fine over every image's PanoPyramid (ops.GradientDescent.run_pyramid), on an engine of its own."""
    pyramid = pyramid_schedule(cfg, (panos[0].H, panos[0].W))
    if pyramid is not None:
        if imgs is None or weight_sets or vis_hook is not None:
            raise ValueError("cfg.pyramid_iters: the plain refinement of omniloc_batch / omniloc_batch_images only")
        if weights is not None:
            raise ValueError("cfg.pyramid_iters does not combine with weights=")
    robust = robust_schedule(cfg)
    if robust is not None and not weight_sets:
        if weights is not None:
            raise ValueError("cfg.robust_iters does not combine with weights= (the chain makes its own)")
        if isinstance(rgb, list) or len(panos) != 1 or not batch_mode or vis_hook is not None:
            raise ValueError("cfg.robust_iters: the parallel refinement of one image over one colour set only")
    if weights is not None and isinstance(rgb, list):
        raise ValueError("per-point weights do not combine with per-image colour sets")
    if weights is not None and bool(_cfg(cfg, "depth_mask", False)):
        raise ValueError("per-point weights do not combine with cfg.depth_mask")
    cloud = packed_cloud_sets(xyz, rgb) if isinstance(rgb, list) else packed_cloud(xyz, rgb, weights)
    trans, rot = ops._dev(trans).reshape(-1, 3), ops._dev(rot).reshape(-1, 3)
    I, p0, num_iter = len(panos), panos[0], _cfg(cfg, "num_iter", 100)
    args = _engine_args(cfg, batch_mode)
    sched = prune_schedule(cfg, int(trans.shape[0]) // I)
    if sched is not None and vis_hook is not None:
        raise ValueError("cfg.visualize does not combine with cfg.prune_iters / cfg.prune_keep")
    extra = {"weight_sets": weight_sets} if weight_sets else {}
    # (one or two launches per iteration is frozen into a captured graph: part of the key, with the other arguments)
    # (the robust chains have engines of their own: a plain call never meets an engine whose plane is switched on, or one of the
    # single-image plan)
    # (and so has a coarse-to-fine chain: its graphs are the levels', and a plain call never meets them)
    tail = tuple(args.values()) + (("robust_images",) if weight_sets else ("robust",) if robust is not None else ())
    if pyramid is not None:
        tail += ("pyramid", tuple(pyramid[0]), pyramid[1])

    def name(gd, graph, fresh):
        if weight_sets or I > 1 or graph or sched is not None:   # (a later segment may replay a graph that holds another image's panorama)
            gd.set_pano_groups(list(panos))                      # addresses as kernel arguments: no H2D copy, nothing waits

    def run(gd, graph):
        if robust is not None:
            gd.run_robust(num_iter, robust[0], robust[1], robust[2], graph=graph)
        elif pyramid is not None:
            pyramids = [packed_pyramid(im, len(pyramid[0]), p, cloud.n) for im, p in zip(imgs, panos)]
            gd.run_pyramid(pyramids, num_iter, pyramid[0], reset_plateau=pyramid[1], graph=graph)
        elif vis_hook is not None:
            vis_hook(gd, num_iter)
        elif graph:
            gd.run_graph(num_iter)
        else:
            gd.run(num_iter)
    return _drive(_Chain(kind="gd", key=lambda per: (I * per, I, p0.H, p0.W, p0.fmt, cloud.color_sets, cloud.weights is not None) + tail,
                         xyzs=(xyz,), clouds=[cloud], boxes=[box], make=lambda cs, bs, t, r: ops.GradientDescent(cs[0], p0, t, r, bs[0], **args, **extra),
                         name=name, groups=I, point_poses=lambda per: cloud.n * I * per, run=run, sched=sched, depth_mask=args["depth_mask"],
                         replay=vis_hook is None), trans, rot, cfg)


def _refine_groups(chain, trans_list, rot_list, polish=None):
    """The groups of one chain, start to end: trans_list / rot_list hold one (B, 3) tensor of starting poses per group of candidates (an
    image, a room, a room's image: the same B everywhere), chain(tr, ro) runs the engine over their concatenation.  -> per group
    [t (3,1), R (3,3), loss ()] of the candidate with the smallest last loss (omniloc.py:271), after ONE D2H copy, the leaf rows written
    back into the callers' tensors.  polish(gd, winners) -> a GPU tensor of one row per group, made from the winners rows on the device:
    it is what the one D2H copy brings, and it is returned as it is (omniloc_batch_images_polished)."""
    n, B = len(trans_list), int(trans_list[0].shape[0])
    tr = torch.cat([ops._dev(t).reshape(B, 3) for t in trans_list])
    ro = torch.cat([ops._dev(r).reshape(B, 3) for r in rot_list])
    gd = chain(tr, ro)
    leaf_t, leaf_r = torch.empty(n * B, 3, dtype=torch.float32, device=tr.device), torch.empty(n * B, 3, dtype=torch.float32, device=tr.device)
    wins = gd.winners(n, leaf_t, leaf_r)
    host = (wins if polish is None else polish(gd, wins)).cpu()
    with torch.no_grad():
        for k, (t, r) in enumerate(zip(trans_list, rot_list)):
            t.copy_(leaf_t[k * B:(k + 1) * B].reshape(t.shape).to(t.device))
            r.copy_(leaf_r[k * B:(k + 1) * B].reshape(r.shape).to(r.device))
    if polish is not None:
        return host
    return [_entry(row) for row in host]


def _over_room_groups(groups, part):
    """part(idx) -> the results of the rooms `idx` (a list of room indices); -> the results of all the rooms of `groups`, in room order"""
    out = [None] * sum(len(idx) for idx in groups)
    for idx in groups:
        for r, o in zip(idx, part(idx)):
            out[r] = o
    return out


def _room_cap_groups(R):
    """rooms 0..R-1 in runs of at most PCL_GD_MAX_ROOMS, the rooms of one chain"""
    cap = ops._lib.GD_MAX_ROOMS
    return [list(range(r0, min(r0 + cap, R))) for r0 in range(0, R, cap)]


def _leaf_buffers(input_trans, input_rot, B):
    """The caller's starting-pose tensors as write-back targets of pcl_gd_winner when they are contiguous float32 GPU tensors of B
    rows (the harness's are); else fresh buffers plus a copy afterwards.  -> (buf_t, buf_r, after)"""
    def usable(t):
        return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 3 * B and not t.requires_grad
    bt = input_trans if usable(input_trans) else torch.empty(B, 3, dtype=torch.float32, device=ops.device())
    br = input_rot if usable(input_rot) else torch.empty(B, 3, dtype=torch.float32, device=ops.device())

    def after():
        with torch.no_grad():
            if bt is not input_trans:
                input_trans.copy_(bt.reshape(input_trans.shape).to(input_trans.device))
            if br is not input_rot:
                input_rot.copy_(br.reshape(input_rot.shape).to(input_rot.device))
    return bt, br, after


def omniloc(img, xyz, rgb, input_trans, input_rot, starting_point, cfg, scalar_summaries, weights=None):
    """Sequential refinement of ONE starting pose.  Returns [t (3,1), R (3,3), loss ()] (+ frames if cfg.visualize).
    weights (not in the reference): (N,) per-point weights of the loss in the order of xyz's rows, non-negative and finite.

    `loss` is the loss of the last forward, i.e. at the pose before the final update, like the reference
    (omniloc.py:46,102).  Row `starting_point` of input_trans / input_rot ends up holding the final pose, as in the
    reference where the optimised tensors are views of those rows (omniloc.py:15-19).
    """
    _refuse(cfg, "omniloc")
    _refuse(cfg, "omniloc", "pyramid")
    vis = _cfg(cfg, "visualize", False)
    out_quantile = _cfg(cfg, "out_of_room_quantile", 0.05)

    pano = packed_pano(img, n_points=xyz.shape[0])
    # the reference recomputes these three quantiles every iteration (omniloc.py:53-55); they are loop invariant
    box = quantile_box_of(xyz, out_quantile)
    frames = []
    hook = (lambda gd, n: frames.extend(_run_with_frames(gd, img, xyz, rgb, n))) if vis else None
    res = _refine(xyz, rgb, [pano], input_trans[starting_point], input_rot[starting_point], box, cfg, False, vis_hook=hook,
                  weights=weights).result()[0]
    R = _rot_matrix(res[3:6])
    out = torch.cat([res[0:3], R.reshape(-1), res[12:13]]).cpu()
    with torch.no_grad():
        input_trans[starting_point] = res[6:9].to(input_trans.device)
        input_rot[starting_point] = res[9:12].to(input_rot.device)
    ret = _entry(out)
    if vis:
        ret.append(frames)
    return ret


def _run_with_frames(gd, img, xyz, rgb, num_iter):
    """cfg.visualize: the frame list the reference means to build (omniloc.py:59-69, :93-100; its own code stops at the
    undefined `new_xyz`): per iteration one PIL frame, the query image on top of the cloud rendered (make_pano, half
    resolution) at the pose that iteration's forward used; the first frame 5 times in all, the last one 10 more times, then
    5 frames with a black lower half.  The harness saves them as a GIF (localize.py:285-288).  Same on-device GD, one
    iteration per call; the renders are the z-buffer kernel."""
    import numpy as np
    from PIL import Image
    h, w = int(img.shape[0]) // 2, int(img.shape[1]) // 2
    gt_img = Image.fromarray(np.uint8(ops._dev(img).cpu().numpy() * 255), "RGB").resize((w, h))
    frames, new_frame = [], None
    for it in range(num_iter):
        pose = gd.result()[0]                               # the parameters this iteration's forward sees
        gd.run(1)
        cur = ops.make_pano(ops.transform_cloud(xyz, pose[0:3], pose[3:6]), rgb, (h, w)).cpu().numpy().astype(np.uint8)
        new_frame = Image.new("RGB", (w, 2 * h))
        new_frame.paste(gt_img, (0, 0))
        new_frame.paste(Image.fromarray(cur), (0, h))
        frames.extend([new_frame] * (5 if it == 0 else 1))
    if new_frame is not None:
        last_frame = Image.new("RGB", (w, 2 * h))
        last_frame.paste(gt_img, (0, 0))
        frames.extend([new_frame] * 10 + [last_frame] * 5)
    return frames


def omniloc_all(img, xyz, rgb, input_trans, input_rot, cfg, scalar_summaries=None, weights=None):
    """Throughput extension: what the reference's non-parallel branch computes with
    `for i in range(num_input): omniloc(..., i, ...)` (localize.py:219-220), for ALL starting points in one launch chain.
    Every starting point keeps omniloc's SEQUENTIAL semantics (its own Adam / scheduler, clamp applied to the parameters
    the next forward reads) and the points never interact, so the list returned equals the K separate calls."""
    _refuse(cfg, "omniloc_all")
    _refuse(cfg, "omniloc_all", "pyramid")
    box = quantile_box_of(xyz, _cfg(cfg, "out_of_room_quantile", 0.05))
    res = _refine(xyz, rgb, [packed_pano(img, n_points=xyz.shape[0])], input_trans, input_rot, box, cfg, False, weights=weights).result()
    K = res.shape[0]
    R = ops.rot_from_ypr(res[:, 3:6])
    host = torch.cat([res[:, 0:3], R.reshape(K, 9), res[:, 12:13]], dim=1).cpu()
    with torch.no_grad():
        input_trans.copy_(res[:, 6:9].to(input_trans.device))
        input_rot.copy_(res[:, 9:12].to(input_rot.device))
    return [_entry(row) for row in host]


def omniloc_batch(img, xyz, rgb, input_trans, input_rot, cfg, scalar_summaries, weights=None):
    """Parallel refinement of all starting poses; returns [t (3,1), R (3,3), loss ()] of the candidate whose LAST
    forward had the smallest loss (omniloc.py:271).  Keeps the reference's clamp lag (omniloc.py:260-269): the
    returned translation is the post-step, pre-clamp value (omniloc.py:272).
    The keys that are not the reference's (what each stands next to: cfg_rules' table; neither of the last two takes a list of colour sets):
    cfg.robust_iters / robust_kind / robust_k (robust_schedule): the robust chain — the returned loss is then the WEIGHTED loss of the last
    forward, the return shapes are unchanged.
    cfg.pose_covariance (a bool): a fourth entry, cov (6, 6) on the CPU — sigma^2 H^-1 of (t, yaw, pitch, roll) at the returned pose
    (pose_information), under weights= or the robust chain's last plane; the first three entries are the run's without the key, bit for bit.
    cfg.gn_iters / gn_step_cap / gn_lambda (gn_schedule): after the chain its winner is polished on the device by gn_iters Levenberg-
    Marquardt iterations on the MEAN SQUARED residual (gauss_newton_refine: not the sampling loss), under weights= or the robust chain's
    last plane.  Where the polish accepted a step (accepted > 1, status 0 or 3) t is the polished translation, R rot_from_ypr of the
    polished angles and loss the sampling loss re-evaluated at that pose; otherwise the three entries are the chain's own, bit for bit.
    With cfg.pose_covariance the fourth entry is the polish's own cov at its returned pose.  The written-back leaves stay the chain's.
    cfg.gn_objective = "l1" (and cfg.gn_delta; gn_schedule): the polish minimises the Huber-L1 objective sum w m rho(l) / sum w m instead —
    for small delta the sampling loss itself —, with the same rules for the three entries; the fourth entry is then pose_information's
    cov at the RETURNED pose, from one plain pass after the polish (omniloc.pose_covariance's bits there).
    cfg.depth_polish = True next to cfg.depth_mask (depth_polish_flag): the gn keys and cfg.pose_covariance are taken under the mask.  The
    depth-masked chain runs as without the key; its winner is polished from the winners row on the device by gauss_newton_refine(depth=...)
    under the chain's own grid, tolerance and stride, the mask rebuilt at every trial pose; the returned loss is ops.sampling_loss(depth=...)
    at the polished pose; the covariance is the one under the mask at the returned pose.  Not with weights=, the robust or the score keys.
    cfg.pyramid_iters / pyramid_reset (pyramid_schedule): the chain runs coarse to fine over the image's PanoPyramid — the first
    pyramid_iters[0] iterations against the coarsest level, the last num_iter - pyramid_iters[-1] against the image itself, ONE optimiser
    state throughout (ops.GradientDescent.run_pyramid; with pyramid_reset the plateau scheduler starts over at every switch).  The returned
    loss is the plain sampling loss at full resolution; the gn keys and cfg.pose_covariance start from that chain's winners row and run at
    level 0, unchanged.  Not with weights=, cfg.depth_mask, the robust, score, density or prune keys; the image must be exactly k/255 and
    its sides multiples of 2^len(pyramid_iters)."""
    depth = _depth_cfg(cfg) if depth_polish_flag(cfg) else None          # (its own refusals first: without the key nothing changes)
    if depth is not None and weights is not None:
        raise ValueError("cfg.depth_polish does not combine with weights=")
    if robust_schedule(cfg) is not None and weights is not None:          # (and the schedule's own refusals, before a device is touched)
        raise ValueError("cfg.robust_iters does not combine with weights= (the chain makes its own)")
    if pyramid_schedule(cfg, getattr(img, "shape", None)) is not None and weights is not None:         # (likewise)
        raise ValueError("cfg.pyramid_iters does not combine with weights=")
    want_cov = pose_covariance_flag(cfg)
    if want_cov and isinstance(rgb, (list, tuple)):
        raise ValueError("cfg.pose_covariance: one colour set only")
    gn = gn_schedule(cfg)
    if gn is not None and isinstance(rgb, (list, tuple)):
        raise ValueError("cfg.gn_iters: one colour set only")
    if strict_reference_asserts:
        assert cfg.num_input > 1
    box = quantile_box_of(xyz, _cfg(cfg, "out_of_room_quantile", 0.05))
    pano = packed_pano(img, n_points=xyz.shape[0])
    gd = _refine(xyz, rgb, [pano], input_trans, input_rot, box, cfg, True, weights=weights, imgs=[img])
    # loss_list.argmin() of the last forward, R of the winner and the write-back of the leaves: one kernel, then the one D2H copy
    # of the whole refinement (64 bytes)
    bt, br, after = _leaf_buffers(input_trans, input_rot, gd.B)
    win = gd.winner(1, bt, br)
    # (the covariance reads the winners row on the device and changes nothing the first three entries are made from)
    if gn is not None:
        # (the polish starts from the winners row on the device; its 13 floats travel with the one D2H copy's worth of the row)
        row, cov = _winner_polish(gd, packed_cloud(xyz, rgb, weights), pano, win, gn, want_cov, depth)
        out = row.cpu()
    else:
        cov = _winner_covariance(gd, packed_cloud(xyz, rgb, weights), pano, win, depth) if want_cov else None
        out = win[0].cpu()
    after()
    ret = _entry(out)
    if want_cov:
        ret.append(cov[0].cpu())
    return ret


def _check_images(who, imgs, trans_list, rot_list, rgb):
    """The list lengths of a several-image entry point `who`, before a device is touched -> (the image count, shared_rgb(rgb))"""
    I = len(imgs)
    if I < 1 or len(trans_list) != I or len(rot_list) != I:
        raise ValueError("%s: %d images, %d / %d lists of starting poses" % (who, I, len(trans_list), len(rot_list)))
    rgb = shared_rgb(rgb)
    if isinstance(rgb, list) and len(rgb) != I:
        raise ValueError("%s: %d colour sets for %d images" % (who, len(rgb), I))
    return I, rgb


def _images_ladder(who, imgs, xyz, rgb, trans_list, rot_list, cfg, scalar_summaries, batch_mode=True, forward_one=False, direct=False,
                   weight_sets=False, polish=None):
    """How the images of ONE cloud are cut into chains, for omniloc_batch_images, _robust and _polished (each has refused the cfg keys it does
    not take): check the lists; one image may be omniloc_batch itself; per-image colour sets beyond color_set_groups' limit go group by group
    through this ladder again; else one chain (_chain_panos, the box, _refine_groups).  What the three forms differ in, as found:

        parameter      omniloc_batch_images         _robust      _polished
        batch_mode     the caller's                 True         True
        forward_one    False: one image runs the    True         True
                       chain (batch_mode=False
                       has no omniloc_batch)
        direct         True: more than 8 images     False        False
                       are packed past the cache
        weight_sets    False                        True         with the robust keys (a weight plane per image)
        polish         None                         None         (gn_schedule, want_cov): _winners_polished after the chain, and
                                                                 prune_schedule's refusals before a device is touched"""
    I, rgb = _check_images(who, imgs, trans_list, rot_list, rgb)
    if polish is not None:
        prune_schedule(cfg, int(trans_list[0].shape[0]))         # (its own refusals, before a device is touched)
    if strict_reference_asserts and batch_mode:
        assert cfg.num_input > 1
    if forward_one and I == 1:
        return [omniloc_batch(imgs[0], xyz, rgb, trans_list[0], rot_list[0], cfg, scalar_summaries)]
    if isinstance(rgb, list):
        out = _over_color_sets(int(xyz.shape[0]), I, lambda i0, i1: _images_ladder(
            who, imgs[i0:i1], xyz, rgb[i0:i1], trans_list[i0:i1], rot_list[i0:i1], cfg, scalar_summaries, batch_mode, forward_one, direct,
            weight_sets, polish))
        if out is not None:
            return out
    panos = _chain_panos(imgs, xyz.shape[0], direct=direct and I > 8)      # (else the texel format every image's own omniloc_batch call takes)
    box = quantile_box_of(xyz, _cfg(cfg, "out_of_room_quantile", 0.05))

    def chain(tr, ro):
        return _refine(xyz, rgb, panos, tr, ro, box, cfg, batch_mode, weight_sets=I if weight_sets else 0, imgs=imgs)
    if polish is None:
        return _refine_groups(chain, trans_list, rot_list)
    gn, want_cov = polish
    cloud = packed_cloud_sets(xyz, rgb) if isinstance(rgb, list) else packed_cloud(xyz, rgb)
    host = _refine_groups(chain, trans_list, rot_list, polish=lambda gd, wins: _winners_polished(gd, cloud, panos, wins, gn, want_cov))
    return [_polished_entry(row, want_cov) for row in host]


def omniloc_batch_images(imgs, xyz, rgb, input_trans_list, input_rot_list, cfg, scalar_summaries=None, batch_mode=True):
    """Throughput extension (not in the reference): omniloc_batch for SEVERAL query images of the same cloud at once.

    imgs: list of (H,W,3) images of one size; input_trans_list / input_rot_list: per image (B,3) starting poses (same B).
    The I * B candidates run through one chain of launches (shared cloud in L2, per-candidate panorama pointer), each with
    its own Adam / scheduler state, so every image gets the result omniloc_batch would give it (bit for bit when the
    cloud is cut into the same chunks, else up to the summation order of the partial sums); at 32 candidates per image,
    8 images per launch are ~25 % faster than 8 separate refinements.  Returns a list of [t, R, loss].
    The same caveat holds for a PRUNED run (cfg.prune_iters / cfg.prune_keep, prune_schedule; here and in omniloc_batch, omniloc_batch_rooms,
    omniloc_batch_rooms_images): after a prune the survivors run the plan of the smaller launch, pcl_gd_plan(n, keep), so their trajectories
    equal the unpruned run's bit for bit only where the two plans cut the cloud into the same chunks, else up to the summation order; the
    optimiser state itself crosses the prune unchanged.  Every candidate's leaf row still comes back: a dropped one's as it was when dropped.
    batch_mode=False gives every candidate omniloc's SEQUENTIAL semantics instead (what omniloc_all computes per image).
    rgb: one (N, 3) tensor, or a LIST of one per image (per-image colours, e.g. color_mod's): the cloud then holds a colour set per image
    and the chain runs the single-image plan, so image i's result is omniloc_batch(imgs[i], xyz, rgb[i], ...)'s bit for bit.  Images
    beyond the colour-set addressing limit go in further groups.  With the depth mask the colour-set chain is the depth chain
    (pcl_gd_run_depth_chain) with this cloud as its one room: the same grouping, the same bits per image.
    cfg.pyramid_iters / pyramid_reset (pyramid_schedule; omniloc_batch describes them): every image's candidates descend that image's own
    pyramid in the one chain, with shared colours or a colour set per image; image i's result is its own omniloc_batch run under the keys,
    under the plain chain's caveat above.
    ValueError, before a device is touched: lists of different lengths, a colour-set count that is not the image count."""
    _refuse(cfg, "omniloc_batch_images")
    pyramid_schedule(cfg, getattr(imgs[0], "shape", None) if imgs else None)       # (its own refusals, before a device is touched)
    return _images_ladder("omniloc_batch_images", imgs, xyz, rgb, input_trans_list, input_rot_list, cfg, scalar_summaries, batch_mode, direct=True)


def omniloc_batch_images_robust(imgs, xyz, rgb, input_trans_list, input_rot_list, cfg, scalar_summaries=None):
    """Throughput extension (not in the reference): the ROBUST omniloc_batch (cfg.robust_iters / robust_kind / robust_k, robust_schedule) for
    several query images of the same cloud in one launch chain.  Arguments, return value and write-back as omniloc_batch_images; rgb: one
    (N, 3) tensor or a list of one per image (per-image colour sets, grouped by color_set_groups).  Every image keeps a weight plane of its
    own: at every entry of robust_iters the chain takes every image's current best candidate, the residuals at its pose against that image's
    panorama (and colours), their lower median, and re-weights that image's plane — eight launches for all the images, nothing waits for the
    host.  The chain runs the single-image plan, with shared colours too, so entry i equals omniloc_batch(imgs[i], xyz, rgb_i, ...) under the
    same cfg bit for bit; every loss is the WEIGHTED loss of the last forward.  Parallel semantics only.  ValueError: cfg without
    robust_iters (and cfg_rules' refusals), cfg.visualize, lists of different lengths.  One image is omniloc_batch."""
    _refuse(cfg, "omniloc_batch_images_robust")
    _refuse(cfg, "omniloc_batch_images_robust", "pyramid")
    robust = robust_schedule(cfg)
    if robust is None:
        raise ValueError("omniloc_batch_images_robust needs cfg.robust_iters (omniloc_batch_images runs the plain chain)")
    if _cfg(cfg, "visualize", False):
        raise ValueError("omniloc_batch_images_robust does not take cfg.visualize")
    return _images_ladder("omniloc_batch_images_robust", imgs, xyz, rgb, input_trans_list, input_rot_list, cfg, scalar_summaries, forward_one=True,
                          weight_sets=True)


def omniloc_batch_images_polished(imgs, xyz, rgb, input_trans_list, input_rot_list, cfg, scalar_summaries=None):
    """Throughput extension (not in the reference): what omniloc_batch does AFTER its chain — the Levenberg-Marquardt polish of the winner
    (cfg.gn_iters / gn_step_cap / gn_lambda, gn_schedule) and / or the covariance at the returned pose (cfg.pose_covariance) — for several
    query images of one cloud at once.  Arguments, return value and write-back as omniloc_batch_images; rgb: one (N, 3) tensor or a list of
    one per image.  The chain is omniloc_batch_images'; with the robust keys omniloc_batch_images_robust's; with the prune keys a pruned
    plain chain.  Then, on the device, from the winners rows: with the gn keys ONE gauss_newton_refine_images_at_winners for all the
    images, under the robust chain's per-image weight planes where there are some; with cfg.pose_covariance a fourth entry per image, cov
    (6, 6) on the CPU — the polish's own, or pose_information_images_at_winners' when there is no polish.  One D2H copy per call; the
    written-back leaves stay the chain's.
    Entry i against omniloc_batch(imgs[i], xyz, rgb_i, ...) under the same cfg: t, R and cov are equal bit for bit (for a plain chain of
    shared colours under omniloc_batch_images' own caveat: where its plan cuts the cloud as the single call's does).  Where the polish took
    no step (it needs accepted > 1 and status 0 or 3) all three entries are the chain's own, bit for bit.  Where it took one, `loss` is
    float32(S1) / float32(M) of the polish's info record at the returned pose: the weighted sampling loss sum w m l / sum w m from the
    pass's own sums — NOT the separate forward-only launch omniloc_batch re-evaluates it with (there is none for a colour set or a
    per-image plane), so that one number differs from omniloc_batch's by the summation order.
    Parallel semantics only.  ValueError, before a device is touched: a cfg with neither the gn keys nor pose_covariance (and cfg_rules'
    refusals), cfg.visualize, lists of different lengths, a colour-set count that is not the image count.  One image is omniloc_batch;
    images beyond the colour-set addressing limit go in further groups.
    cfg.gn_objective = "l1" (and cfg.gn_delta): ONE L1 chain over all winners (gauss_newton_refine_images_at_winners(objective="l1")); a
    polished entry's loss stays float32(S1) / float32(M) of the polish's record — S1 and M are plain there, and the sampling loss is now
    what the polish works on —, and cov comes from one plain pose_information_images call at the returned poses."""
    who = "omniloc_batch_images_polished"
    gn, want_cov = gn_schedule(cfg), pose_covariance_flag(cfg)
    if gn is None and not want_cov:
        raise ValueError("%s needs cfg.gn_iters or cfg.pose_covariance (omniloc_batch_images / omniloc_batch_images_robust run the chain alone)" % who)
    if _cfg(cfg, "visualize", False):
        raise ValueError("%s does not take cfg.visualize" % who)
    _refuse(cfg, who)
    _refuse(cfg, who, "pyramid")
    return _images_ladder(who, imgs, xyz, rgb, input_trans_list, input_rot_list, cfg, scalar_summaries, forward_one=True,
                          weight_sets=robust_schedule(cfg) is not None, polish=(gn, want_cov))


def depth_tau_groups(points, H, W, cfg):
    """Which rooms may share ONE depth-masked chain: lists of room indices, in order.  A chain has one visibility tolerance, a room run on its
    own takes the tolerance of ITS grid (cfg.depth_tau, else the rule 3.5 pi / depth_h clipped to [0.02, 0.15]): rooms go together when that
    value is the same.  One group with an explicit depth_tau or depth_res, and for default grids below 80 rows (clouds below ~150k occluder
    samples: the rule's upper clip); larger rooms of different sizes split by their grids' tolerances.  Without the mask: one group."""
    d = _engine_args(cfg)
    if not d["depth_mask"] or d["depth_tau"] is not None or d["depth_res"] is not None:
        return [list(range(len(points)))]
    groups = {}
    for r, n in enumerate(points):
        groups.setdefault(ops._depth_args(int(n), H, W, None, None, d["depth_stride"])[2], []).append(r)
    return list(groups.values())


def _chain(kind, imgs, rooms, tr, ro, cfg, batch_mode):
    """One launch chain over the images `imgs` x at most PCL_GD_MAX_ROOMS rooms -> the engine, run.  kind "gd_rooms": the one image of
    ops.GradientDescentRooms; "gd_rooms_images": ops.GradientDescentRoomsImages (the two cache kinds).  `rooms`: (xyz, rgb) pairs whose rgb
    is one tensor in every room or a list of one tensor per image in every room; tr / ro: nrooms * images * per_image rows, room by room and
    image by image inside a room.  One texel format for the chain (the one the largest room's refinement would take: fp16 and RGBA8 levels
    give the same bits; float4 when the images do not agree).  Graph replay under _refine's rule on the chain's points x candidates; the
    engine is cached per room set and launch shape (_cached_engine).  With cfg.depth_mask the chain is the depth chain (every room on its own
    grid) and runs eager, as every depth-masked refinement does."""
    one_image = kind == "gd_rooms"
    per_image_sets = isinstance(rooms[0][1], list)
    clouds = [packed_cloud_sets(xyz, rgb) if per_image_sets else packed_cloud(xyz, rgb) for xyz, rgb in rooms]
    boxes = [quantile_box_of(xyz, _cfg(cfg, "out_of_room_quantile", 0.05)) for xyz, _ in rooms]
    per_room = int(tr.shape[0]) // len(rooms)
    nmax = max(int(xyz.shape[0]) for xyz, _ in rooms)
    panos = _chain_panos(imgs, nmax)
    I, p0, num_iter = len(imgs), panos[0], _cfg(cfg, "num_iter", 100)
    args = _engine_args(cfg, batch_mode)
    points = sum(c.n for c in clouds)
    sched = prune_schedule(cfg, per_room // I)

    def make(cs, bs, t, r):
        if one_image:
            return ops.GradientDescentRooms(list(zip(cs, bs)), p0, t, r, **args)
        return ops.GradientDescentRoomsImages(list(zip(cs, bs)), panos, t, r, **args)

    def name(gd, graph, fresh):
        # never on the eager path without a schedule; a new several-image engine has named its panoramas itself (as found)
        if (graph or sched is not None) and (not fresh or one_image):
            gd.set_panos(panos)                  # the pose records name these images' panoramas (the graph holds the first ones')
    return _drive(_Chain(kind=kind, key=lambda per: (I, I * per, p0.H, p0.W, p0.fmt, clouds[0].color_sets) + tuple(args.values()),
                         xyzs=tuple(xyz for xyz, _ in rooms), clouds=clouds, boxes=boxes, make=make, name=name, groups=len(rooms) * I,
                         point_poses=lambda per: points * I * per, run=lambda gd, graph: gd.run_graph(num_iter) if graph else gd.run(num_iter),
                         sched=sched, depth_mask=args["depth_mask"], replay=True), tr, ro, cfg)


def _rooms_chain(img, rooms, tr, ro, cfg, batch_mode):
    """_chain of ONE image: rgb one tensor per room, tr / ro nrooms * per_room rows"""
    return _chain("gd_rooms", [img], rooms, tr, ro, cfg, batch_mode)


def omniloc_batch_rooms(img, rooms, input_trans_list, input_rot_list, cfg, scalar_summaries=None, batch_mode=True):
    """Room search (not in the reference): omniloc_batch of ONE query image against SEVERAL rooms in one launch chain.

    rooms: list of (xyz, rgb) clouds in one frame; input_trans_list / input_rot_list: per room (B,3) starting poses (the same B for every
    room).  Returns one [t (3,1), R (3,3), loss ()] per room and writes the leaf rows back into the callers' tensors, as omniloc_batch does;
    room r's result is omniloc_batch(img, *rooms[r], ...)'s bit for bit (batch_mode=False: omniloc_all's sequential semantics, the winner of
    each room's candidates).  More than PCL_GD_MAX_ROOMS rooms go in several chains.  With the depth mask the chain is the depth chain
    (pcl_gd_run_depth_chain: every room on its own z-buffer grid, the same bits per room); rooms whose tolerances differ (depth_tau_groups)
    go in a chain per tolerance."""
    _refuse(cfg, "omniloc_batch_rooms")
    _refuse(cfg, "omniloc_batch_rooms", "pyramid")
    if strict_reference_asserts and batch_mode:
        assert cfg.num_input > 1
    R = len(rooms)
    if R == 0 or len(input_trans_list) != R or len(input_rot_list) != R:
        raise ValueError("omniloc_batch_rooms: %d rooms, %d / %d starting-pose sets" % (R, len(input_trans_list), len(input_rot_list)))
    B = int(input_trans_list[0].shape[0])
    if any(int(t.shape[0]) != B for t in input_trans_list) or any(int(r.shape[0]) != B for r in input_rot_list):
        raise ValueError("omniloc_batch_rooms: every room needs the same number of starting poses")
    # (the rooms ladder's one-image case)
    out = _rooms_ladder([img], rooms, [[t] for t in input_trans_list], [[r] for r in input_rot_list], cfg,
                        lambda *piece: _plain_leaf(*piece, cfg, scalar_summaries, batch_mode), scalar_summaries, batch_mode)
    return [o[0] for o in out]


# One chain for several images pays where a one-image chain is bound by launch latency (tools/room_images_bench.py, DESIGN.md §4.6d, ms per
# image of the chain alone, all images' chain against a chain per image): 4 rooms x 166,667 points x 6 candidates (4M point-poses per
# image) 2.72 against 3.28 with 8 images, 8 such rooms (8M) 5.21 against 5.46 — and nothing at 4 rooms x 1M points x 32 candidates (128M):
# 39.22 against 39.08, 0.4 % SLOWER with a spread of 0.1 %.  The cut-off is the size up to which a one-image chain replays a graph.
ROOMS_IMAGES_POINT_POSES = GRAPH_POINT_POSES


def rooms_images_chain_pays(points, per_image):
    """Do several images share ONE rooms chain (True) or does every image run its own (False)?  `points`: the rooms' points together."""
    return int(points) * int(per_image) <= ROOMS_IMAGES_POINT_POSES


# The same question under the depth mask for images that SHARE the rooms' colours (tools/depth_chain_bench.py; rooms of
# 166,667 points x 6 candidates, ms per (room, image), the shared depth chain against one omniloc_batch_images per room): 2 / 3 / 4 / 5 / 6 /
# 7 images 1.52 against 1.92, 1.32 / 1.54, 1.20 / 1.36, 1.22 / 1.31, 1.17 / 1.24, 1.14 / 1.19 at 4 rooms (8 rooms alike) — and 8 images 1.11
# against 0.97, 14 % SLOWER: a room's own chain of all its images cuts the cloud by the plan of 48 candidates and, with 8 images, gives every
# XCD one image's texture (pcl_gd_run's mapping for several panoramas), which the rooms launch does not have.  Measured wins up to 42
# candidates per room, the loss at 48; beyond the measured wins every room keeps its own chain.  Per-image colours always share the chain
# (their other route is one chain per room AND image: 1.12 against 2.51 ms at 8 rooms x 8 images).
DEPTH_SHARED_ROOM_CANDIDATES = 42


def depth_shared_chain_pays(nimages, per_image):
    """Under the depth mask, do several images that share the rooms' colours go into ONE rooms chain (True), or does every room run
    omniloc_batch_images over its images (False)?"""
    return int(nimages) * int(per_image) <= DEPTH_SHARED_ROOM_CANDIDATES


def _rooms_images_chain(imgs, rooms, tr, ro, cfg, batch_mode):
    """_chain of SEVERAL images: rgb one tensor in every room (the images share the room's colours) or a list of one per image in every room"""
    return _chain("gd_rooms_images", imgs, rooms, tr, ro, cfg, batch_mode)


def _check_rooms(who, imgs, rooms, input_trans, input_rot):
    """The shapes of a rooms x images entry point `who`, before a device is touched -> (R, I, B, the rooms with shared_rgb colours)"""
    R, I = len(rooms), len(imgs)
    if R == 0 or I == 0 or len(input_trans) != R or len(input_rot) != R:
        raise ValueError("%s: %d rooms, %d images, %d / %d starting-pose sets" % (who, R, I, len(input_trans), len(input_rot)))
    if any(len(t) != I for t in input_trans) or any(len(r) != I for r in input_rot):
        raise ValueError("%s: every room needs one starting-pose set per image" % who)
    B = int(input_trans[0][0].shape[0])
    if any(int(t.shape[0]) != B for ts in input_trans for t in ts) or any(int(r.shape[0]) != B for rs in input_rot for r in rs):
        raise ValueError("%s: every room and image needs the same number of starting poses" % who)
    rooms = [(xyz, shared_rgb(rgb)) for xyz, rgb in rooms]
    for _, rgb in rooms:
        if isinstance(rgb, list) and len(rgb) != I:
            raise ValueError("%s: %d colour sets for %d images" % (who, len(rgb), I))
    return R, I, B, rooms


def _rooms_ladder(imgs, rooms, trans, rot, cfg, leaf, scalar_summaries=None, batch_mode=True):
    """How images x rooms are cut into chains, for omniloc_batch_rooms (one image), omniloc_batch_rooms_images and its polished form, on
    checked arguments (rgb: shared_rgb's; trans[r][i] / rot[r][i]) -> out[r][i].  A step that cuts sends every piece down this ladder again:
      1. rooms whose depth tolerances differ go group by group (depth_tau_groups);
      2. under the depth mask, images that share the rooms' colours run omniloc_batch_images per room where that is faster
         (depth_shared_chain_pays);
      3. every image runs by itself where one chain for all is too large to gain (rooms_images_chain_pays);
      4. more than PCL_GD_MAX_ROOMS rooms go in runs of that many;
      5. per-image colour sets beyond the largest room's limit go in color_set_groups' groups;
      6. leaf(imgs, rooms, trans, rot) runs the chain of what is left.  One image or one room is the leaf's business.
    Why the order is safe for every caller: the polished form refuses the depth mask, so steps 1 and 2 never cut for it;
    rooms_images_chain_pays is monotone in the points (points x candidates <= a constant), so step 3, decided on all the rooms, comes out the
    same for every run of rooms step 4 cuts — deciding it before the room cap equals deciding it after —, and once every image runs by
    itself (or there is one image only) steps 2, 3 and 5 are inert."""
    R, I, B = len(rooms), len(imgs), int(trans[0][0].shape[0])
    points = [int(xyz.shape[0]) for xyz, _ in rooms]

    def of_rooms(idx):
        return _rooms_ladder(imgs, [rooms[r] for r in idx], [trans[r] for r in idx], [rot[r] for r in idx], cfg, leaf, scalar_summaries, batch_mode)

    def of_images(i0, i1):
        return _rooms_ladder(imgs[i0:i1], [(xyz, shared_rgb(rgb[i0:i1]) if isinstance(rgb, list) else rgb) for xyz, rgb in rooms],
                             [t[i0:i1] for t in trans], [r[i0:i1] for r in rot], cfg, leaf, scalar_summaries, batch_mode)
    groups = depth_tau_groups(points, int(imgs[0].shape[0]), int(imgs[0].shape[1]), cfg)
    if len(groups) > 1:
        return _over_room_groups(groups, of_rooms)
    sets = any(isinstance(rgb, list) for _, rgb in rooms)
    if I > 1 and not sets and bool(_cfg(cfg, "depth_mask", False)) and not depth_shared_chain_pays(I, B):
        return [omniloc_batch_images(imgs, xyz, rgb, trans[r], rot[r], cfg, scalar_summaries, batch_mode) for r, (xyz, rgb) in enumerate(rooms)]
    if I > 1 and not rooms_images_chain_pays(sum(points), B):
        return _side_by_side([1] * I, of_images, R)
    if R > ops._lib.GD_MAX_ROOMS:
        return _over_room_groups(_room_cap_groups(R), of_rooms)
    if sets:
        # one kind of cloud per chain: a room whose images share its colours holds them I times
        rooms = [(xyz, rgb if isinstance(rgb, list) else [rgb] * I) for xyz, rgb in rooms]
        out = _over_color_sets(max(points), I, of_images, R)
        if out is not None:
            return out
    return leaf(imgs, rooms, trans, rot)


def _leaf_chain(imgs, rooms, cfg, batch_mode):
    """chain(tr, ro) of one leaf of the rooms ladder: the one-image rooms chain, or the rooms x images chain"""
    if len(imgs) == 1:
        return lambda tr, ro: _rooms_chain(imgs[0], rooms, tr, ro, cfg, batch_mode)
    return lambda tr, ro: _rooms_images_chain(imgs, rooms, tr, ro, cfg, batch_mode)


def _plain_leaf(imgs, rooms, trans, rot, cfg, scalar_summaries, batch_mode):
    """The plain leaf of _rooms_ladder -> out[r][i] = [t, R, loss].  One image in one room is the single-room path itself (no concatenation,
    no per-room write-back)."""
    I, flat_t, flat_r = len(imgs), [t for ts in trans for t in ts], [r for rs in rot for r in rs]
    if len(flat_t) > 1:
        flat = _refine_groups(_leaf_chain(imgs, rooms, cfg, batch_mode), flat_t, flat_r)
    elif batch_mode:
        flat = [omniloc_batch(imgs[0], *rooms[0], flat_t[0], flat_r[0], cfg, scalar_summaries)]
    else:
        flat = omniloc_batch_images(imgs, *rooms[0], flat_t, flat_r, cfg, scalar_summaries, batch_mode=False)
    return [flat[r * I:(r + 1) * I] for r in range(len(rooms))]


def _polished_leaf(imgs, rooms, trans, rot, cfg, gn, want_cov):
    """The polished leaf of _rooms_ladder: the chain, then on the device from its winners rows ONE polish and / or information pass over all
    (room, image) winners -> out[r][i] = _polished_entry + [the chain's own winner loss] (a polished row's column 12 is the polish's)"""
    I = len(imgs)
    clouds = [packed_cloud_sets(xyz, rgb) if isinstance(rgb, list) else packed_cloud(xyz, rgb) for xyz, rgb in rooms]      # (the chain's own: cached)
    panos = _chain_panos(imgs, max(int(xyz.shape[0]) for xyz, _ in rooms))
    host = _refine_groups(_leaf_chain(imgs, rooms, cfg, True), [t for ts in trans for t in ts], [r for rs in rot for r in rs],
                          polish=lambda gd, wins: torch.cat([_polished_rows(
                              wins, gn, want_cov, lambda: ops.pose_information_rooms_at_winners(clouds, panos, wins),
                              lambda: ops.gauss_newton_refine_rooms_at_winners(clouds, panos, wins, iters=gn[0], **gn[1])), wins[:, 12:13]], dim=1))
    # (the chain's losses ride as Python floats — float32 values, exact — so that carrying them costs the host one tolist per chain)
    flat = [_polished_entry(row, want_cov) + [loss] for row, loss in zip(host, host[:, POLISHED_ROW].tolist())]
    return [flat[r * I:(r + 1) * I] for r in range(len(rooms))]


def omniloc_batch_rooms_images(imgs, rooms, input_trans, input_rot, cfg, scalar_summaries=None, batch_mode=True):
    """Room search for SEVERAL query images (not in the reference): omniloc_batch of every image against every room in one launch chain.

    imgs: list of I (H,W,3) images of one size; rooms: list of R (xyz, rgb) clouds, rgb one (N, 3) tensor (the images share the room's
    colours) or a list of I tensors (image i's own colours of that room, e.g. color_mod's); input_trans[r][i] / input_rot[r][i]: (B,3)
    starting poses of image i in room r (the same B everywhere).  Returns out[r][i] = [t (3,1), R (3,3), loss ()] and writes the leaf rows
    back into the callers' tensors, as omniloc_batch does.  out[r][i] and the leaf rows are omniloc_batch(imgs[i], xyz_r, rgb_r[i], ...)'s
    bit for bit (batch_mode=False: those of omniloc_batch_images([imgs[i]], ..., batch_mode=False)[0], the sequential semantics) for images
    whose texels are k/255 levels; for other images against the single call run with the chain's texel format (float4).
    Fallbacks: more than PCL_GD_MAX_ROOMS rooms go in several chains; with per-image colours, images beyond a room's colour-set limit
    (color_set_groups of the largest room) go in groups, each a chain of its own; one image is omniloc_batch_rooms, and so is every image of
    a chain too large to gain from sharing (rooms_images_chain_pays: the same results, a chain per image).  With the depth mask the chain is
    the depth chain (pcl_gd_run_depth_chain) under the same rules; rooms whose tolerances differ (depth_tau_groups) go in a chain per
    tolerance, and images that share the rooms' colours run omniloc_batch_images per room where that is faster (depth_shared_chain_pays:
    its plan of all the images' candidates, so equal to the single calls up to the summation order of the partial sums, as there)."""
    _refuse(cfg, "omniloc_batch_rooms_images")
    _refuse(cfg, "omniloc_batch_rooms_images", "pyramid")
    if strict_reference_asserts and batch_mode:
        assert cfg.num_input > 1
    rooms = _check_rooms("omniloc_batch_rooms_images", imgs, rooms, input_trans, input_rot)[3]
    return _rooms_ladder(imgs, rooms, input_trans, input_rot, cfg, lambda *piece: _plain_leaf(*piece, cfg, scalar_summaries, batch_mode),
                         scalar_summaries, batch_mode)


ROOMS_POLISHED_ROW = POLISHED_ROW + 1      # _winners_polished's row and the chain's own winner loss (a polished row's column 12 is the polish's)


def omniloc_batch_rooms_images_polished(imgs, rooms, input_trans, input_rot, cfg, scalar_summaries=None):
    """Room search with omniloc_batch's polish and covariance (not in the reference): omniloc_batch_rooms_images' chain — pruned under the
    prune keys —, then, on the device from its winners rows, ONE gauss_newton_refine_rooms_at_winners (cfg.gn_iters / gn_step_cap /
    gn_lambda, gn_schedule) and / or pose_information_rooms_at_winners (cfg.pose_covariance) over all (room, image) winners, and one D2H
    copy per chain.  Arguments and write-back as omniloc_batch_rooms_images (the written-back leaves stay the chain's); parallel semantics
    only.  -> (out, chain_loss): out[r][i] = [t (3,1), R (3,3), loss ()] plus cov (6,6) with cfg.pose_covariance, and chain_loss an (R, I)
    CPU tensor of the chain's own winner losses — omniloc_batch_rooms_images' losses bit for bit: what a room search decides the room by.
    out[r][i] against omniloc_batch(imgs[i], xyz_r, rgb_r[i], ...) under the same cfg: t, R and cov bit for bit (under
    omniloc_batch_rooms_images' caveat: images of k/255 levels); loss is float32(S1) / float32(M) of the polish's info record where it took
    a step (accepted > 1, status 0 or 3), else the chain's — omniloc_batch_images_polished's rule.
    omniloc_batch_rooms_images' fallbacks apply: more than PCL_GD_MAX_ROOMS rooms, images beyond the colour-set limit and chains too large
    to gain from sharing go in several chains, each polished by itself; one image runs the one-image rooms chain.
    ValueError, before a device is touched: a cfg with neither the gn keys nor pose_covariance (and cfg_rules' refusals), ragged lists."""
    who = "omniloc_batch_rooms_images_polished"
    gn, want_cov = gn_schedule(cfg), pose_covariance_flag(cfg)
    _refuse_l1(gn, who)
    if gn is None and not want_cov:
        raise ValueError("%s needs cfg.gn_iters or cfg.pose_covariance (omniloc_batch_rooms_images runs the chain alone)" % who)
    if bool(_cfg(cfg, "depth_mask", False)):
        raise ValueError("%s does not combine with cfg.depth_mask" % who)
    _refuse(cfg, who)
    _refuse(cfg, who, "pyramid")
    if _cfg(cfg, "visualize", False):
        raise ValueError("%s does not take cfg.visualize" % who)
    _, _, B, rooms = _check_rooms(who, imgs, rooms, input_trans, input_rot)
    prune_schedule(cfg, B)                                   # (its own refusals, before a device is touched)
    if strict_reference_asserts:
        assert cfg.num_input > 1
    out = _rooms_ladder(imgs, rooms, input_trans, input_rot, cfg, lambda *piece: _polished_leaf(*piece, cfg, gn, want_cov))
    # (every entry carries the chain's own winner loss last: taken apart here, after the ladder has stitched the pieces)
    chain_loss = torch.tensor([[entry.pop() for entry in row] for row in out], dtype=torch.float32)
    return out, chain_loss


def sampling_loss(img, xyz, rgb, input_trans, input_rot, starting_point, cfg, return_list=True, weights=None):
    """Forward-only loss of one starting pose — omniloc.py:105-157.  weights: (N,) per-point weights (not with cfg.depth_mask)."""
    if weights is not None and _depth_cfg(cfg):
        raise ValueError("per-point weights do not combine with cfg.depth_mask")
    cloud, pano = packed_cloud(xyz, rgb, weights), packed_pano(img)
    t, r = input_trans[starting_point], input_rot[starting_point]
    res = ops.sampling_loss(cloud, pano, t, r, with_grad=False, depth=_depth_cfg(cfg))[0]
    loss = res[0].cpu()
    if return_list:
        return [t.detach().reshape(3, 1).cpu().clone(), _rot_matrix(ops._dev(r)).cpu(), loss]
    return loss


def _depth_cfg(cfg):
    """None (the reference's loss), or the depth-mask arguments of ops.sampling_loss from cfg.depth_mask / depth_res / depth_tau —
    the same mask one iteration of the GD loop uses for these poses."""
    if not bool(_cfg(cfg, "depth_mask", False)):
        return None
    return {"depth_res": _cfg(cfg, "depth_res", None), "depth_tau": _cfg(cfg, "depth_tau", None), "depth_stride": _cfg(cfg, "depth_stride", None),
            "on": True}


# ------------------------------------------------------------------------------------------------ nn.Modules
class _LossFn(torch.autograd.Function):
    """loss_b(t_b, ypr_b) for B poses; the fused kernel returns loss and gradient together, backward just scales."""

    @staticmethod
    def forward(ctx, cloud, pano, trans, rot, depth=None):
        res = ops.sampling_loss(cloud, pano, trans, rot, with_grad=True, depth=depth)
        ctx.save_for_backward(res[:, 2:5], res[:, 5:8])
        ctx.devs = (trans.device, rot.device)
        return res[:, 0].to(trans.device)

    @staticmethod
    def backward(ctx, grad_loss):
        gt, gr = ctx.saved_tensors
        g = grad_loss.to(gt.device).reshape(-1, 1)
        return None, None, (g * gt).to(ctx.devs[0]), (g * gr).to(ctx.devs[1]), None


class SamplingLoss(nn.Module):
    """omniloc.py:160-202.  forward(translation (3,1), yaw (1,), pitch (1,), roll (1,)) -> scalar loss."""

    def __init__(self, xyz, rgb, img, device, cfg, weights=None):
        super().__init__()
        self.xyz, self.rgb, self.img, self.cfg = xyz, rgb, img, cfg
        if weights is not None and _depth_cfg(cfg):
            raise ValueError("per-point weights do not combine with cfg.depth_mask")
        self._cloud, self._pano = ops.Cloud(xyz, rgb, weights=weights), ops.Pano(img)

    def forward(self, translation, yaw, pitch, roll):
        trans = translation.reshape(1, 3)
        rot = torch.cat([yaw.reshape(1), pitch.reshape(1), roll.reshape(1)]).reshape(1, 3)
        return _LossFn.apply(self._cloud, self._pano, trans, rot, _depth_cfg(self.cfg))[0]


class BatchSamplingLoss(nn.Module):
    """omniloc.py:299-356.  forward(translation (B,3,1), yaw (B,1), pitch (B,1), roll (B,1)) -> (sum, (B,) list)."""

    def __init__(self, xyz, rgb, img, device, cfg, weights=None):
        super().__init__()
        self.xyz, self.rgb, self.img, self.cfg = xyz, rgb, img, cfg
        self.num_input = cfg.num_input
        if weights is not None and _depth_cfg(cfg):
            raise ValueError("per-point weights do not combine with cfg.depth_mask")
        self._cloud, self._pano = ops.Cloud(xyz, rgb, weights=weights), ops.Pano(img)

    def forward(self, translation, yaw, pitch, roll):
        B = translation.shape[0]
        if B != self.num_input:
            # the reference's (num_input,1) constant tensors make any other batch size a shape error (omniloc.py:307-318)
            raise RuntimeError("BatchSamplingLoss: batch size %d != cfg.num_input %d" % (B, self.num_input))
        trans = translation.reshape(B, 3)
        rot = torch.cat([yaw.reshape(B, 1), pitch.reshape(B, 1), roll.reshape(B, 1)], dim=1)
        loss_list = _LossFn.apply(self._cloud, self._pano, trans, rot, _depth_cfg(self.cfg))
        return loss_list.sum(), loss_list
