"""The cfg keys that are not the reference's, all absent by default: what a value may be, what a key needs beside it, what it may not stand
next to, and which chain a dataset loop routes a run through.  Host only — no device, no file —, so every ValueError here comes first.

    family           needs                      excludes                                      route of the loops; entry points that take it
    prune            both its keys              the robust keys                               any; every batch refinement
    robust           robust_iters               depth_mask, weights=, images_per_launch > 1,  "robust", groups of robust_images_per_launch (parallel);
                                                room_search[_images]                          omniloc_batch, omniloc_batch_images_robust / _polished
    pose_covariance  a bool                     depth_mask, colour-set lists;                 "polished", groups of polish_images_per_launch (parallel; not with
    gn               gn_iters; gn_delta: "l1"   "l1": the rooms forms                         room_search[_images], robust_images_per_launch, images_per_launch
                                                                                              > 1), or "rooms-polished": room_search + room_search_polish
                                                                                              (parallel); omniloc_batch and the *_polished entry points
    score            score_weights = True       every grouping key, robust, room_search,      "scored", one image per launch chain; no entry point (weights=)
                                                depth_mask
    depth_polish     depth_mask, and gn_iters   robust, score, weights=; lifts "depth_mask"   none: both loops refuse it; omniloc_batch alone (and through it
                     and / or pose_covariance   from the gn and pose_covariance rows          localize.refine_image's parallel branch)
    density          density_weights = True     what score excludes, and score                "plain", one image per launch chain, refined under
                     and density_voxel                                                        omniloc.density_weights_of; no entry point (weights=)
    voxel            voxel_size                 nothing: the down-sampled cloud is a cloud    any: localize._read_cloud applies it once per room; the
                                                                                              synthetic driver refuses it (utils.voxel_downsample)
    align            align_cloud = True and     nothing: the aligned cloud is a cloud         any: localize._read_cloud aligns every room once, before the
                     gravity_aligned = False                                                  voxel keys; results are mapped back to the cloud's own frame;
                                                                                              the synthetic driver refuses it (utils.align_cloud)
    pyramid          pyramid_iters (an int or   depth_mask, weights=, the robust, score,      "plain" (parallel), any images_per_launch; omniloc_batch (next to
                     a list: 1 .. 4 switches)   density and prune keys, room_search           the gn keys and pose_covariance, which run at level 0),
                                                                                              omniloc_batch_images and localize.refine_image's parallel branch

An entry point refuses the families it does not take with one _refuse(cfg, its name) (REFUSES) and validates the ones it does with their
schedules; a dataset loop resolves its cfg once, with dataset_plan, and dispatches on the plan."""
import collections

from . import ops


def _cfg(cfg, key, default):
    return getattr(cfg, key, default)


# family -> (its keys, how a refusal names them — None: the first key it finds, what does take them)
ROBUST_KEYS = ("robust_iters", "robust_kind", "robust_k")
GN_KEYS = ("gn_iters", "gn_step_cap", "gn_lambda", "gn_objective", "gn_delta")
SCORE_KEYS = ("score_weights", "score_split", "score_floor", "score_min_count")
DENSITY_KEYS = ("density_weights", "density_voxel", "density_cap")
VOXEL_KEYS = ("voxel_size", "voxel_how")
VOXEL_HOW = ("centroid", "first")
ALIGN_KEYS = ("align_cloud", "align_voxel", "align_max_tilt", "align_yaw", "align_min_count")
PYRAMID_KEYS = ("pyramid_iters", "pyramid_reset")
_EXTENSIONS = {
    "prune": (("prune_iters", "prune_keep"), "prune_iters / cfg.prune_keep", "the batch refinements do"),
    "robust": (ROBUST_KEYS, None, "omniloc_batch, omniloc_batch_images_robust, omniloc_batch_images_polished and localize.refine_image's parallel "
                                  "branch do"),
    "pose_covariance": (("pose_covariance",), None, "omniloc_batch, omniloc_batch_images_polished, omniloc_batch_rooms_images_polished and "
                                                    "localize.refine_image's parallel branch do; the dataset loops with "
                                                    "cfg.polish_images_per_launch, a room search with cfg.room_search_polish"),
    "gn": (GN_KEYS, None, "omniloc_batch, omniloc_batch_images_polished, omniloc_batch_rooms_images_polished and localize.refine_image's parallel "
                          "branch do; the dataset loops with cfg.polish_images_per_launch, a room search with cfg.room_search_polish"),
    "score": (SCORE_KEYS, None, "the known-room dataset loops do, one image per launch chain; elsewhere pass weights=score_weights(score_maps(...))"),
    "density": (DENSITY_KEYS, None, "the known-room dataset loops do, one image per launch chain; elsewhere pass "
                                    "weights=density_weights(xyz, voxel, cap)"),
    "voxel": (VOXEL_KEYS, None, "the dataset loops do, once per room as its cloud is read; elsewhere down-sample the cloud with "
                                "utils.voxel_downsample"),
    "depth_polish": (("depth_polish",), None, "omniloc_batch and localize.refine_image's parallel branch do"),
    "align": (ALIGN_KEYS, None, "the dataset loops do, once per room as its cloud is read; elsewhere align the cloud with utils.align_cloud"),
    "pyramid": (PYRAMID_KEYS, None, "omniloc_batch, omniloc_batch_images and localize.refine_image's parallel branch do; the known-room dataset "
                                    "loops on their plain route"),
}
# The families an entry point refuses, in the order it looks for them: it returns every candidate, records frames, or runs a chain without the
# robust plane, the covariance or the polish.  omniloc_batch must go on accepting the score and density keys: refine_image hands it the
# scored and the density-weighted loops' cfg.  The voxel keys travel with every loop's cfg: only the synthetic driver, which reads no cloud,
# refuses them.
REFUSES = {
    "omniloc": ("prune", "robust", "pose_covariance", "gn", "depth_polish"),
    "omniloc_all": ("prune", "robust", "pose_covariance", "gn", "depth_polish"),
    "omniloc_batch": (),
    "omniloc_batch_images": ("robust", "pose_covariance", "gn", "score", "density", "depth_polish"),
    "omniloc_batch_images_robust": ("pose_covariance", "gn", "score", "density", "depth_polish"),
    "omniloc_batch_images_polished": ("score", "density", "depth_polish"),
    "omniloc_batch_rooms": ("robust", "pose_covariance", "gn", "score", "density", "depth_polish"),
    "omniloc_batch_rooms_images": ("robust", "pose_covariance", "gn", "score", "density", "depth_polish"),
    "omniloc_batch_rooms_images_polished": ("robust", "score", "density", "depth_polish"),
    "localize_synthetic": ("pose_covariance", "gn", "score", "density", "voxel", "align", "depth_polish"),
    "localize_stanford": ("pose_covariance", "gn", "depth_polish"),
    "localize_omniscenes": ("pose_covariance", "gn", "depth_polish"),
}


def _refuse(cfg, who, *families):
    """ValueError for the first key cfg carries of the families `who` does not take (REFUSES[who], or the `families` given)"""
    for keys, named, takers in map(_EXTENSIONS.get, families or REFUSES[who]):
        for key in keys:
            if _cfg(cfg, key, None) is not None:
                raise ValueError("%s does not take cfg.%s (%s)" % (who, named or key, takers))


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _int_list(cfg, name):
    """cfg.`name`, an int or a list of ints, as a list"""
    v = _cfg(cfg, name, None)
    v = list(v) if isinstance(v, (list, tuple)) else [v]
    if not v or not all(_is_int(x) for x in v):
        raise ValueError("cfg.%s: an int or a list of ints, got %r" % (name, v))
    return v


def _inside_num_iter(iters, name, num_iter):
    if any(not 0 < i < num_iter for i in iters) or any(b <= a for a, b in zip(iters, iters[1:])):
        raise ValueError("cfg.%s %r: strictly increasing iteration counts inside (0, %d)" % (name, iters, num_iter))


def _positive(v, name):
    if not isinstance(v, (int, float)) or isinstance(v, bool) or not (0.0 < float(v) < float("inf")):
        raise ValueError("cfg.%s %r: a positive finite number" % (name, v))
    return float(v)


def _count(cfg, key):
    v = _cfg(cfg, key, None)
    if not _is_int(v) or v < 1:
        raise ValueError("cfg.%s %r: an int >= 1" % (key, v))
    return v


def _switch(cfg, key):
    v = _cfg(cfg, key, None)
    if v is not None and not isinstance(v, bool):
        raise ValueError("cfg.%s %r: a bool" % (key, v))
    return bool(v)


# ------------------------------------------------------------------------------------------------ combinations, each stated once
def _no_depth_mask(cfg, key, polish=False):
    """polish: `key` belongs to a family that cfg.depth_polish = True takes under the mask (depth_polish_flag holds the rest of that rule)"""
    if bool(_cfg(cfg, "depth_mask", False)) and not (polish and _cfg(cfg, "depth_polish", None) is True):
        raise ValueError("cfg.%s does not combine with cfg.depth_mask" % key)


def _needs_parallel(cfg, key, chain):
    if not _cfg(cfg, "parallel", False):
        raise ValueError("cfg.%s needs cfg.parallel (the %s chain has parallel semantics only)" % (key, chain))


def _polished_run(cfg, key, otherwise):
    _needs_parallel(cfg, key, "polished")
    if all(_cfg(cfg, k, None) is None for k in GN_KEYS) and not _cfg(cfg, "pose_covariance", None):
        raise ValueError("cfg.%s goes with cfg.gn_iters and / or cfg.pose_covariance (%s)" % (key, otherwise))


def _excludes(cfg, key, others):
    for other in others:
        if _cfg(cfg, other, None):
            raise ValueError("cfg.%s does not combine with cfg.%s" % (key, other))


def _one_image_per_launch(cfg, key, why):
    if int(_cfg(cfg, "images_per_launch", 1)) > 1:
        raise ValueError("cfg.%s does not combine with images_per_launch > 1 (%s)" % (key, why))


def prune_schedule(cfg, per_image):
    """The segments [(iterations, candidates per image), ...] of a refinement of `per_image` candidates per image under cfg.prune_iters /
    cfg.prune_keep (an int each, or lists of equal length), or None when the keys are absent.  prune_iters = 20, 40 with prune_keep = 16, 8
    at num_iter 100 and 32 candidates: [(20, 32), (20, 16), (60, 8)].  Host only."""
    iters, keep = _cfg(cfg, "prune_iters", None), _cfg(cfg, "prune_keep", None)
    if iters is None and keep is None:
        return None
    if iters is None or keep is None:
        raise ValueError("cfg.prune_iters and cfg.prune_keep go together")
    iters, keep = _int_list(cfg, "prune_iters"), _int_list(cfg, "prune_keep")
    num_iter, per_image = int(_cfg(cfg, "num_iter", 100)), int(per_image)
    if len(iters) != len(keep):
        raise ValueError("cfg.prune_iters has %d entries, cfg.prune_keep %d" % (len(iters), len(keep)))
    _inside_num_iter(iters, "prune_iters", num_iter)
    cap = ops._lib.GD_PRUNE_MAX
    if per_image > cap:
        raise ValueError("pruning takes at most %d candidates per image, got %d" % (cap, per_image))
    if any(not 1 <= k <= per_image for k in keep) or any(b > a for a, b in zip(keep, keep[1:])):
        raise ValueError("cfg.prune_keep %r: non-increasing counts in 1 .. %d" % (keep, per_image))
    ends, counts = iters + [num_iter], [per_image] + keep
    return [(e - b, c) for b, e, c in zip([0] + iters, ends, counts)]


def robust_schedule(cfg):
    """(robust_iters as a list, kind, k) of a refinement under cfg.robust_iters (an int, or a strictly increasing list inside (0, num_iter)),
    cfg.robust_kind ("trunc", the default, or "huber") and cfg.robust_k (default 2.5), or None when the keys are absent.  The chain's
    segments end at robust_iters + [num_iter]: [4, 8] at num_iter 12 runs 4 unweighted, 4 and 4 weighted iterations.  Host only."""
    iters, kind, k = (_cfg(cfg, key, None) for key in ROBUST_KEYS)
    if iters is None and kind is None and k is None:
        return None
    if iters is None:
        raise ValueError("cfg.%s goes with cfg.robust_iters" % ("robust_kind" if kind is not None else "robust_k"))
    iters = _int_list(cfg, "robust_iters")
    _inside_num_iter(iters, "robust_iters", int(_cfg(cfg, "num_iter", 100)))
    kind = "trunc" if kind is None else kind
    if kind not in ops.ROBUST_KINDS:
        raise ValueError("cfg.robust_kind %r: one of %s" % (kind, sorted(ops.ROBUST_KINDS)))
    k = _positive(2.5 if k is None else k, "robust_k")
    _no_depth_mask(cfg, "robust_iters")
    if _cfg(cfg, "prune_iters", None) is not None or _cfg(cfg, "prune_keep", None) is not None:
        raise ValueError("cfg.robust_iters does not combine with cfg.prune_iters / cfg.prune_keep")
    return iters, kind, k


def pyramid_schedule(cfg, shape=None):
    """(pyramid_iters as a list, pyramid_reset) of a coarse-to-fine refinement under cfg.pyramid_iters (an int, or a strictly increasing
    list inside (0, num_iter): one entry per coarse level, at most ops.PYRAMID_MAX_LEVELS) and cfg.pyramid_reset (a bool, default False:
    the plateau scheduler carries on across the levels), or None when the keys are absent.  [10, 30] at num_iter 100 runs 10 iterations
    on level 2, 20 on level 1 and 70 on the image itself.  shape: the query image's (H, W), where it is known — both must be multiples
    of 2^len(pyramid_iters).  The keys exclude cfg.depth_mask and the robust, score, density and prune keys (weights= is an argument:
    the entry points refuse it beside the keys).  Host only."""
    iters, reset = (_cfg(cfg, key, None) for key in PYRAMID_KEYS)
    if iters is None:
        if reset is not None:
            raise ValueError("cfg.pyramid_reset goes with cfg.pyramid_iters")
        return None
    iters = _int_list(cfg, "pyramid_iters")
    _inside_num_iter(iters, "pyramid_iters", int(_cfg(cfg, "num_iter", 100)))
    if len(iters) > ops.PYRAMID_MAX_LEVELS:
        raise ValueError("cfg.pyramid_iters %r: at most %d coarse levels" % (iters, ops.PYRAMID_MAX_LEVELS))
    reset = _switch(cfg, "pyramid_reset")
    _no_depth_mask(cfg, "pyramid_iters")
    _excludes(cfg, "pyramid_iters", ROBUST_KEYS + SCORE_KEYS + DENSITY_KEYS + ("prune_iters", "prune_keep"))
    if shape is not None:
        ops.pyramid_shape(int(shape[0]), int(shape[1]), len(iters), "cfg.pyramid_iters %r" % (iters,))
    return iters, reset


def pose_covariance_flag(cfg):
    """cfg.pose_covariance as a bool (absent or None: False).  ValueError: a value that is not a bool, cfg.depth_mask next to it.  Host only."""
    v = _switch(cfg, "pose_covariance")
    if v:
        _no_depth_mask(cfg, "pose_covariance", polish=True)
    return v


def gn_schedule(cfg):
    """(iters, keyword dict for ops.gauss_newton_refine) under cfg.gn_iters / gn_step_cap / gn_lambda / gn_objective / gn_delta, or None when
    the keys are absent.  Without gn_objective, or with "l2", the dict holds hyper-parameters alone, as before the key; with "l1" it gains
    objective="l1" (and delta= when cfg.gn_delta, inside [2^-20, 4], is given).  Host only."""
    iters, cap, lam, objective, delta = (_cfg(cfg, key, None) for key in GN_KEYS)
    if iters is None and cap is None and lam is None and objective is None and delta is None:
        return None
    if objective is not None and (not isinstance(objective, str) or objective not in ops.GN_OBJECTIVES):
        raise ValueError("cfg.gn_objective %r: one of %s" % (objective, list(ops.GN_OBJECTIVES)))
    if iters is None:
        raise ValueError("cfg.%s goes with cfg.gn_iters" % next(key for key, v in zip(GN_KEYS[1:], (cap, lam, objective, delta)) if v is not None))
    if delta is not None:
        if objective != "l1":
            raise ValueError('cfg.gn_delta goes with cfg.gn_objective = "l1"')
        delta = _positive(delta, "gn_delta")
        try:
            ops.gn_objective("cfg.gn_delta", "l1", delta)
        except ValueError as e:
            raise ValueError("cfg.gn_delta: %s" % e) from None
    if not _is_int(iters) or not 1 <= iters <= ops.GN_MAX_ITERS:
        raise ValueError("cfg.gn_iters %r: an int in 1 .. %d" % (iters, ops.GN_MAX_ITERS))
    hyper = {}
    for key, name, v in (("gn_step_cap", "step_cap", cap), ("gn_lambda", "lam0", lam)):
        if v is not None:
            hyper[name] = _positive(v, key)
    try:
        ops.gn_hyper("cfg.gn_step_cap / cfg.gn_lambda", **hyper)          # (what float32 makes of them)
    except ValueError as e:
        raise ValueError("cfg.gn_step_cap / cfg.gn_lambda: %s" % e) from None
    _no_depth_mask(cfg, "gn_iters", polish=True)
    if objective == "l1":
        hyper["objective"] = "l1"
        if delta is not None:
            hyper["delta"] = delta
    return iters, hyper


def depth_polish_flag(cfg):
    """cfg.depth_polish as a bool (absent or None: False): with cfg.depth_mask the winner of omniloc_batch's depth-masked chain is polished
    (the gn keys) and / or gets its covariance (cfg.pose_covariance) UNDER THE MASK, rebuilt at every trial pose.  ValueError: a value
    that is not a bool; set without cfg.depth_mask, without any of the gn keys or cfg.pose_covariance, next to the robust or score keys.
    (weights= is an argument, not a key: omniloc_batch refuses it beside the switch.)  Host only."""
    if not _switch(cfg, "depth_polish"):
        return False
    if not bool(_cfg(cfg, "depth_mask", False)):
        raise ValueError("cfg.depth_polish goes with cfg.depth_mask (without the mask the gn keys and cfg.pose_covariance need no switch)")
    if all(_cfg(cfg, k, None) is None for k in GN_KEYS) and not _cfg(cfg, "pose_covariance", None):
        raise ValueError("cfg.depth_polish goes with cfg.gn_iters and / or cfg.pose_covariance (cfg.depth_mask alone runs the plain depth chain)")
    _excludes(cfg, "depth_polish", ROBUST_KEYS + SCORE_KEYS)
    return True


def _refuse_l1(gn, who):
    """the rooms forms have no L1 twin"""
    if gn is not None and gn[1].get("objective") == "l1":
        raise ValueError('%s does not take cfg.gn_objective = "l1" (the rooms polish has no L1 form; omniloc_batch and '
                         'omniloc_batch_images_polished do)' % who)


# ------------------------------------------------------------------------------------------------ the dataset loops' keys
def score_rules(cfg):
    """cfg.score_weights = True (a known-room loop initialises every image with make_input_scored and refines it under omniloc.score_weights of
    its maps) with cfg.score_split ([num_split_h >= 3, num_split_w >= 1]: the maps' own split, default the initialisation's), score_floor (a
    number in [0, 1), default 0) and score_min_count (an int >= 1, default 1) -> None without the keys, else (split or None, floor, min_count)"""
    others = [key for key in SCORE_KEYS[1:] if _cfg(cfg, key, None) is not None]
    if not _switch(cfg, "score_weights"):
        if others:
            raise ValueError("cfg.%s goes with cfg.score_weights = True" % others[0])
        return None
    split = _cfg(cfg, "score_split", None)
    if split is not None:
        if not isinstance(split, (list, tuple)) or len(split) != 2 or not all(_is_int(v) for v in split) or split[0] < 3 or split[1] < 1:
            raise ValueError("cfg.score_split %r: [num_split_h >= 3, num_split_w >= 1]" % (split,))
        split = (int(split[0]), int(split[1]))
    floor = _cfg(cfg, "score_floor", None)
    if floor is not None and (not isinstance(floor, (int, float)) or isinstance(floor, bool) or not 0.0 <= float(floor) < 1.0):
        raise ValueError("cfg.score_floor %r: a number in [0, 1)" % (floor,))
    min_count = 1 if "score_min_count" not in others else _count(cfg, "score_min_count")
    _one_image_per_launch(cfg, "score_weights", "one image per launch chain")
    _excludes(cfg, "score_weights", ROBUST_KEYS + ("robust_images_per_launch", "polish_images_per_launch", "room_search", "room_search_images",
                                                   "depth_mask"))
    return split, 0.0 if floor is None else float(floor), min_count


def density_rules(cfg):
    """cfg.density_weights = True (a known-room loop refines every image under omniloc.density_weights_of(xyz, density_voxel, density_cap):
    every occupied voxel of cfg.density_voxel metres votes once, or at most density_cap times) with cfg.density_voxel (required: a positive
    finite number) and cfg.density_cap (an int >= 1, default 1) -> None without the keys, else (voxel, cap).  It excludes what the score
    keys exclude, and the score keys."""
    others = [key for key in DENSITY_KEYS[1:] if _cfg(cfg, key, None) is not None]
    if not _switch(cfg, "density_weights"):
        if others:
            raise ValueError("cfg.%s goes with cfg.density_weights = True" % others[0])
        return None
    if "density_voxel" not in others:
        raise ValueError("cfg.density_weights goes with cfg.density_voxel (the voxel's edge in metres)")
    voxel = _positive(_cfg(cfg, "density_voxel", None), "density_voxel")
    cap = 1 if "density_cap" not in others else _count(cfg, "density_cap")
    _one_image_per_launch(cfg, "density_weights", "one image per launch chain")
    _excludes(cfg, "density_weights", SCORE_KEYS + ROBUST_KEYS + ("robust_images_per_launch", "polish_images_per_launch", "room_search",
                                                                   "room_search_images", "depth_mask"))
    return voxel, cap


def voxel_rules(cfg):
    """cfg.voxel_size (a positive finite number: the cloud of every room is replaced by its voxel grid's points as it is read, after
    sample_rate and before everything else) with cfg.voxel_how ("centroid", the default, or "first") -> None without the keys, else
    (voxel, how)"""
    size, how = _cfg(cfg, "voxel_size", None), _cfg(cfg, "voxel_how", None)
    if size is None:
        if how is not None:
            raise ValueError("cfg.voxel_how goes with cfg.voxel_size")
        return None
    size = _positive(size, "voxel_size")
    how = VOXEL_HOW[0] if how is None else how
    if not isinstance(how, str) or how not in VOXEL_HOW:
        raise ValueError("cfg.voxel_how %r: one of %s" % (how, list(VOXEL_HOW)))
    return size, how


AlignRules = collections.namedtuple("AlignRules", "voxel max_tilt yaw min_count")


def align_rules(cfg):
    """cfg.align_cloud = True (the cloud of every room is turned, as it is read — after sample_rate and before voxel_size —, so that its up
    direction is +z: utils.align_cloud; every result is mapped back to the cloud's own frame) with cfg.align_voxel (a positive number, at
    most 2, default 0.1), align_max_tilt (degrees in (0, 45], default 40), align_yaw (a bool: the walls along the axes too, default off) and
    align_min_count (an int >= 3, default 8) -> None without the keys, else AlignRules(voxel, max_tilt, yaw, min_count).  It needs
    cfg.gravity_aligned = False beside it: on a cloud that is declared aligned there is nothing to align.  (gravity_aligned = False
    WITHOUT the switch stays the NotImplementedError of localize._require_gravity_aligned.)"""
    others = [key for key in ALIGN_KEYS[1:] if _cfg(cfg, key, None) is not None]
    if not _switch(cfg, "align_cloud"):
        if others:
            raise ValueError("cfg.%s goes with cfg.align_cloud = True" % others[0])
        return None
    if _cfg(cfg, "gravity_aligned", True):
        raise ValueError("cfg.align_cloud goes with cfg.gravity_aligned = False (a cloud declared gravity-aligned has nothing to align)")
    voxel = 0.1 if "align_voxel" not in others else _positive(_cfg(cfg, "align_voxel", None), "align_voxel")
    if voxel > ops.ALIGN_MAX_VOXEL:
        raise ValueError("cfg.align_voxel %r: at most %g (metres)" % (voxel, ops.ALIGN_MAX_VOXEL))
    tilt = _cfg(cfg, "align_max_tilt", None)
    if tilt is not None and (not isinstance(tilt, (int, float)) or isinstance(tilt, bool) or not 0.0 < float(tilt) <= 45.0):
        raise ValueError("cfg.align_max_tilt %r: degrees in (0, 45]" % (tilt,))
    min_count = _cfg(cfg, "align_min_count", None)
    if min_count is not None and (not _is_int(min_count) or min_count < 3):
        raise ValueError("cfg.align_min_count %r: an int >= 3" % (min_count,))
    return AlignRules(voxel, 40.0 if tilt is None else float(tilt), _switch(cfg, "align_yaw"), 8 if min_count is None else int(min_count))


def robust_rules(cfg):
    """The robust keys in a dataset loop; cfg.robust_images_per_launch (an int >= 1) is such a run's group size."""
    if _cfg(cfg, "robust_images_per_launch", None) is not None:
        _count(cfg, "robust_images_per_launch")
        if _cfg(cfg, "robust_iters", None) is None:
            raise ValueError("cfg.robust_images_per_launch goes with cfg.robust_iters (images_per_launch groups a plain run)")
        _needs_parallel(cfg, "robust_images_per_launch", "robust")
    for key in ROBUST_KEYS:
        if _cfg(cfg, key, None) is not None:
            _one_image_per_launch(cfg, key, "a robust run groups its images with robust_images_per_launch")
            _excludes(cfg, key, ("room_search", "room_search_images"))
            robust_schedule(cfg)
            return


def polish_rules(cfg, who):
    """The gn keys and cfg.pose_covariance in the dataset loop `who`: refused without cfg.polish_images_per_launch, the group size of a
    known-room run through omniloc_batch_images_polished (a robust polished run's too).  -> the group size, or None without the key"""
    if _cfg(cfg, "polish_images_per_launch", None) is None:
        _refuse(cfg, who)
        return None
    ppl = _count(cfg, "polish_images_per_launch")
    _polished_run(cfg, "polish_images_per_launch", "images_per_launch groups a plain run")
    _excludes(cfg, "polish_images_per_launch", ("room_search", "room_search_images", "robust_images_per_launch"))
    _one_image_per_launch(cfg, "polish_images_per_launch", "it is the polished run's group size")
    gn_schedule(cfg)
    pose_covariance_flag(cfg)
    return int(ppl)


def room_polish_rules(cfg):
    """cfg.room_search_polish = True lets a room search carry the gn keys and / or cfg.pose_covariance: every group then goes through
    omniloc_batch_rooms_images_polished.  -> whether the key is set (without it the loop refuses those keys)"""
    if not _switch(cfg, "room_search_polish"):
        return False
    if not _cfg(cfg, "room_search", None):
        raise ValueError("cfg.room_search_polish goes with cfg.room_search (polish_images_per_launch polishes a known-room run)")
    if _cfg(cfg, "polish_images_per_launch", None) is not None:
        raise ValueError("cfg.polish_images_per_launch does not combine with cfg.room_search")
    _polished_run(cfg, "room_search_polish", "room_search alone runs the plain search")
    _refuse_l1(gn_schedule(cfg), "cfg.room_search_polish")
    pose_covariance_flag(cfg)
    return True


def group_size(cfg):
    """images per group of a known-room loop: cfg.polish_images_per_launch where set (a robust polished run too), else under the robust keys
    cfg.robust_images_per_launch (default 1), else cfg.images_per_launch"""
    if _cfg(cfg, "polish_images_per_launch", None) is not None:
        return int(cfg.polish_images_per_launch)
    if _cfg(cfg, "robust_iters", None) is not None:
        return int(_cfg(cfg, "robust_images_per_launch", None) or 1)
    return int(_cfg(cfg, "images_per_launch", 1))


def on(cfg, key):
    """whether cfg sets the switch `key` (parallel, pose_covariance, room_search_polish), for code that does not validate it itself"""
    return bool(_cfg(cfg, key, None))


class DatasetPlan(collections.namedtuple("DatasetPlan", "route group_size parallel score room_search sigmas")):
    """dataset_plan's answer; .align is align_rules' answer, None without the align keys.  It is an attribute, not a field — the tuple keeps
    its six, which older tests pin —, so `==`, iteration and a plain tuple(plan) do not see it; with_align and _replace carry it."""
    align = None

    def with_align(self, align):
        plan = DatasetPlan(*self)
        plan.align = align
        return plan

    def _replace(self, **fields):
        return DatasetPlan(*super()._replace(**fields)).with_align(self.align)


def dataset_plan(cfg, loop):
    """What `loop` ("localize_stanford" / "localize_omniscenes") does with cfg, decided once, before any file is read: the rules above in
    the loop's order — align, score, density, voxel, robust, the room search's polish (Stanford) else the known-room polish, room_search x
    images_per_launch —, then route (plain | robust | polished | scored, or Stanford's rooms | rooms-polished), group_size (images per
    localize_group call), parallel,
    score (score_rules' triple or None), room_search (cfg's, where the loop searches: localize_omniscenes ignores the room-search keys) and
    sigmas (every result carries a covariance, the CSV its two sigma columns); the plan's attribute .align is align_rules' answer."""
    align = align_rules(cfg)
    return _dataset_plan(cfg, loop).with_align(align)


def _dataset_plan(cfg, loop):
    stanford = {"localize_stanford": True, "localize_omniscenes": False}[loop]
    _refuse(cfg, loop, "depth_polish")
    score = score_rules(cfg)
    density_rules(cfg)
    voxel_rules(cfg)
    robust_rules(cfg)
    rooms_polished = stanford and room_polish_rules(cfg)
    polished = None if rooms_polished else polish_rules(cfg, loop)
    room_search = (_cfg(cfg, "room_search", None) or None) if stanford else None
    if pyramid_schedule(cfg) is not None:
        # (the plain route alone: the room searches, the robust and the polished images forms have no coarse-to-fine chain)
        if room_search or polished is not None:
            _refuse(cfg, "a room search" if room_search else "a polished run (cfg.polish_images_per_launch)", "pyramid")
        _needs_parallel(cfg, "pyramid_iters", "coarse-to-fine")
    if room_search:
        if int(_cfg(cfg, "images_per_launch", 1)) > 1:
            raise ValueError("room_search does not combine with images_per_launch > 1: a room search groups its images with room_search_images")
        return DatasetPlan("rooms-polished" if rooms_polished else "rooms", int(_cfg(cfg, "room_search_images", 1)), on(cfg, "parallel"), None,
                           room_search, rooms_polished and on(cfg, "pose_covariance"))
    route = ("scored" if score is not None else "polished" if polished is not None else
             "robust" if _cfg(cfg, "robust_iters", None) is not None else "plain")
    return DatasetPlan(route, group_size(cfg), on(cfg, "parallel"), score, None, on(cfg, "pose_covariance"))
