"""cfg.pyramid_iters / cfg.pyramid_reset (cfg_rules.pyramid_schedule, the family "pyramid"): the schedule's values, every refusal with
its words, who takes the keys and who refuses them — all from dummy arguments, before a file is read or a device is touched."""
import os

import pytest

from conftest import REPO, Cfg

TAKERS = "omniloc_batch, omniloc_batch_images and localize.refine_image's parallel branch do; the known-room dataset loops on their plain route"


@pytest.fixture(scope="module")
def rules():
    from piccolo_amd import cfg_rules
    return cfg_rules


def msg(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_the_schedule_and_its_values(rules):
    assert rules.pyramid_schedule(Cfg()) is None and rules.pyramid_schedule(Cfg(pyramid_iters=None, pyramid_reset=None)) is None
    assert rules.pyramid_schedule(Cfg(pyramid_iters=10)) == ([10], False)
    assert rules.pyramid_schedule(Cfg(pyramid_iters=[10, 30], num_iter=100)) == ([10, 30], False)
    assert rules.pyramid_schedule(Cfg(pyramid_iters=(3, 6), num_iter=9, pyramid_reset=True)) == ([3, 6], True)
    assert rules.pyramid_schedule(Cfg(pyramid_iters=[1, 2, 3, 4], num_iter=5, pyramid_reset=False)) == ([1, 2, 3, 4], False)
    # the image's size, where it is known: multiples of 2^levels
    assert rules.pyramid_schedule(Cfg(pyramid_iters=[10, 30]), (1024, 2048)) == ([10, 30], False)
    assert rules.pyramid_schedule(Cfg(pyramid_iters=[10, 30]), (1024, 2048, 3)) == ([10, 30], False)
    assert rules.pyramid_schedule(Cfg(pyramid_iters=[1, 2, 3, 4]), (16, 32)) == ([1, 2, 3, 4], False)
    # it goes with the gn keys, pose_covariance and the grouping keys
    assert rules.pyramid_schedule(Cfg(pyramid_iters=5, gn_iters=4, pose_covariance=True, images_per_launch=8)) == ([5], False)
    assert rules.PYRAMID_KEYS == ("pyramid_iters", "pyramid_reset")
    assert rules._EXTENSIONS["pyramid"] == (rules.PYRAMID_KEYS, None, TAKERS)
    assert "pyramid" in rules.__doc__ and "pyramid_iters" in rules.__doc__


def test_every_refusal_of_the_schedule(rules):
    s = rules.pyramid_schedule
    assert msg(lambda: s(Cfg(pyramid_reset=True))) == "cfg.pyramid_reset goes with cfg.pyramid_iters"
    assert msg(lambda: s(Cfg(pyramid_reset=False))) == "cfg.pyramid_reset goes with cfg.pyramid_iters"
    for bad in ([], "10", 2.5, [3, 2.0], True, [True]):
        assert msg(lambda: s(Cfg(pyramid_iters=bad))).startswith("cfg.pyramid_iters: an int or a list of ints, got "), bad
    for bad, n in (([0], 10), ([10], 10), ([11], 10), ([-1], 10), ([4, 4], 10), ([5, 3], 10), ([100], 100)):
        assert msg(lambda: s(Cfg(pyramid_iters=bad, num_iter=n))) == \
            "cfg.pyramid_iters %r: strictly increasing iteration counts inside (0, %d)" % (bad, n)
    assert msg(lambda: s(Cfg(pyramid_iters=100))) == "cfg.pyramid_iters [100]: strictly increasing iteration counts inside (0, 100)"    # (the default num_iter)
    assert msg(lambda: s(Cfg(pyramid_iters=[1, 2, 3, 4, 5]))) == "cfg.pyramid_iters [1, 2, 3, 4, 5]: at most 4 coarse levels"
    for bad in (1, 0, "yes", [True]):
        assert msg(lambda: s(Cfg(pyramid_iters=5, pyramid_reset=bad))) == "cfg.pyramid_reset %r: a bool" % (bad,)
    assert msg(lambda: s(Cfg(pyramid_iters=5, depth_mask=True))) == "cfg.pyramid_iters does not combine with cfg.depth_mask"
    assert msg(lambda: s(Cfg(pyramid_iters=5, depth_mask=True, depth_polish=True, gn_iters=3))) == "cfg.pyramid_iters does not combine with cfg.depth_mask"
    for key, v in (("robust_iters", 4), ("robust_kind", "huber"), ("robust_k", 2.0), ("score_weights", True), ("score_split", [4, 4]),
                   ("score_floor", 0.1), ("score_min_count", 2), ("density_weights", True), ("density_voxel", 0.1), ("density_cap", 2),
                   ("prune_iters", 20), ("prune_keep", 2)):
        assert msg(lambda: s(Cfg(pyramid_iters=5, **{key: v}))) == "cfg.pyramid_iters does not combine with cfg.%s" % key
    # the image's size
    assert msg(lambda: s(Cfg(pyramid_iters=[10, 30]), (1022, 2048))) == \
        "cfg.pyramid_iters [10, 30]: a 1022 x 2048 image has no 2 coarse levels (H and W must be multiples of 4)"
    assert msg(lambda: s(Cfg(pyramid_iters=[10, 20, 30]), (1024, 2052))) == \
        "cfg.pyramid_iters [10, 20, 30]: a 1024 x 2052 image has no 3 coarse levels (H and W must be multiples of 8)"


def test_what_was_pinned_stays(rules):
    for who, families in rules.REFUSES.items():
        if who != "omniloc_batch":
            assert families[-1] == "depth_polish" and "pyramid" not in families, who
    assert rules.REFUSES["omniloc_batch"] == ()
    assert rules.DatasetPlan._fields == ("route", "group_size", "parallel", "score", "room_search", "sigmas")
    # every other family's words
    assert rules._EXTENSIONS["depth_polish"] == (("depth_polish",), None, "omniloc_batch and localize.refine_image's parallel branch do")
    assert msg(lambda: rules._refuse(Cfg(prune_iters=3), "omniloc")) == "omniloc does not take cfg.prune_iters / cfg.prune_keep (the batch refinements do)"


def test_every_other_entry_point_refuses_the_family_before_a_device(rules):
    from piccolo_amd import localize, omniloc
    for cfg, key in ((Cfg(pyramid_iters=[3, 6], num_iter=9, parallel=True), "pyramid_iters"), (Cfg(pyramid_reset=True, parallel=True), "pyramid_reset")):
        calls = {
            "omniloc": lambda: omniloc.omniloc(None, None, None, None, None, 0, cfg, None),
            "omniloc_all": lambda: omniloc.omniloc_all(None, None, None, None, None, cfg),
            "omniloc_batch_rooms": lambda: omniloc.omniloc_batch_rooms(None, [None], [None], [None], cfg),
            "omniloc_batch_rooms_images": lambda: omniloc.omniloc_batch_rooms_images([None], [None], [None], [None], cfg),
            "omniloc_batch_images_robust": lambda: omniloc.omniloc_batch_images_robust([None], None, None, [None], [None], cfg),
        }
        for who, call in calls.items():
            assert msg(call) == "%s does not take cfg.%s (%s)" % (who, key, TAKERS), who
    # the polished forms want their own keys first; with them, the family is refused
    cfg = Cfg(pyramid_iters=[3, 6], num_iter=9, parallel=True, gn_iters=3)
    assert msg(lambda: omniloc.omniloc_batch_images_polished([None], None, None, [None], [None], cfg)) == \
        "omniloc_batch_images_polished does not take cfg.pyramid_iters (%s)" % TAKERS
    assert msg(lambda: omniloc.omniloc_batch_rooms_images_polished([None], [None], [None], [None], cfg)) == \
        "omniloc_batch_rooms_images_polished does not take cfg.pyramid_iters (%s)" % TAKERS
    # a robust cfg: whichever rule speaks first, a ValueError before a device
    with pytest.raises(ValueError, match="pyramid_iters"):
        omniloc.omniloc_batch_images_robust([None], None, None, [None], [None], Cfg(pyramid_iters=3, robust_iters=4, num_iter=9))
    # refine_image's non-parallel branch is omniloc_all
    assert msg(lambda: localize.refine_image(None, None, None, None, None, Cfg(pyramid_iters=3, num_iter=9))) == \
        "omniloc_all does not take cfg.pyramid_iters (%s)" % TAKERS


def test_the_dataset_loops(rules):
    base = dict(pyramid_iters=[10, 30], num_iter=100, parallel=True)
    for loop in ("localize_stanford", "localize_omniscenes"):
        for ipl in (1, 2, 8):
            plan = rules.dataset_plan(Cfg(**base, images_per_launch=ipl), loop)
            assert plan.route == "plain" and plan.group_size == ipl and plan.parallel is True
            assert plan == rules.dataset_plan(Cfg(parallel=True, images_per_launch=ipl), loop)        # the plan itself does not change
        assert msg(lambda: rules.dataset_plan(Cfg(pyramid_iters=[10, 30], num_iter=100), loop)) == \
            "cfg.pyramid_iters needs cfg.parallel (the coarse-to-fine chain has parallel semantics only)"
        assert msg(lambda: rules.dataset_plan(Cfg(**base, polish_images_per_launch=2, gn_iters=3), loop)) == \
            "a polished run (cfg.polish_images_per_launch) does not take cfg.pyramid_iters (%s)" % TAKERS
        for extra, key in ((dict(robust_iters=4), "robust_iters"), (dict(score_weights=True), "score_weights"),
                           (dict(density_weights=True, density_voxel=0.1), "density_weights"), (dict(prune_iters=20, prune_keep=2), "prune_iters")):
            assert msg(lambda: rules.dataset_plan(Cfg(**base, **extra), loop)) == "cfg.pyramid_iters does not combine with cfg.%s" % key
        assert msg(lambda: rules.dataset_plan(Cfg(**base, depth_mask=True), loop)) == "cfg.pyramid_iters does not combine with cfg.depth_mask"
        assert msg(lambda: rules.dataset_plan(Cfg(pyramid_iters=[30, 10], parallel=True), loop)).startswith("cfg.pyramid_iters [30, 10]: strictly")
    # the room searches refuse the keys (localize_omniscenes ignores the room-search keys: a plain run there)
    for extra in (dict(room_search=True), dict(room_search=True, room_search_images=4), dict(room_search=True, room_search_polish=True, gn_iters=3)):
        assert msg(lambda: rules.dataset_plan(Cfg(**base, **extra), "localize_stanford")) == \
            "a room search does not take cfg.pyramid_iters (%s)" % TAKERS


class _Reached(Exception):
    pass


@pytest.fixture()
def front(monkeypatch):
    """omniloc with everything behind its rules replaced: reaching the box / a panorama / a cloud / the chain raises _Reached"""
    from piccolo_amd import omniloc

    def reached(*a, **k):
        raise _Reached()
    for name in ("quantile_box_of", "packed_pano", "packed_cloud", "packed_cloud_sets", "_chain_panos", "_refine"):
        monkeypatch.setattr(omniloc, name, reached)
    monkeypatch.setattr(omniloc, "strict_reference_asserts", False)
    return omniloc


class _Shaped:
    def __init__(self, *shape):
        self.shape = shape


def test_the_entry_points_that_take_the_keys(front):
    img = _Shaped(64, 128, 3)
    for extra in ({}, dict(pyramid_reset=True), dict(gn_iters=4), dict(pose_covariance=True), dict(gn_iters=4, gn_objective="l1", pose_covariance=True)):
        with pytest.raises(_Reached):
            front.omniloc_batch(img, None, None, None, None, Cfg(pyramid_iters=[3, 6], num_iter=9, **extra), None)
    with pytest.raises(_Reached):
        front.omniloc_batch_images([img, img], _Shaped(10, 3), None, [_Shaped(4, 3)] * 2, [_Shaped(4, 3)] * 2, Cfg(pyramid_iters=[3, 6], num_iter=9))
    # ... and refuse, before a device: weights=, a bad schedule, an image size that has no such levels
    assert msg(lambda: front.omniloc_batch(img, None, None, None, None, Cfg(pyramid_iters=3, num_iter=9), None, weights=object())) == \
        "cfg.pyramid_iters does not combine with weights="
    assert msg(lambda: front.omniloc_batch(img, None, None, None, None, Cfg(pyramid_iters=9, num_iter=9), None)).startswith("cfg.pyramid_iters [9]: strictly")
    assert msg(lambda: front.omniloc_batch(_Shaped(62, 128, 3), None, None, None, None, Cfg(pyramid_iters=[3, 6], num_iter=9), None)) == \
        "cfg.pyramid_iters [3, 6]: a 62 x 128 image has no 2 coarse levels (H and W must be multiples of 4)"
    assert msg(lambda: front.omniloc_batch_images([_Shaped(64, 130, 3)] * 2, None, None, [None] * 2, [None] * 2, Cfg(pyramid_iters=[3, 6], num_iter=9))) == \
        "cfg.pyramid_iters [3, 6]: a 64 x 130 image has no 2 coarse levels (H and W must be multiples of 4)"
    for extra, key in ((dict(robust_iters=4), "robust_iters"), (dict(prune_iters=4, prune_keep=2), "prune_iters"), (dict(depth_mask=True), "depth_mask"),
                       (dict(score_weights=True), "score_weights"), (dict(density_weights=True, density_voxel=0.1), "density_weights")):
        assert msg(lambda: front.omniloc_batch(img, None, None, None, None, Cfg(pyramid_iters=3, num_iter=9, **extra), None)) == \
            "cfg.pyramid_iters does not combine with cfg.%s" % key, key
    # without the keys nothing is asked
    with pytest.raises(_Reached):
        front.omniloc_batch(None, None, None, None, None, Cfg(), None)


def test_the_shipped_config_parses_into_a_schedule(rules):
    from piccolo_amd.parse_utils import parse_ini
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32_pyramid.ini"))
    assert cfg.num_input == 32 and cfg.parallel is True and cfg.num_iter == 100
    assert rules.pyramid_schedule(cfg, (1024, 2048)) == ([10, 30], False)
    plan = rules.dataset_plan(cfg, "localize_stanford")
    assert plan.route == "plain" and plan.parallel is True
    base = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini"))
    differ = {k for k in cfg._fields if getattr(cfg, k) != getattr(base, k, None)}
    assert differ == {"pyramid_iters", "pyramid_reset"}
