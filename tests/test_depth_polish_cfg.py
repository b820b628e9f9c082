"""cfg.depth_polish (cfg_rules.depth_polish_flag, its row in cfg_rules' table): every rule with its message, every refusal that exists
without the key unchanged, the accepted combinations accepted — all from dummy arguments, before a device is touched."""
import pytest

from conftest import Cfg


@pytest.fixture(scope="module")
def rules():
    from piccolo_amd import cfg_rules
    return cfg_rules


GN = dict(gn_iters=5)
MASKED = dict(depth_mask=True, depth_polish=True, parallel=True, num_iter=60)


def test_the_switch_alone_and_its_values(rules):
    assert rules.depth_polish_flag(Cfg()) is False and rules.depth_polish_flag(Cfg(depth_polish=None)) is False
    assert rules.depth_polish_flag(Cfg(depth_polish=False, depth_mask=True, gn_iters=3)) is False      # (False is absent: the old refusals hold)
    for v in (1, 0, "yes", 1.0, [True]):
        with pytest.raises(ValueError, match=r"cfg\.depth_polish .*: a bool"):
            rules.depth_polish_flag(Cfg(depth_polish=v, depth_mask=True, gn_iters=3))
    for extra in (GN, dict(pose_covariance=True), dict(gn_iters=5, gn_step_cap=0.05, gn_lambda=1e-2), dict(gn_iters=4, gn_objective="l1", gn_delta=1 / 64),
                  dict(gn_iters=5, pose_covariance=True), dict(gn_iters=5, prune_iters=20, prune_keep=2)):
        assert rules.depth_polish_flag(Cfg(**MASKED, **extra)) is True, extra


def test_what_the_switch_needs(rules):
    with pytest.raises(ValueError, match=r"cfg\.depth_polish goes with cfg\.depth_mask"):
        rules.depth_polish_flag(Cfg(depth_polish=True, **GN))
    with pytest.raises(ValueError, match=r"cfg\.depth_polish goes with cfg\.depth_mask"):
        rules.depth_polish_flag(Cfg(depth_polish=True, depth_mask=False, pose_covariance=True))
    with pytest.raises(ValueError, match=r"cfg\.depth_polish goes with cfg\.gn_iters and / or cfg\.pose_covariance"):
        rules.depth_polish_flag(Cfg(depth_polish=True, depth_mask=True))
    with pytest.raises(ValueError, match=r"cfg\.depth_polish goes with cfg\.gn_iters and / or cfg\.pose_covariance"):
        rules.depth_polish_flag(Cfg(depth_polish=True, depth_mask=True, pose_covariance=False))


def test_what_the_switch_excludes(rules):
    for key, v in (("robust_iters", 4), ("robust_kind", "huber"), ("robust_k", 2.0), ("score_weights", True), ("score_split", [4, 4]),
                   ("score_floor", 0.1), ("score_min_count", 2)):
        with pytest.raises(ValueError, match=r"cfg\.depth_polish does not combine with cfg\.%s" % key):
            rules.depth_polish_flag(Cfg(**MASKED, **GN, **{key: v}))


def test_the_switch_lifts_the_mask_from_the_gn_and_covariance_rules_only(rules):
    """with the switch gn_schedule and pose_covariance_flag answer under the mask what they answer without it; robust_schedule does not"""
    for extra in (dict(gn_iters=5), dict(gn_iters=5, gn_step_cap=0.05, gn_lambda=1e-2), dict(gn_iters=4, gn_objective="l1", gn_delta=1 / 64)):
        assert rules.gn_schedule(Cfg(**MASKED, **extra)) == rules.gn_schedule(Cfg(**extra))
    assert rules.pose_covariance_flag(Cfg(**MASKED, pose_covariance=True)) is True
    with pytest.raises(ValueError, match=r"cfg\.robust_iters does not combine with cfg\.depth_mask"):
        rules.robust_schedule(Cfg(**MASKED, robust_iters=4))
    # the values of the keys are still checked
    with pytest.raises(ValueError, match=r"cfg\.gn_iters 0: an int in 1"):
        rules.gn_schedule(Cfg(**MASKED, gn_iters=0))
    with pytest.raises(ValueError, match=r"cfg\.pose_covariance 1: a bool"):
        rules.pose_covariance_flag(Cfg(**MASKED, pose_covariance=1))


def test_without_the_switch_every_refusal_is_what_it_was(rules):
    for absent in ({}, dict(depth_polish=None), dict(depth_polish=False)):
        with pytest.raises(ValueError) as e:
            rules.gn_schedule(Cfg(depth_mask=True, gn_iters=5, **absent))
        assert str(e.value) == "cfg.gn_iters does not combine with cfg.depth_mask"
        with pytest.raises(ValueError) as e:
            rules.pose_covariance_flag(Cfg(depth_mask=True, pose_covariance=True, **absent))
        assert str(e.value) == "cfg.pose_covariance does not combine with cfg.depth_mask"
        with pytest.raises(ValueError) as e:
            rules.robust_schedule(Cfg(depth_mask=True, robust_iters=4, num_iter=60, **absent))
        assert str(e.value) == "cfg.robust_iters does not combine with cfg.depth_mask"
    # and without the mask the schedules never looked at the switch
    assert rules.gn_schedule(Cfg(gn_iters=5)) == (5, {})
    # the families the entry points refused, in the order they refused them, with the new family behind them
    for who, families in rules.REFUSES.items():
        if who != "omniloc_batch":
            assert families[-1] == "depth_polish" and "depth_polish" not in families[:-1], who
    assert rules.REFUSES["omniloc_batch"] == ()
    assert rules.DatasetPlan._fields == ("route", "group_size", "parallel", "score", "room_search", "sigmas")
    assert "depth_polish" in rules.__doc__


def test_every_other_entry_point_and_both_loops_refuse_the_switch(rules):
    from piccolo_amd import localize, omniloc
    cfg = Cfg(**MASKED, **GN)
    first = {                                                   # the entry points whose first act is _refuse(cfg, their name)
        "omniloc": lambda: omniloc.omniloc(None, None, None, None, None, 0, cfg, None),
        "omniloc_all": lambda: omniloc.omniloc_all(None, None, None, None, None, cfg),
        "omniloc_batch_images": lambda: omniloc.omniloc_batch_images([None], None, None, [None], [None], cfg),
        "omniloc_batch_rooms": lambda: omniloc.omniloc_batch_rooms(None, [None], [None], [None], cfg),
        "omniloc_batch_rooms_images": lambda: omniloc.omniloc_batch_rooms_images([None], [None], [None], [None], cfg),
        "localize_synthetic": lambda: localize.localize_synthetic(cfg),
    }
    for who, call in first.items():
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value).startswith("%s does not take cfg." % who), (who, str(e.value))
    plain = Cfg(depth_mask=True, depth_polish=True, parallel=True)          # (nothing but the switch: it is what gets named)
    for who in first:
        with pytest.raises(ValueError) as e:
            rules._refuse(plain, who)
        assert str(e.value) == "%s does not take cfg.depth_polish (omniloc_batch and localize.refine_image's parallel branch do)" % who
    # the robust and the polished several-image forms: a ValueError before a device, whichever of their rules speaks first
    robust = Cfg(depth_polish=True, depth_mask=True, robust_iters=4, num_iter=60, parallel=True)
    with pytest.raises(ValueError, match="depth_polish|depth_mask"):
        omniloc.omniloc_batch_images_robust([None], None, None, [None], [None], robust)
    with pytest.raises(ValueError, match="depth_polish"):
        omniloc.omniloc_batch_images_polished([None], None, None, [None], [None], cfg)
    with pytest.raises(ValueError, match="depth_polish|depth_mask"):
        omniloc.omniloc_batch_rooms_images_polished([None], [None], [None], [None], cfg)
    for loop in ("localize_stanford", "localize_omniscenes"):
        for extra in ({}, dict(polish_images_per_launch=2), dict(room_search=True, room_search_polish=True)):
            with pytest.raises(ValueError) as e:
                rules.dataset_plan(Cfg(**MASKED, **GN, **extra), loop)
            assert str(e.value) == "%s does not take cfg.depth_polish (omniloc_batch and localize.refine_image's parallel branch do)" % loop
    # refine_image's non-parallel branch is omniloc_all
    with pytest.raises(ValueError, match=r"omniloc_all does not take cfg\."):
        localize.refine_image(None, None, None, None, None, Cfg(depth_mask=True, depth_polish=True, gn_iters=5))


class _Reached(Exception):
    pass


@pytest.fixture()
def batch(monkeypatch):
    """omniloc_batch with everything behind its rules replaced: reaching the box / panorama / chain raises _Reached"""
    from piccolo_amd import omniloc

    def reached(*a, **k):
        raise _Reached()
    for name in ("quantile_box_of", "packed_pano", "packed_cloud", "_refine"):
        monkeypatch.setattr(omniloc, name, reached)
    monkeypatch.setattr(omniloc, "strict_reference_asserts", False)
    return omniloc.omniloc_batch


def test_omniloc_batch_takes_the_accepted_combinations(batch):
    for extra in (GN, dict(pose_covariance=True), dict(gn_iters=5, pose_covariance=True), dict(gn_iters=5, gn_step_cap=0.05, gn_lambda=1e6),
                  dict(gn_iters=4, gn_objective="l1", gn_delta=1 / 64), dict(gn_iters=5, prune_iters=20, prune_keep=2)):
        with pytest.raises(_Reached):
            batch(None, None, None, None, None, Cfg(**MASKED, **extra), None)
    # and goes on taking what it took
    for cfg in (Cfg(depth_mask=True), Cfg(gn_iters=5), Cfg(pose_covariance=True), Cfg()):
        with pytest.raises(_Reached):
            batch(None, None, None, None, None, cfg, None)


def test_omniloc_batch_refuses_before_a_device(batch):
    def msg(cfg, **kw):
        with pytest.raises(ValueError) as e:
            batch(None, None, None, None, None, cfg, None, **kw)
        return str(e.value)
    assert msg(Cfg(depth_polish=True, **GN)).startswith("cfg.depth_polish goes with cfg.depth_mask")
    assert msg(Cfg(depth_polish=True, depth_mask=True)).startswith("cfg.depth_polish goes with cfg.gn_iters and / or cfg.pose_covariance")
    assert msg(Cfg(**MASKED, **GN, robust_iters=4)) == "cfg.depth_polish does not combine with cfg.robust_iters"
    assert msg(Cfg(**MASKED, **GN, score_weights=True)) == "cfg.depth_polish does not combine with cfg.score_weights"
    assert msg(Cfg(**MASKED, **GN), weights=object()) == "cfg.depth_polish does not combine with weights="
    assert msg(Cfg(**MASKED, pose_covariance=True), weights=object()) == "cfg.depth_polish does not combine with weights="
    assert msg(Cfg(depth_polish="on", depth_mask=True, **GN)) == "cfg.depth_polish 'on': a bool"
    # the old ones, word for word
    assert msg(Cfg(depth_mask=True, **GN)) == "cfg.gn_iters does not combine with cfg.depth_mask"
    assert msg(Cfg(depth_mask=True, pose_covariance=True)) == "cfg.pose_covariance does not combine with cfg.depth_mask"
    assert msg(Cfg(depth_mask=True, robust_iters=4, num_iter=60)) == "cfg.robust_iters does not combine with cfg.depth_mask"
