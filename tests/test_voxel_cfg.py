"""CPU checks of the voxel and density configuration: cfg_rules.voxel_rules / density_rules read their keys and refuse every malformed one
and every combination the density-weighted known-room path does not run (with the exact messages of the exclusions), dataset_plan keeps
its six fields and routes a density run "plain", the dataset loops raise before they read a file, the entry points that do not take
the keys refuse them before they touch a device, and each shipped config is the b32 one plus the stated keys."""
import os

import pytest
import torch

from conftest import REPO, Cfg


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    kw.setdefault("num_input", 6)
    kw.setdefault("parallel", True)
    return Cfg(**kw)


@pytest.fixture(scope="module")
def rules():
    from piccolo_amd import cfg_rules
    return cfg_rules


# ------------------------------------------------------------------------------------------------ accepted forms
def test_voxel_rules_reads_the_keys(rules):
    assert rules.voxel_rules(_cfg()) is None
    assert rules.voxel_rules(_cfg(voxel_size=None, voxel_how=None)) is None
    assert rules.voxel_rules(_cfg(voxel_size=0.05)) == (0.05, "centroid")
    assert rules.voxel_rules(_cfg(voxel_size=1)) == (1.0, "centroid")
    assert rules.voxel_rules(_cfg(voxel_size=0.02, voxel_how="centroid")) == (0.02, "centroid")
    assert rules.voxel_rules(_cfg(voxel_size=0.02, voxel_how="first")) == (0.02, "first")
    assert rules.VOXEL_KEYS == ("voxel_size", "voxel_how") and rules.VOXEL_HOW == ("centroid", "first")
    # the down-sampled cloud is a cloud: the key stands next to every other family
    for other in (dict(images_per_launch=4), dict(robust_iters=20), dict(room_search=True, room_search_images=2), dict(depth_mask=True),
                  dict(score_weights=True), dict(gn_iters=5, polish_images_per_launch=4), dict(density_weights=True, density_voxel=0.05)):
        plan = rules.dataset_plan(_cfg(voxel_size=0.05, **other), "localize_stanford")
        assert plan._fields == ("route", "group_size", "parallel", "score", "room_search", "sigmas")


def test_density_rules_reads_the_keys(rules):
    assert rules.density_rules(_cfg()) is None
    assert rules.density_rules(_cfg(density_weights=None, density_voxel=None, density_cap=None)) is None
    assert rules.density_rules(_cfg(density_weights=False)) is None
    assert rules.density_rules(_cfg(density_weights=True, density_voxel=0.05)) == (0.05, 1)
    assert rules.density_rules(_cfg(density_weights=True, density_voxel=2, density_cap=3)) == (2.0, 3)
    assert rules.density_rules(_cfg(density_weights=True, density_voxel=0.02, density_cap=1, images_per_launch=1, depth_mask=False,
                                    room_search=None, parallel=False)) == (0.02, 1)
    assert rules.DENSITY_KEYS == ("density_weights", "density_voxel", "density_cap")
    assert rules._EXTENSIONS["density"][0] == rules.DENSITY_KEYS and rules._EXTENSIONS["voxel"][0] == rules.VOXEL_KEYS
    assert "density" in rules.__doc__ and "voxel_size" in rules.__doc__


def test_dataset_plan_keeps_its_fields_and_routes_density_plain(rules):
    assert rules.DatasetPlan._fields == ("route", "group_size", "parallel", "score", "room_search", "sigmas")
    for loop in ("localize_stanford", "localize_omniscenes"):
        plan = rules.dataset_plan(_cfg(density_weights=True, density_voxel=0.05, density_cap=2), loop)
        assert plan == rules.DatasetPlan("plain", 1, True, None, None, False)
        assert rules.dataset_plan(_cfg(density_weights=True, density_voxel=0.05, parallel=False), loop).parallel is False
        assert rules.dataset_plan(_cfg(voxel_size=0.05, voxel_how="first", images_per_launch=4), loop) == \
            rules.DatasetPlan("plain", 4, True, None, None, False)
        # with pruning, which every batch refinement takes
        assert rules.dataset_plan(_cfg(density_weights=True, density_voxel=0.05, prune_iters=20, prune_keep=3), loop).route == "plain"
    # every entry point that refuses the score family refuses the density family, right behind it; omniloc_batch takes both
    for who, families in rules.REFUSES.items():
        assert ("score" in families) == ("density" in families), who
        if "score" in families:
            assert families.index("density") == families.index("score") + 1, who
    assert rules.REFUSES["omniloc_batch"] == () and "voxel" in rules.REFUSES["localize_synthetic"]
    assert [who for who, families in rules.REFUSES.items() if "voxel" in families] == ["localize_synthetic"]


# ------------------------------------------------------------------------------------------------ refusals
ON = dict(density_weights=True, density_voxel=0.05)
BAD = [
    # the voxel keys
    (dict(voxel_how="first"), "cfg.voxel_how goes with cfg.voxel_size"),
    (dict(voxel_size=0), "cfg.voxel_size 0: a positive finite number"),
    (dict(voxel_size=-0.05), "cfg.voxel_size -0.05: a positive finite number"),
    (dict(voxel_size=float("inf")), "cfg.voxel_size inf: a positive finite number"),
    (dict(voxel_size=float("nan")), "cfg.voxel_size nan: a positive finite number"),
    (dict(voxel_size="0.05"), "cfg.voxel_size '0.05': a positive finite number"),
    (dict(voxel_size=True), "cfg.voxel_size True: a positive finite number"),
    (dict(voxel_size=[0.05]), "cfg.voxel_size [0.05]: a positive finite number"),
    (dict(voxel_size=0.05, voxel_how="mean"), "cfg.voxel_how 'mean': one of ['centroid', 'first']"),
    (dict(voxel_size=0.05, voxel_how=1), "cfg.voxel_how 1: one of ['centroid', 'first']"),
    # the density keys without the switch, and malformed
    (dict(density_voxel=0.05), "cfg.density_voxel goes with cfg.density_weights = True"),
    (dict(density_cap=2), "cfg.density_cap goes with cfg.density_weights = True"),
    (dict(density_weights=False, density_voxel=0.05), "cfg.density_voxel goes with cfg.density_weights = True"),
    (dict(density_weights=1, density_voxel=0.05), "cfg.density_weights 1: a bool"),
    (dict(density_weights="True", density_voxel=0.05), "cfg.density_weights 'True': a bool"),
    (dict(density_weights=True), "cfg.density_weights goes with cfg.density_voxel (the voxel's edge in metres)"),
    (dict(density_weights=True, density_cap=2), "cfg.density_weights goes with cfg.density_voxel (the voxel's edge in metres)"),
    (dict(density_weights=True, density_voxel=0), "cfg.density_voxel 0: a positive finite number"),
    (dict(density_weights=True, density_voxel=-1.0), "cfg.density_voxel -1.0: a positive finite number"),
    (dict(density_weights=True, density_voxel=float("inf")), "cfg.density_voxel inf: a positive finite number"),
    (dict(density_weights=True, density_voxel="0.05"), "cfg.density_voxel '0.05': a positive finite number"),
    (dict(density_weights=True, density_voxel=True), "cfg.density_voxel True: a positive finite number"),
    (dict(ON, density_cap=0), "cfg.density_cap 0: an int >= 1"),
    (dict(ON, density_cap=2.0), "cfg.density_cap 2.0: an int >= 1"),
    (dict(ON, density_cap=True), "cfg.density_cap True: an int >= 1"),
    # what the density-weighted path does not combine with: what the score keys exclude, and the score keys
    (dict(ON, images_per_launch=4), "cfg.density_weights does not combine with images_per_launch > 1 (one image per launch chain)"),
    (dict(ON, score_weights=True), "cfg.density_weights does not combine with cfg.score_weights"),
    (dict(ON, robust_iters=20), "cfg.density_weights does not combine with cfg.robust_iters"),
    (dict(ON, robust_kind="huber"), "cfg.density_weights does not combine with cfg.robust_kind"),
    (dict(ON, robust_k=2.5), "cfg.density_weights does not combine with cfg.robust_k"),
    (dict(ON, robust_images_per_launch=4), "cfg.density_weights does not combine with cfg.robust_images_per_launch"),
    (dict(ON, gn_iters=5, polish_images_per_launch=4), "cfg.density_weights does not combine with cfg.polish_images_per_launch"),
    (dict(ON, room_search=True), "cfg.density_weights does not combine with cfg.room_search"),
    (dict(ON, room_search=["office_1"]), "cfg.density_weights does not combine with cfg.room_search"),
    (dict(ON, room_search_images=4), "cfg.density_weights does not combine with cfg.room_search_images"),
    (dict(ON, depth_mask=True), "cfg.density_weights does not combine with cfg.depth_mask"),
]


@pytest.mark.parametrize("kw,message", BAD)
def test_rules_and_loops_refuse_at_configuration_time(rules, kw, message, tmp_path):
    """the exact message from the rule, and the dataset loops raise a ValueError before they read a file: the root does not even exist"""
    from piccolo_amd import localize
    cfg = _cfg(**kw)
    rule = rules.voxel_rules if any(k.startswith("voxel") for k in kw) else rules.density_rules
    with pytest.raises(ValueError) as e:
        rule(cfg)
    assert str(e.value) == message
    root = str(tmp_path / "nowhere")
    for loop in ("localize_stanford", "localize_omniscenes"):
        with pytest.raises(ValueError):
            rules.dataset_plan(cfg, loop)
        with pytest.raises(ValueError):
            getattr(localize, loop)(cfg, None, None, root)
    assert not os.path.exists(root)


def test_score_keys_beside_the_density_switch_are_refused_by_name(rules):
    for key, value in (("score_split", [16, 32]), ("score_floor", 0.25), ("score_min_count", 2)):
        with pytest.raises(ValueError) as e:
            rules.density_rules(_cfg(score_weights=True, **{key: value}, **ON))
        assert str(e.value) == "cfg.density_weights does not combine with cfg.score_weights"
    # the loops' polish keys need their group key, which the family excludes: refused one way or the other
    for extra in (dict(gn_iters=5), dict(pose_covariance=True)):
        with pytest.raises(ValueError):
            rules.dataset_plan(_cfg(**extra, **ON), "localize_stanford")


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


@pytest.mark.parametrize("key,value", [("density_weights", True), ("density_voxel", 0.05), ("density_cap", 2)])
def test_entry_points_that_do_not_take_the_density_keys_refuse_them(key, value):
    """the several-image and rooms entry points and the synthetic driver raise before they touch a device"""
    from piccolo_amd import localize, omniloc as po
    cfg = _cfg(num_input=4, **{key: value})
    two = [Z.clone(), Z.clone()]
    with pytest.raises(ValueError, match="omniloc_batch_images does not take cfg.%s" % key):
        po.omniloc_batch_images([IMG, IMG], Z, Z, two, two, cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_images_robust([IMG, IMG], Z, Z, two, two, _cfg(num_input=4, robust_iters=20, **{key: value}))
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_images_polished([IMG, IMG], Z, Z, two, two, _cfg(num_input=4, gn_iters=5, **{key: value}))
    with pytest.raises(ValueError, match="omniloc_batch_rooms does not take cfg.%s" % key):
        po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], two, two, cfg)
    with pytest.raises(ValueError, match="omniloc_batch_rooms_images does not take cfg.%s" % key):
        po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_rooms_images_polished([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], _cfg(num_input=4, gn_iters=5, **{key: value}))
    with pytest.raises(ValueError, match="localize_synthetic does not take cfg.%s" % key):
        localize.localize_synthetic(cfg)


@pytest.mark.parametrize("key,value", [("voxel_size", 0.05), ("voxel_how", "first")])
def test_localize_synthetic_refuses_the_voxel_keys(key, value):
    from piccolo_amd import localize
    with pytest.raises(ValueError, match="localize_synthetic does not take cfg.%s" % key):
        localize.localize_synthetic(_cfg(**{key: value}))


def test_without_the_keys_nothing_is_refused(rules):
    rules._refuse(_cfg(), "anything", "density", "voxel")
    rules._refuse(_cfg(density_weights=None, density_voxel=None, density_cap=None, voxel_size=None, voxel_how=None), "anything", "density", "voxel")
    rules._refuse(_cfg(density_weights=True, density_voxel=0.05, voxel_size=0.05), "omniloc_batch")


# ------------------------------------------------------------------------------------------------ shipped configs
@pytest.mark.parametrize("name,extra", [("voxel", dict(voxel_size=0.02)), ("density", dict(density_weights=True, density_voxel=0.02))])
def test_shipped_config_is_b32_plus_the_stated_keys(rules, name, extra):
    from piccolo_amd.parse_utils import parse_ini
    b32 = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini"))._asdict()
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32_%s.ini" % name))
    got = cfg._asdict()
    assert {k: v for k, v in got.items() if k not in b32} == extra
    assert {k: v for k, v in got.items() if k in b32} == b32
    assert rules.voxel_rules(cfg) == ((0.02, "centroid") if name == "voxel" else None)
    assert rules.density_rules(cfg) == ((0.02, 1) if name == "density" else None)
    assert rules.dataset_plan(cfg, "localize_stanford") == rules.DatasetPlan("plain", 1, True, None, None, False)
    assert cfg.lr == 0.1 and cfg.num_iter == 100 and cfg.patience == 5 and cfg.factor == 0.8
